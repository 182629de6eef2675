"""CPU expectation for guided upsampling (include/rgk.h rgk_upsample_device), for test_upsample_cpu.py / test_gpu_upsample.py.

* `upsample_ref`: k_us_prepare + k_us_gather (rgk_amd/csrc/rgk_post.hip) restated in numpy float32, the same operations in the same
  order -- with contraction off on both sides they give the kernels' bits.  A tap that does not count adds +0 to every sum, which
  changes no bit of a sum that started at +0.
* `project_low`: the projection of the full grid's pixels into the low grid (steps 1 and 2 of the definition).
* `bilinear_ref`: a plain bilinear upscale of the low image through the same projection, taps clamped to the frame, no guide: what
  the guided stage is measured against.

Cameras are what temporal_ref's helpers take: anything with origin, direction, viewscreen, viewscreen_x, viewscreen_y.
"""
import numpy as np

from temporal_ref import F, _dot, _len, _v, camera_rays


def low_records(cam_low, accum, count, albedo, normal, depth, demodulate=1, albedo_floor=0.02):
    """Per low pixel: (c, m, live, flat, x_q) -- k_us_prepare."""
    yl, xl = depth.shape
    cnt = count.astype(np.uint32)
    live = cnt > 0
    c = np.zeros((yl, xl, 3), F)
    c[live] = accum.astype(F)[live] / cnt[live].astype(F)[:, None]
    if demodulate:
        div = np.where(albedo > 0, np.fmax(albedo.astype(F), F(albedo_floor)), F(1)).astype(F)
    else:
        div = np.ones((yl, xl, 3), F)
    m = (c / div).astype(F)
    normal = normal.astype(F)
    flat = (normal[..., 0] == 0) & (normal[..., 1] == 0) & (normal[..., 2] == 0)
    o_low, d_low = camera_rays(cam_low, xl, yl)
    xq = (o_low + d_low * depth.astype(F)[..., None]).astype(F)
    return c, m, live, flat, xq


def project_low(cam, cam_low, normal, depth, xl, yl):
    """(x_p, flat_p, len(x_p - o), qd, fx, fy) per full pixel, float32 (fx, fy meaningless where !(qd > 0))."""
    yres, xres = depth.shape
    o, d = camera_rays(cam, xres, yres)
    normal = normal.astype(F)
    flat = (normal[..., 0] == 0) & (normal[..., 1] == 0) & (normal[..., 2] == 0)
    o_low, N = _v(cam_low, "origin"), _v(cam_low, "direction")
    vs, vx, vy = _v(cam_low, "viewscreen"), _v(cam_low, "viewscreen_x"), _v(cam_low, "viewscreen_y")
    xp = (o + d * depth.astype(F)[..., None]).astype(F)
    v = np.where(flat[..., None], d, xp - o_low).astype(F)
    qd = _dot(v, N)
    s = _dot(vs - o_low, N) / qd
    w = (o_low + v * s[..., None]) - vs
    a = _dot(w, vx) / _dot(vx, vx)
    b = _dot(w, vy) / _dot(vy, vy)
    fx = a * F(xl) - F(0.5)
    fy = b * F(yl) - F(0.5)
    return xp, flat, _len((xp - o).astype(F)), qd, fx, fy


def upsample_ref(cam, albedo, normal, depth, cam_low, low_accum, low_count, low_albedo, low_normal, low_depth,
                 plane_tol=0.01, normal_cos=0.9, demodulate=1, albedo_floor=0.02):
    """(out (y, x, 3) float32, support (y, x) uint8)."""
    yres, xres = depth.shape
    yl, xl = low_depth.shape
    old = np.seterr(all="ignore")
    try:
        c, m, live, flat_q, xq = low_records(cam_low, low_accum, low_count, low_albedo, low_normal, low_depth, demodulate, albedo_floor)
        nq_all = low_normal.astype(F)
        npl = normal.astype(F)
        xp, flat_p, lenp, qd, fx, fy = project_low(cam, cam_low, npl, depth, xl, yl)
        ok = (qd > 0) & (fx > F(-2)) & (fx < F(xl + 1)) & (fy > F(-2)) & (fy < F(yl + 1))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        flx, fly = np.floor(fxs), np.floor(fys)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = fxs - flx, fys - fly
        tol = F(plane_tol) * lenp
        one = F(1)

        def ring(taps):
            """taps: [(qx, qy, w)] in tap order -> (A, W)."""
            A = np.zeros((yres, xres, 3), F)
            W = np.zeros((yres, xres), F)
            for qx, qy, w in taps:
                inside = ok & (qx >= 0) & (qx < xl) & (qy >= 0) & (qy < yl)
                cx, cy = np.clip(qx, 0, xl - 1), np.clip(qy, 0, yl - 1)
                nq = nq_all[cy, cx]
                surf = (_dot(npl, nq) >= F(normal_cos)) & (np.abs(_dot(xq[cy, cx] - xp, npl)) <= tol)
                counted = inside & live[cy, cx] & (flat_q[cy, cx] == flat_p) & (flat_p | surf)
                wk = np.where(counted, w, F(0)).astype(F)
                W = W + wk
                A = A + np.where(counted[..., None], wk[..., None] * m[cy, cx], F(0)).astype(F)
            return A, W

        A1, W1 = ring([(ix, iy, (one - tx) * (one - ty)), (ix + 1, iy, tx * (one - ty)), (ix, iy + 1, (one - tx) * ty), (ix + 1, iy + 1, tx * ty)])
        taps2 = []
        for dy in range(-1, 3):
            for dx in range(-1, 3):
                qx, qy = ix + dx, iy + dy
                ex, ey = fxs - qx.astype(F), fys - qy.astype(F)
                taps2.append((qx, qy, one / (one + (ex * ex + ey * ey))))
        A2, W2 = ring(taps2)
        have1 = ok & (W1 > 0)
        have2 = ok & ~have1 & (W2 > 0)
        if demodulate:
            divp = np.where(albedo > 0, np.fmax(albedo.astype(F), F(albedo_floor)), F(1)).astype(F)
        else:
            divp = np.ones((yres, xres, 3), F)
        nx = np.clip(np.floor(fxs + F(0.5)).astype(np.int64), 0, xl - 1)
        ny = np.clip(np.floor(fys + F(0.5)).astype(np.int64), 0, yl - 1)
        out = np.where(ok[..., None], c[ny, nx], F(0)).astype(F)
        out = np.where(have2[..., None], (A2 / W2[..., None]) * divp, out)
        out = np.where(have1[..., None], (A1 / W1[..., None]) * divp, out).astype(F)
        support = np.where(have1, 1, np.where(have2, 2, 0)).astype(np.uint8)
    finally:
        np.seterr(**old)
    return out, support


def bilinear_ref(cam, normal, depth, cam_low, low_image):
    """The low IMAGE (y, x, 3) sampled bilinearly at every full pixel's projection, taps clamped to the frame, float32; pixels
    whose projection is not in front of the low camera get 0."""
    yl, xl = low_image.shape[:2]
    old = np.seterr(all="ignore")
    try:
        _, _, _, qd, fx, fy = project_low(cam, cam_low, normal, depth, xl, yl)
        ok = (qd > 0) & np.isfinite(fx) & np.isfinite(fy)
        fxs = np.clip(np.where(ok, fx, F(0)), F(0), F(xl - 1))
        fys = np.clip(np.where(ok, fy, F(0)), F(0), F(yl - 1))
        ix, iy = np.floor(fxs).astype(np.int64), np.floor(fys).astype(np.int64)
        tx, ty = (fxs - ix.astype(F))[..., None], (fys - iy.astype(F))[..., None]
        x1, y1 = np.minimum(ix + 1, xl - 1), np.minimum(iy + 1, yl - 1)
        img = low_image.astype(F)
        top = img[iy, ix] * (F(1) - tx) + img[iy, x1] * tx
        bot = img[y1, ix] * (F(1) - tx) + img[y1, x1] * tx
        out = np.where(ok[..., None], top * (F(1) - ty) + bot * ty, F(0)).astype(F)
    finally:
        np.seterr(**old)
    return out
