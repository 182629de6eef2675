"""CPU expectations for temporal reuse (include/rgk.h rgk_temporal_reproject_device / rgk_temporal_blend_device), for
test_temporal_cpu.py / test_gpu_temporal.py.

* `camera_rays`: camera_ray() (rgk_amd/csrc/rgk_trace.h) of a pinhole camera through every pixel centre, restated in float32.
* `reproject_ref`, `blend_ref`: k_tp_reproject / k_tp_blend (rgk_amd/csrc/rgk_post.hip) restated in numpy float32, the same
  operations in the same order -- with contraction off on both sides they give the kernels' bits.  A tap that does not count
  adds +0 to every sum, which changes no bit of a sum that started at +0.
* `tri_kinds`: the top-level material kind of every triangle of a scene descriptor.

A camera is anything with the members origin, direction, viewscreen, viewscreen_x, viewscreen_y (three floats each): a
capi.Camera, or the SimpleNamespace `pinhole_camera` makes for the synthetic cases.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np

F = np.float32
SPECULAR_KINDS = (1, 2, 3)  # RGK_BXDF_MIRROR, RGK_BXDF_DIELECTRIC, RGK_BXDF_TRANSPARENT


def _v(cam, name):
    return np.array([F(x) for x in getattr(cam, name)], F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _len(v):
    return np.sqrt(_dot(v, v))


def _norm(v):
    return v * (F(1) / np.sqrt(_dot(v, v)))[..., None]


def pinhole_camera(pos, lookat, up, xview, yview):
    """A camera from explicit values, for the synthetic cases (their own meaning is tested, not Camera::Camera): the view
    screen is the unit-distance plane in front of `pos`, xview wide and yview high, its corner at pixel (0, 0)'s top left."""
    pos, lookat, up = (np.array(a, F) for a in (pos, lookat, up))
    d = _norm(lookat - pos)
    left = _norm(np.cross(up, d).astype(F))
    cup = np.cross(d, left).astype(F)
    vx = (-left * F(xview)).astype(F)
    vy = (-cup * F(yview)).astype(F)
    vs = (pos + d - F(0.5) * vx - F(0.5) * vy).astype(F)
    return SimpleNamespace(origin=pos, direction=d, viewscreen=vs, viewscreen_x=vx, viewscreen_y=vy)


def camera_rays(cam, xres, yres):
    """(o (3,), d (yres, xres, 3)): camera_ray at offset (0.5, 0.5) with no lens."""
    o, vs, vx, vy = _v(cam, "origin"), _v(cam, "viewscreen"), _v(cam, "viewscreen_x"), _v(cam, "viewscreen_y")
    fx = (np.arange(xres).astype(F) + F(0.5)) / F(xres)
    fy = (np.arange(yres).astype(F) + F(0.5)) / F(yres)
    p = (vs + fx[None, :, None] * vx) + fy[:, None, None] * vy
    return o, _norm((p - o).astype(F))


def tri_kinds(desc):
    """Material kind per triangle of a capi.SceneDesc."""
    nt = desc.n_triangles
    tmat = np.ctypeslib.as_array(C.cast(desc.tri_material, C.POINTER(C.c_uint32)), shape=(nt,)).copy()
    kinds = np.array([desc.materials[i].kind for i in range(desc.n_materials)], np.uint32)
    return kinds[tmat]


def project_ref(cam_cur, cam_prev, depth, tri, xres, yres):
    """The first half of the kernel: (x_p, v, len(v), q, fx, fy) per pixel, float32 (fx, fy meaningless where !(q > 0))."""
    o, d = camera_rays(cam_cur, xres, yres)
    o_prev, N = _v(cam_prev, "origin"), _v(cam_prev, "direction")
    vs, vx, vy = _v(cam_prev, "viewscreen"), _v(cam_prev, "viewscreen_x"), _v(cam_prev, "viewscreen_y")
    hit = tri >= 0
    xp = o + d * depth.astype(F)[..., None]
    v = np.where(hit[..., None], xp - o_prev, d).astype(F)
    q = _dot(v, N)
    s = _dot(vs - o_prev, N) / q
    w = (o_prev + v * s[..., None]) - vs
    a = _dot(w, vx) / _dot(vx, vx)
    b = _dot(w, vy) / _dot(vy, vy)
    fx = a * F(xres) - F(0.5)
    fy = b * F(yres) - F(0.5)
    return xp, v, _len(v), q, fx, fy


def reproject_ref(cam_cur, cam_prev, depth, normal, tri, depth_prev, normal_prev, tri_prev, hist_rgb_prev, hist_len_prev, kinds,
                  plane_tol=0.01, normal_cos=0.9, want_taps=False):
    """(hist_rgb (y, x, 3), hist_len (y, x)) float32.  `kinds`: material kind per triangle id (a triangle id beyond it gets no
    history).  want_taps: also the number of counted taps per pixel."""
    yres, xres = depth.shape
    old = np.seterr(all="ignore")
    try:
        normal, normal_prev = normal.astype(F), normal_prev.astype(F)
        xp, v, lenv, q, fx, fy = project_ref(cam_cur, cam_prev, depth, tri, xres, yres)
        hit = tri >= 0
        known = hit & (tri < len(kinds))
        kind = np.asarray(kinds)[np.where(known, tri, 0)] if len(kinds) else np.zeros(tri.shape, np.uint32)
        zero_n = (normal[..., 0] == 0) & (normal[..., 1] == 0) & (normal[..., 2] == 0)
        ok = ~hit | (known & ~zero_n & ~np.isin(kind, SPECULAR_KINDS))
        ok &= q > 0
        ok &= (fx > F(-1)) & (fx < F(xres)) & (fy > F(-1)) & (fy < F(yres))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        flx, fly = np.floor(fxs), np.floor(fys)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = fxs - flx, fys - fly
        one = F(1)
        wt = [(one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty]
        tol = F(plane_tol) * lenv
        o_prev = _v(cam_prev, "origin")
        _, d_prev = camera_rays(cam_prev, xres, yres)
        x_prev = o_prev + d_prev * depth_prev.astype(F)[..., None]
        sc = np.zeros((yres, xres, 3), F)
        sl = np.zeros((yres, xres), F)
        sw = np.zeros((yres, xres), F)
        ntaps = np.zeros((yres, xres), np.int32)
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            inside = ok & (qx >= 0) & (qx < xres) & (qy >= 0) & (qy < yres)
            cx, cy = np.clip(qx, 0, xres - 1), np.clip(qy, 0, yres - 1)
            lq = hist_len_prev.astype(F)[cy, cx]
            hq = tri_prev[cy, cx] >= 0
            nq = normal_prev[cy, cx]
            dist = np.abs(_dot(xp - x_prev[cy, cx], nq))
            surf = (_dot(normal, nq) >= F(normal_cos)) & (dist <= tol)
            counted = inside & (lq > 0) & (hq == hit) & (~hit | surf)
            w = np.where(counted, wt[k], F(0)).astype(F)
            c = hist_rgb_prev.astype(F)[cy, cx]
            sc = sc + np.where(counted[..., None], w[..., None] * c, F(0)).astype(F)
            sl = sl + np.where(counted, w * lq, F(0)).astype(F)
            sw = sw + w
            ntaps += counted
        have = sw > 0
        rgb = np.where(have[..., None], sc / sw[..., None], F(0)).astype(F)
        length = np.where(have, sl / sw, F(0)).astype(F)
    finally:
        np.seterr(**old)
    return (rgb, length, ntaps) if want_taps else (rgb, length)


def blend_ref(accum, count, albedo, hist_rgb, hist_len, alpha_min=0.1, max_len=10.0, demodulate=1, albedo_floor=0.02):
    """(out_hist_rgb, out_hist_len, out_rgb) float32."""
    old = np.seterr(all="ignore")
    try:
        cnt = count.astype(np.uint32)
        some = cnt > 0
        c = np.zeros(accum.shape, F)
        c[some] = accum.astype(F)[some] / cnt[some].astype(F)[:, None]
        if demodulate:
            div = np.where(albedo > 0, np.fmax(albedo.astype(F), F(albedo_floor)), F(1)).astype(F)
        else:
            div = np.ones(accum.shape, F)
        m = c / div
        h, L = hist_rgb.astype(F), hist_len.astype(F)
        alpha = np.fmax(F(1) / (L + F(1)), F(alpha_min))
        mixed = (m - h) * alpha[..., None] + h
        has = L > 0
        m1 = np.where(has[..., None], mixed, m)
        L1 = np.where(has, np.fmin(L + F(1), F(max_len)), F(1))
        m1 = np.where(some[..., None], m1, h).astype(F)
        L1 = np.where(some, L1, L).astype(F)
        out = (m1 * div).astype(F)
    finally:
        np.seterr(**old)
    return m1, L1, out
