"""CPU expectations for the feature pass and the a-trous denoiser (include/rgk.h), for test_post_cpu.py / test_gpu_post.py.

* `atrous_ref`: the filter restated in numpy float32, the same operations in the same order as k_dn_prepare / k_dn_atrous /
  k_dn_finish (rgk_amd/csrc/rgk_post.hip) -- with contraction off on both sides it gives the kernels' bits.
* `oracle_features`: albedo / normal / depth / triangle planes composed from the oracle library's orc_camera_ray,
  orc_trace_closest and orc_texture_sample, with surface_point() (rgk_amd/csrc/rgk_device.h) restated in float32.
"""
import ctypes as C

import numpy as np

from rgk_amd import capi

F = np.float32
H5 = [F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16)]


def mean_color(accum, count):
    """c = rgb / count, 0 where the count is 0 (float32)."""
    cnt = count.astype(np.uint32)
    c = np.zeros(accum.shape, F)
    m = cnt > 0
    c[m] = accum[m].astype(F) / cnt[m].astype(F)[:, None]
    return c


def default_sigma_color(accum, count, k):
    """What RenderDriver.denoise chooses: k x the mean over pixels of the largest channel of c."""
    return float(k) * float(mean_color(accum, count).max(axis=-1).astype(np.float64).mean())


def atrous_ref(accum, count, albedo, normal, depth, iterations=5, sigma_color=1.0, sigma_depth=0.02, normal_power_log2=6, demodulate=1):
    """(yres, xres, 3) float32 accumulator, (yres, xres) counts and the feature planes -> the denoised image."""
    yres, xres = depth.shape
    c = mean_color(accum, count)
    if iterations == 0:
        return c
    div = np.where(albedo > 0, albedo, F(1)).astype(F)
    if demodulate:
        c = c / div
    n = normal.astype(F)
    z = depth.astype(F)
    live = ~((n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0))
    sd = F(sigma_depth)
    old = np.seterr(all="ignore")
    try:
        for i in range(iterations):
            s = 1 << i
            si = F(sigma_color) * F(2.0 ** -i)
            sigma2 = F(si * si)
            sr = np.zeros((yres, xres, 3), F)
            sw = np.zeros((yres, xres), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    # p ranges over [y0, y1) x [x0, x1), q = p + (oy, ox) stays inside the frame
                    y0, y1 = max(0, -oy), min(yres, yres - oy)
                    x0, x1 = max(0, -ox), min(xres, xres - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    npq = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
                    wn = np.maximum(F(0), npq)
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    r = np.abs(z[P] - z[Q]) / (sd * (z[P] + z[Q]) + F(1e-20))
                    wz = F(1) / (F(1) + r * r)
                    d = c[P] - c[Q]
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wc = F(1) / (F(1) + d2 / sigma2)
                    w = (((H5[dy + 2] * H5[dx + 2]) * wn) * wz) * wc
                    w = np.where(live[Q], w, F(0)).astype(F)  # a tap without a normal is skipped: adding 0 changes no sum
                    sr[P] = sr[P] + w[..., None] * c[Q]
                    sw[P] = sw[P] + w
            ok = live & (sw > 0)
            out = c.copy()
            out[ok] = sr[ok] / sw[ok][:, None]
            c = out
    finally:
        np.seterr(**old)
    if demodulate:
        c = c * div
    return c.astype(F)


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))


# ------------------------------------------------------------------ features from the oracle
def _arr(ptr, n, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dtype)), shape=(n,)).copy() if n else np.zeros(0)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _norm(v):
    return v * (F(1) / np.sqrt(_dot(v, v)))[..., None]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0],
                     x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], axis=-1)


def pinhole(camera):
    cam = capi.Camera.from_buffer_copy(camera)
    cam.lens_size = 0.0
    return cam


def oracle_features(O, osc, desc, camera, xres, yres, bumpmap_scale):
    """Whole-frame feature planes: albedo (y, x, 3), normal (y, x, 3), depth (y, x), tri (y, x) int32."""
    L = O.lib()
    cam = pinhole(camera)
    Pn = xres * yres
    rays = np.zeros((Pn, 8), F)
    sub, lens, out6 = (C.c_float * 2)(0.5, 0.5), (C.c_float * 2)(0.0, 0.0), (C.c_float * 6)()
    for p in range(Pn):
        L.orc_camera_ray(C.byref(cam), p % xres, p // xres, xres, yres, sub, lens, out6)
        rays[p, :6] = out6[:]
    rays[:, 6], rays[:, 7] = 0.0, 10000.0
    hits, _ = osc.trace_closest(rays)
    tri = hits["tri"].astype(np.int32)
    hit = tri >= 0
    depth = np.where(hit, hits["t"], F(0)).astype(F)

    nv, nt = desc.n_vertices, desc.n_triangles
    normals = _arr(desc.normals, 3 * nv, C.c_float).reshape(-1, 3)
    tangents = _arr(desc.tangents, 3 * nv, C.c_float).reshape(-1, 3)
    texc = _arr(desc.texcoords, 2 * nv, C.c_float).reshape(-1, 2) if desc.texcoords else None
    idx = _arr(desc.tri_indices, 3 * nt, C.c_uint32).reshape(-1, 3)
    tmat = _arr(desc.tri_material, nt, C.c_uint32)
    mats = [desc.materials[i] for i in range(desc.n_materials)]

    t = np.where(hit, tri, 0)
    al, be = hits["b"].astype(F), hits["c"].astype(F)
    ia, ib, ic = (F(1) - al - be)[:, None], al[:, None], be[:, None]
    va, vb, vc = idx[t, 0], idx[t, 1], idx[t, 2]
    old = np.seterr(all="ignore")
    try:
        nA, nB, nC = normals[va], normals[vb], normals[vc]
        faceN = ia * nA + ib * nB + ic * nC
        ok = hit.copy()
        for alt in (nA, nB, nC):  # NaN fallbacks
            bad = np.isnan(faceN[:, 0])
            faceN[bad] = alt[bad]
        ok &= ~np.isnan(faceN[:, 0])
        ok &= ~(np.sqrt(_dot(faceN, faceN)) <= 0)
        faceN = _norm(faceN)
        uv = np.zeros((Pn, 2), F)
        if texc is not None:
            uv = (ia * texc[va] + ib * texc[vb] + ic * texc[vc]).astype(F)
        tangent = ia * tangents[va] + ib * tangents[vb] + ic * tangents[vc]
        lightN = faceN.copy()
        albedo = np.zeros((Pn, 3), F)
        mid = tmat[t]

        def tex(ti, p, slopes=False):
            rgb, r, b = (C.c_float * 3)(), C.c_float(), C.c_float()
            L.orc_texture_sample(osc.h, int(ti), (C.c_float * 2)(float(uv[p, 0]), float(uv[p, 1])), rgb, C.byref(r), C.byref(b))
            return (F(r.value), F(b.value)) if slopes else np.array(rgb[:], F)

        def leaf(m, p):
            k = m.kind
            if k == capi.BXDF_DIFFUSE:
                return tex(m.tex_diffuse, p)
            if k in (capi.BXDF_LTC_BECKMANN, capi.BXDF_LTC_GGX):
                return tex(m.tex_color, p)
            if k in (capi.BXDF_LTC_BECKMANN_DIFFUSE, capi.BXDF_LTC_GGX_DIFFUSE):
                return tex(m.tex_diffuse, p) + tex(m.tex_color, p)
            if k in (capi.BXDF_MIRROR, capi.BXDF_DIELECTRIC, capi.BXDF_TRANSPARENT):
                return np.ones(3, F)
            return np.zeros(3, F)

        def alb(m, p, level=0):
            if m.kind != capi.BXDF_MIX:
                return leaf(m, p)
            if level == 2:
                return np.zeros(3, F)
            a = F(m.amount)
            return a * alb(mats[m.mix_m1], p, level + 1) + (F(1) - a) * alb(mats[m.mix_m2], p, level + 1)

        for p in np.nonzero(ok)[0]:
            m = mats[mid[p]]
            if m.tex_bump >= 0:  # (a solid bump texture has slopes 0 and still takes this route: the sum is normalised again)
                right, bottom = tex(m.tex_bump, p, slopes=True)
                tg = tangent[p]
                if not ((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2] < F(0.001)):
                    tg = _norm(tg)
                    fn = faceN[p]
                    bit = _norm(_cross(fn, tg))
                    tg2 = _cross(bit, fn)
                    ln = _norm(fn + (tg2 * right + bit * bottom) * F(bumpmap_scale))
                    lightN[p] = fn if np.isnan(ln[0]) else ln
            albedo[p] = alb(m, p)
    finally:
        np.seterr(**old)
    normal = np.where(ok[:, None], lightN, F(0)).astype(F)
    albedo = np.where(ok[:, None], albedo, F(0)).astype(F)
    return (albedo.reshape(yres, xres, 3), normal.reshape(yres, xres, 3), depth.reshape(yres, xres), tri.reshape(yres, xres))


def reference_exact_ties(O, osc, desc, camera, xres, yres):
    """(y, x) bool: pixels whose centre ray has, by the oracle's own triangle test, two nearest triangles at exactly the same
    distance (an edge shared by coplanar triangles, coincident surfaces).  The reference has no rule for those: the winner is
    whichever its kd leaf lists first (the walker's rule is the higher id, rgk_trace.h)."""
    L = O.lib()
    cam = pinhole(camera)
    sub, lens, out6, tab = (C.c_float * 2)(0.5, 0.5), (C.c_float * 2)(0.0, 0.0), (C.c_float * 6)(), (C.c_float * 3)()
    ties = np.zeros((yres, xres), bool)
    for p in range(xres * yres):
        L.orc_camera_ray(C.byref(cam), p % xres, p // xres, xres, yres, sub, lens, out6)
        ray = (C.c_float * 8)(*out6[:], 0.0, 10000.0)
        ts = sorted(tab[0] for t in range(desc.n_triangles) if L.orc_test_intersection(osc.h, t, ray, tab))
        ties[p // xres, p % xres] = len(ts) >= 2 and ts[0] == ts[1]
    return ties
