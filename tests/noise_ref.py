"""CPU expectations for the half-buffer noise estimate and the variance-guided a-trous filter (include/rgk.h
rgk_noise_estimate_device / rgk_denoise_variance_device), for test_noise_cpu.py / test_gpu_noise.py and tools/noise_sweep.py.

The numpy float32 restatement of k_nz_tile_sums / k_nz_prepare / k_nz_prefilter / k_nz_atrous / k_dn_finish
(rgk_amd/csrc/rgk_post.hip): the same operations in the same order, so with contraction off on both sides it gives the kernels'
bits.  Shared pieces (mean_color, the tap table, rel_l2) come from post_ref.py.
"""
import numpy as np

import post_ref as R

F = np.float32
H5 = R.H5


def halves(accum, count, half_accum, half_count, div=None):
    """c, a, b (each (y, x, 3) float32, divided by `div` when given), f (y, x) and the estimable mask."""
    n = count.astype(np.uint32)
    nb = half_count.astype(np.uint32)
    est = (nb > 0) & (nb < n)
    na = np.where(est, n - nb, 1).astype(np.uint32)
    S, SB = accum.astype(F), half_accum.astype(F)
    c = R.mean_color(accum, count)
    a = np.zeros(S.shape, F)
    b = np.zeros(S.shape, F)
    f = np.zeros(n.shape, F)
    a[est] = (S[est] - SB[est]) / na[est].astype(F)[:, None]
    b[est] = SB[est] / nb[est].astype(F)[:, None]
    f[est] = (na[est].astype(F) * nb[est].astype(F)) / (n[est].astype(F) * n[est].astype(F))
    if div is not None:
        c, a, b = c / div, a / div, b / div
    return c, a, b, f, est


def variance(a, b, f, est):
    h = a - b
    v = ((h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1]) + h[..., 2] * h[..., 2]) * f
    return np.where(est, v, F(0)).astype(F)


def raw_variance(accum, count, half_accum, half_count):
    """The v plane of rgk_noise_estimate_device (nothing demodulated)."""
    _, a, b, f, est = halves(accum, count, half_accum, half_count)
    return variance(a, b, f, est)


def noise_tiles(accum, count, half_accum, half_count, tile_size):
    """Per tile, row-major: float64 sums of the float32 per-pixel terms over the estimable pixels -> (ty, tx, 2) float64
    {sum_var, sum_sq} and (ty, tx) uint64 n_estimable."""
    c, a, b, f, est = halves(accum, count, half_accum, half_count)
    v = variance(a, b, f, est)
    sq = ((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]).astype(F)
    yres, xres = est.shape
    ty, tx = -(-yres // tile_size), -(-xres // tile_size)
    sums = np.zeros((ty, tx, 2), np.float64)
    ne = np.zeros((ty, tx), np.uint64)
    for j in range(ty):
        for i in range(tx):
            T = (slice(j * tile_size, min(yres, (j + 1) * tile_size)), slice(i * tile_size, min(xres, (i + 1) * tile_size)))
            m = est[T]
            sums[j, i, 0] = v[T][m].astype(np.float64).sum()
            sums[j, i, 1] = sq[T][m].astype(np.float64).sum()
            ne[j, i] = int(m.sum())
    return sums, ne


def rel_noise(sums):
    """sqrt(sum of sum_var / sum of sum_sq), tiles added in row-major order in double."""
    sv = sq = 0.0
    for t in np.asarray(sums, np.float64).reshape(-1, 2):
        sv += float(t[0])
        sq += float(t[1])
    return float(np.sqrt(sv / sq)) if sq > 0 else 0.0


def _taps(yres, xres, s):
    """(dy, dx, P, Q): for every tap, the slices of the pixels p whose tap q = p + s * (dx, dy) lies inside the frame."""
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = s * dy, s * dx
            y0, y1 = max(0, -oy), min(yres, yres - oy)
            x0, x1 = max(0, -ox), min(xres, xres - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            yield dy, dx, (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _guide_weights(n, z, P, Q, sd, npow):
    npq = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
    wn = np.maximum(F(0), npq)
    for _ in range(npow):
        wn = wn * wn
    r = np.abs(z[P] - z[Q]) / (sd * (z[P] + z[Q]) + F(1e-20))
    wz = F(1) / (F(1) + r * r)
    return wn, wz


def _prefilter(var, n, z, live, sd, npow):
    """5 x 5, step 1: the (wn * wz)-weighted mean of v over the live taps; a pixel that is not live keeps its v."""
    yres, xres = var.shape
    sv = np.zeros((yres, xres), F)
    sw = np.zeros((yres, xres), F)
    for dy, dx, P, Q in _taps(yres, xres, 1):
        wn, wz = _guide_weights(n, z, P, Q, sd, npow)
        w = np.where(live[Q], wn * wz, F(0)).astype(F)
        sv[P] = sv[P] + w * var[Q]
        sw[P] = sw[P] + w
    ok = live & (sw > 0)
    out = var.copy()
    out[ok] = sv[ok] / sw[ok]
    return out


def variance_atrous_ref(accum, count, half_accum, half_count, albedo, normal, depth, iterations=5, sigma_k=3.0, sigma_depth=0.02,
                        normal_power_log2=6, demodulate=1, albedo_floor=0.25):
    """-> (image (y, x, 3) float32, variance (y, x) float32), what rgk_denoise_variance_device writes to out_rgb / out_variance."""
    yres, xres = depth.shape
    if iterations == 0:
        return R.mean_color(accum, count), raw_variance(accum, count, half_accum, half_count)
    div = None
    if demodulate:
        div = np.where(albedo > 0, np.maximum(albedo.astype(F), F(albedo_floor)), F(1)).astype(F)
    c, a, b, f, est = halves(accum, count, half_accum, half_count, div)
    var = variance(a, b, f, est)
    n = normal.astype(F)
    z = depth.astype(F)
    live = ~((n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0))
    sd = F(sigma_depth)
    k2 = F(F(sigma_k) * F(sigma_k))
    old = np.seterr(all="ignore")
    try:
        var = _prefilter(var, n, z, live, sd, normal_power_log2)
        for i in range(iterations):
            s = 1 << i
            sr = np.zeros((yres, xres, 3), F)
            sw = np.zeros((yres, xres), F)
            sv = np.zeros((yres, xres), F)
            for dy, dx, P, Q in _taps(yres, xres, s):
                wn, wz = _guide_weights(n, z, P, Q, sd, normal_power_log2)
                d = c[P] - c[Q]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                wc = F(1) / (F(1) + d2 / (k2 * (var[P] + var[Q]) + F(1e-20)))
                w = (((H5[dy + 2] * H5[dx + 2]) * wn) * wz) * wc
                w = np.where(live[Q], w, F(0)).astype(F)  # a tap without a normal is skipped: adding 0 changes no sum
                sr[P] = sr[P] + w[..., None] * c[Q]
                sw[P] = sw[P] + w
                sv[P] = sv[P] + (w * w) * var[Q]
            ok = live & (sw > 0)
            oc, ov = c.copy(), var.copy()
            oc[ok] = sr[ok] / sw[ok][:, None]
            ov[ok] = sv[ok] / (sw[ok] * sw[ok])
            c, var = oc, ov
    finally:
        np.seterr(**old)
    if demodulate:
        c = c * div
    return c.astype(F), var.astype(F)


# ------------------------------------------------------------------ the oracle's images as two halves
CASES = [("cornell 96x96, 2 + 2 vs 256 spp", "cornell-256", 0.375, 2, 256), ("sponza proxy 115x64, 2 + 2 vs 128 spp", "sponza-1080p", 0.06, 2, 128)]
HALF_SEEDS = (42, 100042)  # seedstart of the tile seeds of the two halves


def oracle_case(O, name, scale, spp_half, hi):
    """(S, n, S_B, n_B) of two oracle rounds of `spp_half` samples with tile seeds from HALF_SEEDS, the oracle's image at `hi`
    samples, and the feature planes composed from the oracle (post_ref.oracle_features)."""
    from rgk_amd.workloads import Workload
    wl = Workload(name, scale=scale, spp=spp_half)
    desc = wl.builder.to_desc()
    osc = O.OracleScene(desc)
    half = [osc.render_round(wl.camera, wl.params(), O.generate_task_list(wl.xres, wl.yres, seedstart=s))[:2] for s in HALF_SEEDS]
    feats = R.oracle_features(O, osc, desc, wl.camera, wl.xres, wl.yres, wl.bumpscale)
    wh = Workload(name, scale=scale, spp=hi)
    hacc, hcnt, _ = O.OracleScene(wh.builder.to_desc()).render_round(wh.camera, wh.params(), O.generate_task_list(wh.xres, wh.yres))
    (sa, na), (sb, nb) = half
    return (sa + sb, na + nb, sb, nb), R.mean_color(hacc, hcnt), feats
