"""CPU expectations for per-sample demodulated accumulation (include/rgk.h rgk_render_round_demod_device, rgk_remodulate_device), for
test_demod_cpu.py / test_gpu_demod.py / test_gpu_demod_memstate.py.

* `sample_divisors`: div_s of every sample of a round, composed from the oracle library's pieces -- the pixel seeds of Tracer::Render
  (tile.seed + (k + 1) * 0x42424242, k row-major in the tile), orc_sampler_eval (2-D dimension 0: pixel jitter, 1: lens),
  orc_camera_ray, first hits by orc_trace_closest_exhaustive (the rule the walkers are pinned to bit for bit) and the albedo composed
  as post_ref.oracle_features composes it, through the floor rule.
* `divisor_sum`, `demod_sum`: A and D of a round from those, float32, in sample order.
* `remodulate`: rgk_remodulate_device in both of its modes.
* `uniform_albedo`: a copy of a fixture scene with every material diffuse with one solid colour, black sky, lights kept.
"""
import copy
import ctypes as C

import numpy as np

from rgk_amd import capi

import post_ref as PR

F = np.float32


def floor_rule(a, floor):
    """div = a > 0 ? max(a, floor) : 1 per channel (float32)."""
    a = np.asarray(a, F)
    return np.where(a > 0, np.maximum(a, F(floor)), F(1)).astype(F)


def pixel_seeds(tiles, xres, yres):
    """(y, x) uint32: PathTracer::samplerSeed of every pixel the tiles cover (the others: 0), and (y, x) bool: covered."""
    seed, covered = np.zeros((yres, xres), np.uint32), np.zeros((yres, xres), bool)
    for t in tiles:
        tw = t.x1 - t.x0
        for y in range(t.y0, t.y1):
            for x in range(t.x0, t.x1):
                k = (y - t.y0) * tw + (x - t.x0)
                seed[y, x] = (t.seed + (k + 1) * 0x42424242) & 0xFFFFFFFF
                covered[y, x] = True
    return seed, covered


def sample_rays(O, camera, tiles, xres, yres, multisample, centre=False):
    """(y, x, s, 8) float32: the camera ray RenderPixel traces for sample s of every covered pixel, near 0, far 10000.
    centre: the feature pass's ray instead -- through the pixel centre, the lens ignored -- for every s."""
    L = O.lib()
    seed, covered = pixel_seeds(tiles, xres, yres)
    cam = PR.pinhole(camera) if centre else capi.Camera.from_buffer_copy(camera)
    rays = np.zeros((yres, xres, multisample, 8), F)
    rays[..., 7] = 10000.0
    out6 = (C.c_float * 6)()
    s_idx = np.arange(multisample, dtype=np.uint32)
    for y in range(yres):
        for x in range(xres):
            if not covered[y, x]:
                continue
            sd = np.full(multisample, seed[y, x], np.uint32)
            jit = O.sampler_eval(sd, s_idx, np.zeros(multisample, np.uint32), True)
            lens = O.sampler_eval(sd, s_idx, np.ones(multisample, np.uint32), True)
            for s in range(multisample):
                sub = (C.c_float * 2)(0.5, 0.5) if centre else (C.c_float * 2)(float(jit[s, 0]), float(jit[s, 1]))
                ln = (C.c_float * 2)(0.0, 0.0) if centre else (C.c_float * 2)(float(lens[s, 0]), float(lens[s, 1]))
                L.orc_camera_ray(C.byref(cam), x, y, xres, yres, sub, ln, out6)
                rays[y, x, s, :6] = out6[:]
    return rays, covered


def ray_albedo(O, osc, desc, rays, trace=None):
    """(n, 3) float32 albedo at the first hit of each of the n rays, and (n,) bool: the ray has a vertex (a hit whose interpolated
    normal is usable).  post_ref.oracle_features' composition for rays of any kind; 0 where there is no vertex.
    trace: rays -> hits, default the oracle's exhaustive search."""
    L = O.lib()
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n_rays = len(rays)
    hits = (trace or osc.trace_closest_exhaustive)(rays)
    if isinstance(hits, tuple):
        hits = hits[0]
    tri = hits["tri"].astype(np.int32)
    hit = tri >= 0
    nv, nt = desc.n_vertices, desc.n_triangles
    normals = PR._arr(desc.normals, 3 * nv, C.c_float).reshape(-1, 3)
    texc = PR._arr(desc.texcoords, 2 * nv, C.c_float).reshape(-1, 2) if desc.texcoords else None
    idx = PR._arr(desc.tri_indices, 3 * nt, C.c_uint32).reshape(-1, 3)
    tmat = PR._arr(desc.tri_material, nt, C.c_uint32)
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
        ok &= ~(np.sqrt(PR._dot(faceN, faceN)) <= 0)
        uv = np.zeros((n_rays, 2), F)
        if texc is not None:
            uv = (ia * texc[va] + ib * texc[vb] + ic * texc[vc]).astype(F)
    finally:
        np.seterr(**old)
    mid = tmat[t]
    cache = {}

    def tex(ti, p):
        key = (int(ti), uv[p, 0].tobytes(), uv[p, 1].tobytes())
        if key not in cache:
            rgb, r, b = (C.c_float * 3)(), C.c_float(), C.c_float()
            L.orc_texture_sample(osc.h, int(ti), (C.c_float * 2)(float(uv[p, 0]), float(uv[p, 1])), rgb, C.byref(r), C.byref(b))
            cache[key] = np.array(rgb[:], F)
        return cache[key]

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

    albedo = np.zeros((n_rays, 3), F)
    for p in np.nonzero(ok)[0]:
        albedo[p] = alb(mats[mid[p]], p)
    return albedo, ok


def sample_divisors(O, osc, desc, camera, tiles, xres, yres, multisample, albedo_floor, centre=False, trace=None):
    """(y, x, s, 3) float32: div_s of every sample of a round over `tiles` ((1, 1, 1) for a miss, a dropped vertex and a pixel no
    tile covers), and (y, x) bool: covered."""
    rays, covered = sample_rays(O, camera, tiles, xres, yres, multisample, centre)
    albedo, ok = ray_albedo(O, osc, desc, rays, trace)
    div = np.where(ok[:, None], floor_rule(albedo, albedo_floor), F(1)).astype(F)
    return div.reshape(yres, xres, multisample, 3), covered


def divisor_sum(div, covered):
    """A of one round: per pixel ((0 + div_0) + div_1) + ..., float32; 0 where no tile covers the pixel."""
    A = np.zeros(div.shape[:2] + (3,), F)
    for s in range(div.shape[2]):
        A = (A + div[:, :, s]).astype(F)
    return np.where(covered[..., None], A, F(0)).astype(F)


def demod_sum(values, div, covered):
    """D of one round from the samples' values v_s (y, x, s, 3): per pixel ((0 + v_0 / div_0) + v_1 / div_1) + ..., float32."""
    D = np.zeros(div.shape[:2] + (3,), F)
    for s in range(div.shape[2]):
        D = (D + (values[:, :, s].astype(F) / div[:, :, s]).astype(F)).astype(F)
    return np.where(covered[..., None], D, F(0)).astype(F)


def remodulate(img, div_rgb, div_count=None, albedo_floor=0.02):
    """rgk_remodulate_device: img * (A / n) (1 where n == 0) with a count plane, img * floor_rule(albedo) without."""
    img, div_rgb = np.asarray(img, F), np.asarray(div_rgb, F)
    if div_count is None:
        dbar = floor_rule(div_rgb, albedo_floor)
    else:
        n = np.asarray(div_count).astype(np.uint32)
        dbar = np.ones(div_rgb.shape, F)
        m = n > 0
        dbar[m] = (div_rgb[m] / n[m].astype(F)[:, None]).astype(F)
    return (img * dbar).astype(F)


def uniform_albedo(builder, v):
    """A copy of a scene builder with every material a diffuse one of the solid colour (v, v, v) -- emission kept, so emitters still
    light the scene -- and a black sky; point lights and geometry as they are."""
    sb = copy.copy(builder)
    sb.textures = list(builder.textures) + [dict(kind=capi.TEX_SOLID, color=(float(v),) * 3, data=None, lut=None)]
    t = len(sb.textures) - 1
    sb.materials = []
    for m in builder.materials:
        m = dict(m)
        m.update(kind=capi.BXDF_DIFFUSE, tex_diffuse=t, tex_color=-1, tex_bump=-1, mix_m1=-1, mix_m2=-1, amount=0.0)
        sb.materials.append(m)
    sb.mat_by_name = {m["name"]: i for i, m in enumerate(sb.materials)}
    sb.sky = dict(builder.sky, mode=capi.SKY_COLOR, color=(0.0, 0.0, 0.0), tex=-1)
    return sb
