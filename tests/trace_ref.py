"""Scenes, rays and the comparison of the exhaustive-search traversal tests (test_exhaustive_cpu.py, test_gpu_exhaustive.py,
and the re-check in test_gpu_parity.check_closest).

The reference is OracleScene.trace_closest_exhaustive / visibility_exhaustive (oracle/rgk_cpu.cpp Scene::FindExhaustive): every
triangle tested with the kernels' own triangle test under the walkers' stated rule (rgk_amd/csrc/rgk_trace.h) -- no tree, so
nothing here depends on a builder.  Everything is seeded and made in memory; nothing is read from disk but tests/golden/.
"""
import ctypes as C

import numpy as np

from rgk_amd import capi
from rgk_amd.scene import SceneBuilder

F = np.float32
FIELDS = ("t", "a", "b", "c")


# ------------------------------------------------------------------ scenes
def builder_of(tri):
    """(k, 3, 3) float32 corner positions -> a SceneBuilder over k triangles with three vertices each (the construction of
    test_gpu_parity.test_triangle_soup_with_degenerates)."""
    tri = np.ascontiguousarray(tri, dtype=F)
    sb = SceneBuilder()
    m = sb.new_material("m", capi.BXDF_DIFFUSE)
    m["tex_diffuse"] = sb.create_solid_texture((0.5, 0.5, 0.5))
    sb.register_material(m)
    pos = tri.reshape(-1, 3)
    sb.add_mesh(pos, np.tile([0, 1, 0], (len(pos), 1)).astype(F), np.zeros((len(pos), 2), F), np.tile([1, 0, 0], (len(pos), 1)).astype(F),
                np.arange(len(pos)).reshape(-1, 3), 0)
    return sb


def indexed_builder(V, faces):
    """Shared vertices: the edges of neighbouring triangles are the same floats."""
    V = np.ascontiguousarray(V, dtype=F)
    sb = SceneBuilder()
    m = sb.new_material("m", capi.BXDF_DIFFUSE)
    m["tex_diffuse"] = sb.create_solid_texture((0.5, 0.5, 0.5))
    sb.register_material(m)
    sb.add_mesh(V, np.tile([0, 1, 0], (len(V), 1)).astype(F), np.zeros((len(V), 2), F), np.tile([1, 0, 0], (len(V), 1)).astype(F), faces, 0)
    return sb


def soup(k, seed=4):
    """k random triangles in general position, every 97th from the 6th on degenerate (two equal corners: a NaN plane, never hit)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-5, 5, (k, 1, 3))
    tri = (c + rng.normal(scale=0.4, size=(k, 3, 3))).astype(F)
    tri[5::97, 2] = tri[5::97, 1]
    return tri


def flat():
    """33 triangles in the plane y = 0: the scene box has no extent on one axis (the Morton scale of that axis is 0)."""
    rng = np.random.default_rng(11)
    c = rng.uniform(-5, 5, (33, 1, 3))
    tri = (c + rng.normal(scale=0.8, size=(33, 3, 3))).astype(F)
    tri[:, :, 1] = 0.0
    return tri


def nested():
    """40 triangles around one centroid, each 1.25 x the one before and turned a little: every Morton key is the same, and a
    surface-area build sees one chain."""
    rng = np.random.default_rng(12)
    base = rng.normal(size=(3, 3))
    base -= base.mean(axis=0)
    tri = np.zeros((40, 3, 3))
    for i in range(40):
        a = 0.37 * i
        rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(2 * a), -np.sin(2 * a)], [0, np.sin(2 * a), np.cos(2 * a)]])
        tri[i] = 0.01 * 1.25 ** i * base @ rot.T
    return tri.astype(F)


def duplicates():
    """The 65-triangle soup with runs of 2, 3 and 9 coincident copies of three of its triangles (65 in all): exact ties decide."""
    tri = soup(65)
    for first, run, src in ((10, 2, 3), (20, 3, 40), (30, 9, 57)):
        tri[first:first + run] = tri[src]
    return tri


def icosphere(levels=2):
    """(V, faces) of a closed mesh with shared vertices: an icosahedron subdivided `levels` times (2: 162 vertices, 320 faces),
    vertices pushed onto the unit sphere in float32."""
    p = (1 + 5 ** 0.5) / 2
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, out = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(V).astype(F), np.array(faces, np.uint32)


def deep(levels=20, per_level=60):
    """A geometric progression of sizes along a line: `per_level` small triangles around x = 2^-j, scattered over 0.3 * 2^-j, for
    each j < levels.  Whatever splits the scene by position peels off a level or two at a time: a deep tree from 1 200 triangles
    (the host's binned-SAH build: 22 levels of 4-wide nodes, 68 stack entries)."""
    rng = np.random.default_rng(13)
    out = []
    for j in range(levels):
        s = 2.0 ** -j
        c = np.array([s, 0, 0]) + rng.uniform(-0.3, 0.3, (per_level, 1, 3)) * s
        out.append(c + rng.normal(scale=0.04 * s, size=(per_level, 3, 3)))
    return np.concatenate(out).astype(F)


SCENES = {  # name -> () -> SceneBuilder
    **{f"count{k}": (lambda k=k: builder_of(soup(k))) for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65, 257)},
    "flat": lambda: builder_of(flat()),
    "nested": lambda: builder_of(nested()),
    "duplicates": lambda: builder_of(duplicates()),
    "closed": lambda: indexed_builder(*icosphere(2)),
    "deep": lambda: builder_of(deep()),
    "scaled-down": lambda: builder_of(soup(65) * F(1e-3)),
    "scaled-up-moved": lambda: builder_of(soup(65) * F(1e3) + np.array([1e4, -1e4, 1e4], F)),
}


# ------------------------------------------------------------------ rays
def random_rays(rng, lo, hi, n):
    """Origins inside the box [lo, hi] (2 % off its faces), normalised normal directions."""
    o = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, 3))).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


def box_of(info):
    return np.array(list(info.bbox_min), np.float64), np.array(list(info.bbox_max), np.float64)


def targets_of(sb, seed=0):
    """Points of the scene's surface in float32: every vertex, every edge midpoint, and three random interior points per triangle."""
    sb.finalize()
    rng = np.random.default_rng(seed)
    P = sb.V[sb.F.astype(np.int64)]                                    # (k, 3, 3)
    mids = (P + np.roll(P, 1, axis=1)) * F(0.5)
    w = rng.dirichlet((1, 1, 1), (len(P), 3)).astype(F)                # (k, 3 points, 3 weights)
    inner = np.einsum("kpw,kwx->kpx", w, P).astype(F)
    return np.concatenate([P.reshape(-1, 3), mids.reshape(-1, 3), inner.reshape(-1, 3)]).astype(F)


def ray_mix(osc, n, seed, targets, in_plane_y=None, inside=None, within=None):
    """(n, 8) float32 rays against the oracle scene `osc`, in ten equal shares:
      0    origins inside the scene box, random directions          1  the same origins, aimed at `targets`
      2    origins up to half a box outside, half of them aimed     3  axis-parallel through a target, +0 and -0 in the other two
      4    aimed with one direction component exactly 0, that one replaced by +-1e-30      5  aimed, random near / far windows
      6    aimed, near > far                                        8  aimed, far = 1e30
      7    aimed, windows that end or begin at the first hit: far = t, t - eps, t - 1.5 eps, t / 2 and near = t, t + eps, t + 1.5 eps
      9    aimed -- or, with in_plane_y, origin and direction in the plane y = in_plane_y
    "Aimed": the direction is normalize(target - origin) in float32, `targets` being points of the surface (targets_of: vertices,
    edge midpoints, interior points), so most rays hit something and many pass exactly through a vertex or an edge.
    `inside` = (centre, radius): every origin is drawn in that ball instead; shares 3 and 4 then move theirs onto a line through
    the target -- anywhere, or with `within` only where the new origin stays within that distance of the centre (a closed mesh
    around it: the ray still starts inside).  No NaN, no infinity.  The first hits that share 7 needs
    come from the exhaustive reference."""
    rng = np.random.default_rng(seed)
    info = osc.info()
    lo, hi = box_of(info)
    eps = F(info.epsilon)
    diag = float(np.linalg.norm(hi - lo))
    o, d = random_rays(rng, lo, hi, n)
    share = np.arange(n) * 10 // max(n, 1)
    s = share == 2
    o[s] = (lo + (hi - lo) * rng.uniform(-0.5, 1.5, (s.sum(), 3))).astype(F)
    if inside is not None:
        c, r = inside
        v = rng.normal(size=(n, 3))
        v *= (r * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
        o = (np.asarray(c) + v).astype(F)
    tg = np.asarray(targets, F)[rng.integers(0, len(targets), n)]
    aimed = (share != 0) & ~((share == 2) & (np.arange(n) % 2 == 0))
    v = tg - o                                                      # float32 all the way: the direction a caller would compute
    ln = np.sqrt((v * v).sum(axis=1, dtype=F))
    aimed &= ln > 0
    d[aimed] = v[aimed] / ln[aimed, None]
    centre = None if inside is None else np.asarray(inside[0], F)

    def allowed(cand):                                              # may an origin be moved to `cand`?
        if inside is None or within is None:
            return np.ones(len(cand), bool)
        return np.linalg.norm(cand - centre, axis=1) < within
    # share 3: start on the axis-parallel line through the target (the other two coordinates are the target's), so the ray passes
    # exactly through that vertex, edge midpoint or interior point
    idx = np.nonzero(share == 3)[0]
    axis, sign = np.arange(len(idx)) % 3, np.where(np.arange(len(idx)) % 2, 1, -1).astype(F)
    cand = tg[idx].copy()
    if inside is None or within is None:
        cand[np.arange(len(idx)), axis] = (tg[idx, axis] - sign * rng.uniform(0.05, 0.6, len(idx)).astype(F) * F(diag)).astype(F)
    else:                                                           # ... from the centre's side of the target, part of the way back to the centre's plane
        rel = tg[idx, axis] - centre[axis]
        sign = np.where(rel >= 0, 1, -1).astype(F)
        cand[np.arange(len(idx)), axis] = (centre[axis] + rel * rng.uniform(0.05, 0.7, len(idx)).astype(F)).astype(F)
    ok = allowed(cand) & (cand != tg[idx]).any(axis=1)
    ax = np.zeros((len(idx), 3), F)
    ax[rng.integers(0, 2, (len(idx), 3)) == 1] = F(-0.0)
    ax[np.arange(len(idx)), axis] = sign
    d[idx] = ax
    o[idx[ok]] = cand[ok]
    # share 4: the origin takes one coordinate of its target, so the aimed direction is exactly 0 there -- replaced by +-1e-30
    idx = np.nonzero(share == 4)[0]
    comp = idx % 3
    cand = o[idx].copy()
    cand[np.arange(len(idx)), comp] = tg[idx, comp]
    v = tg[idx] - cand
    ln = np.sqrt((v * v).sum(axis=1, dtype=F))
    ok = allowed(cand) & (ln > 0)
    o[idx[ok]] = cand[ok]
    d[idx[ok]] = v[ok] / ln[ok, None]
    d[idx, comp] = np.where(idx % 2, F(1e-30), F(-1e-30))
    if in_plane_y is not None:
        idx = np.nonzero(share == 9)[0]
        o[idx, 1] = in_plane_y
        d[idx, 1] = np.where(idx % 2, F(0.0), F(-0.0))
        d[idx] /= np.linalg.norm(d[idx], axis=1, keepdims=True)
    near = np.zeros(n, F)
    far = np.full(n, 10000.0, F)
    s = share == 5
    near[s] = rng.uniform(0, 0.5 * diag, s.sum())
    far[s] = near[s] + rng.uniform(0, diag, s.sum()).astype(F)
    s = share == 6
    far[s] = rng.uniform(0, 0.5 * diag, s.sum())
    near[s] = far[s] + rng.uniform(0.01 * diag, diag, s.sum()).astype(F)
    far[share == 8] = 1e30
    idx = np.nonzero(share == 7)[0]
    first = osc.trace_closest_exhaustive(np.concatenate([o[idx], d[idx], near[idx, None], far[idx, None]], axis=1))
    t = np.where(first["tri"] >= 0, first["t"], F(0.5 * diag)).astype(F)
    kind = np.arange(len(idx)) % 7
    far[idx] = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [t, t - eps, t - F(1.5) * eps, t * F(0.5)], far[idx]).astype(F)
    near[idx] = np.select([kind == 4, kind == 5, kind == 6], [t, t + eps, t + F(1.5) * eps], near[idx]).astype(F)
    rays = np.concatenate([o, d, near[:, None], far[:, None]], axis=1).astype(F)
    assert np.isfinite(rays).all()
    return np.ascontiguousarray(rays)


def visibility_pairs(osc, n, seed):
    """n pairs of distinct points inside the scene box (a == b would make a NaN direction: none)."""
    rng = np.random.default_rng(seed)
    lo, hi = box_of(osc.info())
    a = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, 3))).astype(F)
    b = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, 3))).astype(F)
    same = (a == b).all(axis=1)
    b[same] = a[same] + F(0.25) * (hi - lo).astype(F) + F(1e-3)
    assert not (a == b).all(axis=1).any()
    return a, b


def camera_rays(O, camera, xres, yres):
    """(xres * yres, 8) rays through the pixel centres, row-major, by the oracle's Camera::GetPixelRay (lens ignored), [0, 10000]."""
    L = O.lib()
    cam = capi.Camera.from_buffer_copy(camera)
    cam.lens_size = 0.0
    rays = np.zeros((xres * yres, 8), F)
    sub, lens, out6 = (C.c_float * 2)(0.5, 0.5), (C.c_float * 2)(0.0, 0.0), (C.c_float * 6)()
    for p in range(xres * yres):
        L.orc_camera_ray(C.byref(cam), p % xres, p // xres, xres, yres, sub, lens, out6)
        rays[p, :6] = out6[:]
    rays[:, 7] = 10000.0
    return rays


# ------------------------------------------------------------------ the comparison
def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def differing(got, want):
    """Per-ray bool: the two hit records differ in the triangle or in one bit of t, a, b, c (a miss is t = +inf, a = b = c = 0
    on both sides, so misses are compared in full as well)."""
    bad = got["tri"] != want["tri"]
    for k in FIELDS:
        bad |= bits(got[k]) != bits(want[k])
    return bad


def describe(rays, got, want, bad, limit=5):
    return "; ".join(f"ray {i} o={rays[i, :3]} d={rays[i, 3:6]} [{rays[i, 6]!r}, {rays[i, 7]!r}]: got tri {got['tri'][i]} t {got['t'][i]!r}, "
                     f"exhaustive tri {want['tri'][i]} t {want['t'][i]!r}" for i in np.nonzero(bad)[0][:limit])


def kd_vs_exhaustive(kd, ex, eps):
    """The kd-tree oracle against the exhaustive one on the same rays.  Asserts what must hold (t_ex <= t_kd per ray with a miss
    as +inf, equal bits where the triangle is the same) and returns how the rest splits: exact-t ties, within 2 eps, beyond."""
    tk = np.where(kd["tri"] >= 0, kd["t"], np.inf).astype(np.float64)
    te = np.where(ex["tri"] >= 0, ex["t"], np.inf).astype(np.float64)
    assert (te <= tk).all(), np.nonzero(te > tk)[0][:10]
    same = kd["tri"] == ex["tri"]
    for k in FIELDS:
        assert np.array_equal(bits(kd[k][same]), bits(ex[k][same])), k
    other = ~same
    exact = other & (tk == te)
    with np.errstate(invalid="ignore"):
        band = other & ~exact & (tk - te <= 2.0 * float(eps))
    beyond = other & ~exact & ~band
    return dict(rays=len(kd), differ=int(other.sum()), exact_ties=int(exact.sum()), within_2eps=int(band.sum()), beyond=int(beyond.sum()))
