"""Scenes, moves and references of the rgk_scene_refit tests (test_refit_cpu.py, test_gpu_refit.py, memstate_ref.py), GPU-free.

A refit rewrites the intersection records, the tree's boxes and codes, the per-triangle shading records (when normals or
tangents are passed), the areal-light tables, epsilon and the padded box, and drops the per-frame lists.  Three families of
cases, each made once per process and never changed afterwards:

    shade      test_gpu_const_light.small_scene (bump-mapped, textured LTC surfaces, mirror, glass) with a sphere light and an
               emissive triangle -- or, `point=True`, with its one point light of size 0, the constant-light route's scene --
               twisted, its normals and tangents turned by each vertex's own twist angle;
    lights     the all-diffuse Cornell box with its emissive quad, an emissive fan of three triangles of clearly different areas,
               an emissive pair above the floor and a sphere light, under a smooth non-uniform stretch that reverses area
               orders and moves the light powers;
    geometry   moves of the scenes of trace_ref.SCENES that a smooth twist never makes (GEOMETRY below).

Frames are memstate_ref's: 67 x 45, 8 spp, depth 5.  Every reference is the oracle's: rounds with every ray answered by
exhaustive search, feature planes composed by post_ref.oracle_features on exhaustive first hits, hits by
trace_closest_exhaustive / visibility_exhaustive."""
import functools

import numpy as np

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params

import trace_ref as T

F = np.float32
W, H, SPP, DEPTH = 67, 45, 8, 5


def params(reverse=0):
    return make_params(W, H, SPP, DEPTH, clamp=30.0, russian=0.7, bumpscale=2.0, reverse=reverse)


# ------------------------------------------------------------------ the moves
def twist_angles(V0, angle):
    ctr, ext = V0.mean(axis=0), np.ptp(V0, axis=0).max()
    return angle * (V0[:, 1] - ctr[1]) / ext


def twist_and_swell(V0, angle=0.35, swell=0.03):
    """A smooth, non-rigid move: a twist about the vertical axis that grows with height, and a swell of `swell` x the scene size."""
    ctr, ext = V0.mean(axis=0), np.ptp(V0, axis=0).max()
    ang = angle * (V0[:, 1] - ctr[1]) / ext
    c, s_ = np.cos(ang), np.sin(ang)
    V1 = V0.copy()
    V1[:, 0] = ctr[0] + c * (V0[:, 0] - ctr[0]) - s_ * (V0[:, 2] - ctr[2])
    V1[:, 2] = ctr[2] + s_ * (V0[:, 0] - ctr[0]) + c * (V0[:, 2] - ctr[2])
    return (V1 + swell * ext * np.sin(3.0 * V0[:, [1, 2, 0]] / ext)).astype(F)


def turned(vec, ang):
    """Unit vectors turned about the vertical axis by `ang` (per row), normalised in float32."""
    c, s_ = np.cos(ang), np.sin(ang)
    out = np.stack([c * vec[:, 0] - s_ * vec[:, 2], vec[:, 1], s_ * vec[:, 0] + c * vec[:, 2]], axis=1).astype(F)
    ln = np.sqrt((out * out).sum(axis=1, dtype=F)).astype(F)
    return (out / ln[:, None]).astype(F)


def with_mesh(make, V=None, N=None, Tn=None):
    """A fresh builder of `make` holding the given vertices / normals / tangents (None: its own)."""
    sb = make()
    sb.finalize()
    for name, a in (("vertices", V), ("normals", N), ("tangents", Tn)):
        if a is not None:
            setattr(sb, name, [np.ascontiguousarray(a, dtype=F)])
    return sb.finalize()


# ------------------------------------------------------------------ shade
def _shade_builder(point):
    import test_gpu_const_light as CL
    return CL.small_scene() if point else CL.small_scene(lights=((0.3, 2.6, 0.4, 0.15),), emitter=True)


@functools.lru_cache(maxsize=None)
def shade_case(point=False):
    """dict: make, camera, prm, and `mesh`: key -> (V, N, T) for the keys "000" (as built), "100" (moved vertices only),
    "110" (moved vertices, turned normals, old tangents), "111" (everything moved)."""
    make = functools.partial(_shade_builder, point)
    sb = make().finalize()
    V0, N0, T0 = sb.V.copy(), sb.N.copy(), sb.T.copy()
    V1 = twist_and_swell(V0)
    ang = twist_angles(V0, 0.35)
    N1, T1 = turned(N0, ang), turned(T0, ang)
    for a in (V0, N0, T0, V1, N1, T1):
        a.setflags(write=False)
    cam = make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=W, yres=H, focus_plane=5.0)
    mesh = {"000": (V0, N0, T0), "100": (V1, N0, T0), "110": (V1, N1, T0), "111": (V1, N1, T1)}
    return dict(make=make, camera=cam, prm=params(), mesh=mesh, bump=2.0)


def cache_camera(view="low"):
    """The cameras of the frame-cache test.  "low": low and close, so that the cubes cover whole pixel groups; "narrow": the
    frame's camera with a field of view of 25 degrees.  After the twist many pixel groups see past a cube to a wall beyond
    everything they hit before (test_refit_cpu.py), where an entry list or a cap kept from before the refit no longer holds."""
    if view == "narrow":
        return make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=25, xres=W, yres=H, focus_plane=5.0)
    return make_camera((1.5, 0.4, 3.0), (-0.5, 0.4, -0.5), (0, 1, 0), fov=50, xres=W, yres=H, focus_plane=5.0)


def first_hit_depths(key, camera, point=True):
    """(y, x) float32: distance of the exhaustive first hit through every pixel centre of the shade case's mesh `key`, inf for a miss."""
    from oracle import rgk_oracle as O
    ex = oracle_scene("shade", key, point)[0].trace_closest_exhaustive(T.camera_rays(O, camera, W, H))
    return np.where(ex["tri"] >= 0, ex["t"], np.inf).astype(F).reshape(H, W)


# ------------------------------------------------------------------ lights
def _lights_builder():
    from test_bdpt_cpu import cornell_builder
    sb = cornell_builder("quad")
    m = sb.new_material("fan", capi.BXDF_DIFFUSE)
    m["tex_diffuse"] = sb.create_solid_texture((0.5, 0.5, 0.5))
    m["emission"] = (3.0, 2.0, 1.0)
    mi = sb.register_material(m)
    # three triangles in the plane z = -0.9 facing the camera, areas 0.03 : 0.04 : 0.05, spread over x
    z, y0 = -0.9, 0.6
    pos = []
    for x0, base, height in ((0.55, 0.3, 0.2), (-0.1, 0.4, 0.2), (-0.75, 0.4, 0.25)):
        pos += [(x0, y0, z), (x0, y0 + height, z), (x0 + base, y0, z)]
    pos = np.array(pos, F)
    n = len(pos)
    sb.add_mesh(pos, np.tile([0, 0, 1], (n, 1)).astype(F), np.zeros((n, 2), F), np.tile([1, 0, 0], (n, 1)).astype(F), np.arange(n).reshape(-1, 3), mi)
    # ... and a second light of several triangles: two just above the floor facing up, areas 0.02 : 0.025
    m = sb.new_material("pair", capi.BXDF_DIFFUSE)
    m["tex_diffuse"] = sb.create_solid_texture((0.5, 0.5, 0.5))
    m["emission"] = (1.0, 2.0, 4.0)
    mi = sb.register_material(m)
    y = 0.05
    pos = np.array([(0.4, y, 0.5), (0.6, y, 0.5), (0.4, y, 0.7), (-0.7, y, 0.5), (-0.5, y, 0.5), (-0.7, y, 0.75)], F)
    sb.add_mesh(pos, np.tile([0, 1, 0], (6, 1)).astype(F), np.zeros((6, 2), F), np.tile([1, 0, 0], (6, 1)).astype(F), np.arange(6).reshape(-1, 3), mi)
    sb.add_point_light((0.5, 1.2, 0.3), (1.0, 0.9, 0.7), 2.0, 0.1)
    return sb


def stretch(V0):
    """Smooth and non-uniform: heights grow with x, depths grow with x and by a seventh overall."""
    V1 = V0.astype(np.float64).copy()
    V1[:, 1] = V0[:, 1] * (1.0 + 0.3 * V0[:, 0])
    V1[:, 2] = V0[:, 2] * (1.15 + 0.6 * V0[:, 0])
    return V1.astype(F)


def light_tables(sb, V):
    """What build_areal_tables (rgk_commit.cpp) derives, restated in float32: per areal light (areas in the light's own order,
    triangle ids by descending (area, id), power); and the total areal power."""
    sb.finalize()
    V = np.asarray(V, F)
    out, total = [], F(0)
    for tris in sb.areal:
        P = V[sb.F[np.asarray(tris, np.int64)].astype(np.int64)]
        c = np.cross((P[:, 0] - P[:, 1]).astype(F), (P[:, 2] - P[:, 1]).astype(F)).astype(F)
        area = (F(0.5) * np.sqrt((c * c).sum(axis=1, dtype=F))).astype(F)
        order = [t for _, t in sorted(zip(area.tolist(), tris), reverse=True)]
        e = sb.materials[int(sb.FM[tris[0]])]["emission"]
        power = F(area.sum(dtype=F)) * F(F(e[0]) + F(e[1]) + F(e[2]))
        out.append(dict(tris=list(tris), area=area, order=order, power=float(power)))
        total = F(total + power)
    return out, float(total)


def point_power(sb):
    return float(sum(4.0 * np.pi * l["intensity"] for l in sb.pointlights))


@functools.lru_cache(maxsize=None)
def lights_case():
    """dict: make, camera, prm, `mesh`: "00" (as built), "10" (stretched), "11" (stretched, with normals that change every
    emissive triangle's vertex-A normal)."""
    from test_bdpt_cpu import cornell_camera
    sb = _lights_builder().finalize()
    V0, N0 = sb.V.copy(), sb.N.copy()
    V1 = stretch(V0)
    tilt = N0.astype(np.float64) + 0.25 * np.sin(3.0 * V0[:, [1, 2, 0]] + np.array([1.0, 2.0, 3.0]))
    N1 = (tilt / np.linalg.norm(tilt, axis=1, keepdims=True)).astype(F)
    for a in (V0, N0, V1, N1):
        a.setflags(write=False)
    mesh = {"00": (V0, N0, None), "10": (V1, N0, None), "11": (V1, N1, None)}
    return dict(make=_lights_builder, camera=cornell_camera(W, H), prm=params(), mesh=mesh)


# ------------------------------------------------------------------ oracle references of shade and lights
def case_of(family, point=False):
    return shade_case(point) if family == "shade" else lights_case()


@functools.lru_cache(maxsize=None)
def oracle_scene(family, key, point=False):
    from oracle import rgk_oracle as O
    c = case_of(family, point)
    sb = with_mesh(c["make"], *c["mesh"][key])
    desc = sb.to_desc()
    return O.OracleScene(desc), desc, sb


@functools.lru_cache(maxsize=None)
def oracle_round(family, key, reverse=0, point=False, cache_cam=None):
    """The oracle's round of the case's frame (cache_cam: through that view of cache_camera()) on mesh `key`, every ray answered by
    exhaustive search."""
    from oracle import rgk_oracle as O
    c = case_of(family, point)
    osc, _, _ = oracle_scene(family, key, point)
    return osc.render_round_split(cache_camera(cache_cam) if cache_cam else c["camera"], params(reverse), O.generate_task_list(W, H), exhaustive=True)


class _Exhaustive:
    """An OracleScene whose trace_closest answers by exhaustive search: what post_ref.oracle_features then composes from."""

    def __init__(self, osc):
        self.osc, self.h = osc, osc.h

    def trace_closest(self, rays, ignore=None):
        return self.osc.trace_closest_exhaustive(rays, ignore), None


@functools.lru_cache(maxsize=None)
def oracle_planes(key, point=False):
    """(albedo, normal, depth, tri) of the shade case's frame on mesh `key`."""
    from oracle import rgk_oracle as O
    import post_ref as R
    c = shade_case(point)
    osc, desc, _ = oracle_scene("shade", key, point)
    planes = R.oracle_features(O, _Exhaustive(osc), desc, c["camera"], W, H, c["bump"])
    for p in planes:
        p.setflags(write=False)
    return planes


def bump_mapped_pixels(key, point=False):
    """(y, x) bool: the first hit lies on a material with a bump texture."""
    _, _, sb = oracle_scene("shade", key, point)
    tri = oracle_planes(key, point)[3]
    bumped = np.array([m["tex_bump"] >= 0 for m in sb.materials])
    return (tri >= 0) & bumped[sb.FM[np.where(tri >= 0, tri, 0)]]


# ------------------------------------------------------------------ geometry
N_RAYS = 10000
SMALLER = {"count257": 6000}
COLLAPSED = (10, 20, 30, 40, 50)   # of count65, by the `degenerate` move: the first three get two equal corners, the others three collinear ones


def _per_triangle(V0, offsets):
    return (V0.reshape(-1, 3, 3) + offsets[:, None, :]).reshape(-1, 3).astype(F)


def _up(V0):
    return (T.soup(65) * F(1e3) + np.array([1e4, -1e4, 1e4], F)).reshape(-1, 3).astype(F)


def _down(V0):
    return (T.soup(65) * F(1e-3)).reshape(-1, 3).astype(F)


def _lifted(V0):
    V1 = V0.copy()
    V1[:, 1] = (1.5 * np.sin(0.6 * V0[:, 0]) * np.cos(0.4 * V0[:, 2]) + 0.05 * V0[:, 0]).astype(F)
    return V1


def _flattened(V0):
    V1 = V0.copy()
    V1[:, 1] = 0.0
    return V1


def _apart(V0):
    return _per_triangle(V0, np.random.default_rng(21).normal(scale=1.5, size=(len(V0) // 3, 3)))


def _collapsed(V0):
    return _per_triangle(V0, -V0.reshape(-1, 3, 3).astype(np.float64).mean(axis=1))


def _scrambled(V0):
    lo, hi = V0.min(axis=0), V0.max(axis=0)
    return (lo + (hi - lo) * np.random.default_rng(22).uniform(0, 1, V0.shape)).astype(F)


def _degenerate(V0):
    P = V0.reshape(-1, 3, 3).copy()
    for t in COLLAPSED[:3]:
        P[t, 2] = P[t, 1]
    for t in COLLAPSED[3:]:   # corners on a 1/64 grid, v1 = v0 + d, v2 = v0 + 2 d: every difference and product is exact, the cross product is 0
        v0 = np.round(P[t, 0] * 64) / 64
        d = np.round((P[t, 1] - P[t, 0]) * 64) / 64 + np.array([1, 0, 0]) / 64
        P[t] = np.stack([v0, v0 + d, v0 + 2 * d])
    return P.reshape(-1, 3).astype(F)


FLAT_RAYS = dict(in_plane_y=0.0, inside=((0.0, 0.0, 0.0), 6.0))   # (the box is a slab: origins inside it would only see the triangles edge-on)
GEOMETRY = {   # name -> (scene of trace_ref.SCENES, V0 -> V1, ray_mix keywords {step: ...})
    "count65-up-1e3": ("count65", _up, {}),
    "count65-down-1e-3": ("count65", _down, {}),
    "flat-lifted": ("flat", _lifted, {"back": FLAT_RAYS}),
    "count65-flattened": ("count65", _flattened, {"moved": FLAT_RAYS}),
    "duplicates-apart": ("duplicates", _apart, {}),
    "count64-collapsed": ("count64", _collapsed, {}),
    "count1-twisted": ("count1", twist_and_swell, {}),
    "count2-twisted": ("count2", twist_and_swell, {}),
    "count3-twisted": ("count3", twist_and_swell, {}),
    "count257-scrambled": ("count257", _scrambled, {}),
    "count65-degenerate": ("count65", _degenerate, {}),
}


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    """(scene name, V0, V1)."""
    scene, move, _ = GEOMETRY[name]
    V0 = T.SCENES[scene]().finalize().V.copy()
    V1 = np.ascontiguousarray(move(V0), dtype=F)
    assert V1.shape == V0.shape
    V0.setflags(write=False); V1.setflags(write=False)
    return scene, V0, V1


def aimed_at(osc, points, seed):
    """One ray per point from inside the scene box, aimed at it in float32."""
    rng = np.random.default_rng(seed)
    lo, hi = T.box_of(osc.info())
    o = (lo + (hi - lo) * rng.uniform(0.1, 0.9, (len(points), 3))).astype(F)
    v = (np.asarray(points, F) - o).astype(F)
    d = v / np.sqrt((v * v).sum(axis=1, dtype=F))[:, None]
    return np.concatenate([o, d, np.zeros((len(o), 1), F), np.full((len(o), 1), 10000.0, F)], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def geometry_reference(name):
    """[(step, V, oracle scene, rays, exhaustive hits, ignore, exhaustive hits with it, a, b, exhaustive visibility)] for the
    steps "moved" and "back".  The degenerate case's rays end with one aimed at a corner of each collapsed triangle."""
    from oracle import rgk_oracle as O
    scene, V0, V1 = geometry_case(name)
    n = SMALLER.get(scene, N_RAYS)
    steps = []
    for step, V in (("moved", V1), ("back", V0)):
        sb = with_mesh(T.SCENES[scene], V)
        osc = O.OracleScene(sb.to_desc())
        rays = T.ray_mix(osc, n, seed=31, targets=T.targets_of(sb), **GEOMETRY[name][2].get(step, {}))
        if name == "count65-degenerate" and step == "moved":
            rays = np.concatenate([rays, aimed_at(osc, V.reshape(-1, 3, 3)[list(COLLAPSED), 0], seed=33)])
        ex = osc.trace_closest_exhaustive(rays)
        ig = ex["tri"].astype(np.int32)
        ex2 = osc.trace_closest_exhaustive(rays, ig)
        a, b = T.visibility_pairs(osc, n, seed=32)
        vis = osc.visibility_exhaustive(a, b)
        for x in (rays, ex, ig, ex2, a, b, vis):
            x.setflags(write=False)
        steps.append((step, V, osc, rays, ex, ig, ex2, a, b, vis))
    return steps
