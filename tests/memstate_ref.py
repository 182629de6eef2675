"""Named cases for tests/test_gpu_memstate.py: every entry of the library run once, on a scene handle of its own, returning
every output it can reach as numpy arrays.  The test runs each case twice -- in the pytest process on fresh (in practice zero)
device memory, and in a child process with RGK_POISON=1, where every fresh device allocation of the library starts as 0xFF
bytes -- and asks for the same bits.  A third state of device memory, the leftovers of a larger and different frame in buffers
that DevBuf::alloc keeps, is the "stale" pair of cases.

    CASES      name -> function(rd) -> {key: numpy array}; keys that start with "_" are measurements of the run (poisoned bytes
               across a build), not outputs, and are not compared between runs
    FAMILIES   family -> case names; the test starts one child per family
    ROUNDS     name -> RoundSpec of every render-round case: what the test needs to ask the oracle for the same round

As a script:  python tests/memstate_ref.py --cases a,b,... | --family f  --out file.npz
runs the cases in this process, prints rgk_debug_poisoned_bytes() behind each and writes the arrays as "<case>::<key>".

Shapes are the smallest at which the kernels can still go wrong: frames of 67 x 45 (ragged against the 8 x 8 slot blocks and the
32 x 32 tiles), 8 spp, depth 5 unless a case says otherwise."""
import argparse
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from rgk_amd import capi  # noqa: E402
from rgk_amd.config import make_camera, make_params  # noqa: E402

import chain_ref as CR  # noqa: E402
import pad_ref as PAD  # noqa: E402
import refit_cases as RC  # noqa: E402
import trace_ref as T  # noqa: E402

F = np.float32
W, H, SPP, DEPTH = 67, 45, 8, 5
POISON_WORD = 0xFFFFFFFF
# bytes per reference of the device builder's scratch (rgk_build.hip rgk_build_bvh4_device): prims 44, keys + keys_sorted 16,
# left / right / parent / leaf_parent / arrived 20, first + count 8, nbox 24, fa + fb 16; the clustering adds cid / cid2 / nn 12,
# cbox / cbox2 48, cnum / cnum2 / keep / pos / place 20, keys_tree 8, leaf_parent_tree 4.  hipcub's storage comes on top.
BUILD_TMP_BYTES = 44 + 16 + 20 + 8 + 24 + 16
PLOC_TMP_BYTES = 12 + 48 + 20 + 8 + 4
# ... and of the refit (rgk_refit_bvh4_device): refbox 24 per reference; nbox 24, parent / n_inner / arrived 12 per node
REFIT_REF_BYTES, REFIT_NODE_BYTES = 24, 36


def poisoned():
    return int(capi.load_product().rgk_debug_poisoned_bytes())


def bits(a):
    """The uint32 words of an array of any dtype (bytes are widened, 64-bit words split)."""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 1:
        return a.astype(np.uint32).reshape(-1)
    return a.reshape(-1).view(np.uint32)


def counters_of(k, fields=("paths", "path_rays", "shadow_rays")):
    return np.array([int(getattr(k, f)) for f in fields], np.uint64)


def hit_arrays(prefix, hits):
    return {f"{prefix}.{f}": np.ascontiguousarray(hits[f]) for f in ("t", "tri", "a", "b", "c")}


def params(w=W, h=H, spp=SPP, depth=DEPTH, reverse=0, russian=0.7):
    return make_params(w, h, spp, depth, clamp=30.0, russian=russian, bumpscale=2.0, reverse=reverse)


def small_scene():
    from test_gpu_const_light import small_scene as mk
    return mk()


def small_camera(w=W, h=H):
    return make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=w, yres=h, focus_plane=5.0)


CASES = {}
FAMILIES = {"unit": [], "rounds": [], "bidirectional": [], "post": [], "builder": [], "stale": []}


def case(family, name):
    def add(fn):
        assert name not in CASES and "::" not in name
        CASES[name] = fn
        FAMILIES[family].append(name)
        return fn
    return add


# ======================================================================= unit entries
def exhaustive_ref(scene):
    """test_gpu_exhaustive's per-scene reference (made once per process): builder, oracle scene, fixed rays and pairs, answers."""
    import test_gpu_exhaustive as EX
    return EX._reference(scene)


def dense_rays(scene, n):
    """The first n of the scene's fixed rays in the order of test_gpu_exhaustive._dense_order: three of four hit, the last one too."""
    import test_gpu_exhaustive as EX
    ref = exhaustive_ref(scene)
    sel = EX._dense_order(scene)[:n]
    return ref, sel


def _closest(n):
    def run(rd):
        import test_gpu_exhaustive as EX
        ref, sel = dense_rays("duplicates", n)
        g = EX.gpu_scene(rd, ref["sb"], "host-sah")
        out = {}
        h0, _ = g.trace_closest(ref["rays"][sel])
        h1, _ = g.trace_closest(ref["rays"][sel], ref["ignore"][sel])
        h2, c = g.trace_closest(ref["rays"][sel], count=True)
        out.update(hit_arrays("plain", h0)); out.update(hit_arrays("ignore", h1)); out.update(hit_arrays("counted", h2))
        out["counters"] = counters_of(c, ("node_visits", "tri_tests", "path_rays"))
        g.close()
        return out
    return run


for _n in (1, 65, 4097):
    case("unit", f"unit.closest-n{_n}")(_closest(_n))


@case("unit", "unit.visibility")
def _visibility(rd):
    import test_gpu_exhaustive as EX
    ref = exhaustive_ref("duplicates")
    g = EX.gpu_scene(rd, ref["sb"], "host-sah")
    out = {}
    for n in (1, 65, 4097):
        v, _ = g.visibility(ref["a"][:n], ref["b"][:n])
        out[f"visible-n{n}"] = v
    v, c = g.visibility(ref["a"][:4097], ref["b"][:4097], count=True)
    out["visible-counted"] = v
    out["counters"] = counters_of(c, ("shadow_node_visits", "shadow_tri_tests", "shadow_rays"))
    g.close()
    return out


N_UNIT = 193   # three waves and one lane


@case("unit", "unit.bxdf")
def _bxdf(rd):
    from test_gpu_parity import _unit_dirs, material_zoo
    sb = material_zoo()
    g = rd.Scene(sb.to_desc())
    lib, n = g.lib, N_UNIT
    rng = np.random.default_rng(41)
    mat = (np.arange(n) % len(sb.materials)).astype(np.uint32)
    Vi, Vr = _unit_dirs(rng, n), _unit_dirs(rng, n)
    Vr[::3] = Vi[::3] * np.array([-1, -1, 1], F)
    uv = rng.uniform(-1, 2, (n, 2)).astype(F)
    u = rng.uniform(0, 1, (n, 2)).astype(F)
    out = {}
    for route in (0, 1):
        val = np.zeros((n, 3), F); d = np.zeros((n, 3), F); w = np.zeros((n, 3), F); leak = np.zeros(n, np.uint8)
        capi.check(lib, lib.rgk_bxdf_value(g.h, n, route, mat.ctypes.data, Vi.ctypes.data, Vr.ctypes.data, uv.ctypes.data, val.ctypes.data))
        capi.check(lib, lib.rgk_bxdf_sample(g.h, n, route, mat.ctypes.data, Vi.ctypes.data, uv.ctypes.data, u.ctypes.data, d.ctypes.data, w.ctypes.data, leak.ctypes.data))
        out.update({f"route{route}.value": val, f"route{route}.dir": d, f"route{route}.weight": w, f"route{route}.may_leak": leak})
    g.close()
    return out


@case("unit", "unit.texture")
def _texture(rd):
    from rgk_amd.scene import SceneBuilder
    sb = SceneBuilder()
    rng = np.random.default_rng(42)
    ids = [sb.create_solid_texture((0.2, 0.5, 0.9)), sb.add_image_texture("f32", rng.random((37, 53, 3)).astype(F) * 3.0),
           sb.add_image_texture8("u8", rng.integers(0, 256, (29, 64, 3), dtype=np.uint8))]
    m = sb.new_material("m", capi.BXDF_DIFFUSE); m["tex_diffuse"] = ids[0]; sb.register_material(m)
    sb.add_primitive("cube", np.eye(4, dtype=F), "m")
    g = rd.Scene(sb.to_desc())
    n = N_UNIT
    tex = np.array([ids[i % 3] for i in range(n)], np.int32)
    uv = rng.uniform(-2, 3, (n, 2)).astype(F)
    uv[::7] = np.round(uv[::7] * 8) / 8
    rgb = np.zeros((n, 3), F); sr = np.zeros(n, F); sbm = np.zeros(n, F)
    capi.check(g.lib, g.lib.rgk_texture_sample(g.h, n, tex.ctypes.data, uv.ctypes.data, rgb.ctypes.data, sr.ctypes.data, sbm.ctypes.data))
    g.close()
    return {"rgb": rgb, "slope_right": sr, "slope_bottom": sbm}


@case("unit", "unit.sampler")
def _sampler(rd):
    rng = np.random.default_rng(43)
    n = N_UNIT
    seed = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    idx = rng.integers(0, 4096, n).astype(np.uint32)
    dim = (np.arange(n) % 40).astype(np.uint32)
    return {"u2": rd.sampler_eval(seed, idx, dim, 1), "u1": rd.sampler_eval(seed, idx, dim, 0)}


@case("unit", "unit.libm")
def _libm(rd):
    lib = capi.load_product()
    rng = np.random.default_rng(44)
    n = N_UNIT
    x = np.concatenate([rng.uniform(-50, 50, n - 4), [0.0, -0.0, np.pi, 1e-30]]).astype(F)
    u = np.concatenate([rng.uniform(-1, 1, n - 4), [1, -1, 0, 0.5]]).astype(F)
    y = rng.normal(size=n).astype(F)
    out = {}
    for fn, a, b in ((0, x, x), (1, x, x), (2, u, u), (3, u, u), (4, x, y)):
        r = np.zeros(n, F)
        capi.check(lib, lib.rgk_libm_eval(fn, n, a.ctypes.data, b.ctypes.data, r.ctypes.data))
        out[f"fn{fn}"] = r
    return out


# ======================================================================= rounds
class RoundSpec:
    """One render-round case.  oracle_key: the cases that share it render the same round (same scene, camera, parameters and
    tiles) and are held to ONE oracle round.  make() -> (builder, camera).  builder_name: a key of test_gpu_exhaustive.BUILDERS.
    refit_from() -> the builder the handle is created from; it is then refitted (rgk_scene_refit with vertices, normals and
    tangents) to the mesh of make()'s builder, the one the oracle renders."""

    def __init__(self, oracle_key, make, prm, rounds=1, tuning=None, builder_name=None, refit_from=None):
        self.oracle_key, self.make, self.prm, self.rounds, self.tuning, self.builder_name = oracle_key, make, prm, rounds, tuning or {}, builder_name
        self.refit_from = refit_from


ROUNDS = {}


def gpu_scene_of(rd, spec, sb):
    if spec.builder_name:
        import test_gpu_exhaustive as EX
        return EX.gpu_scene(rd, sb, spec.builder_name)
    return rd.Scene(sb.to_desc())


def run_round(rd, spec):
    sb, cam = spec.make()
    if spec.refit_from:
        g = gpu_scene_of(rd, spec, spec.refit_from())
        sb.finalize()
        g.refit(sb.V, sb.N, sb.T)
    else:
        g = gpu_scene_of(rd, spec, sb)
    if spec.tuning:
        g.set_tuning(**spec.tuning)
    tiles = rd.generate_task_list(spec.prm.xres, spec.prm.yres)
    out = {}
    for r in range(spec.rounds):   # one frame, separate accumulators: from the second round on the entry lists are capped
        a, c, k = g.render_round(cam, spec.prm, tiles)
        out.update({f"round{r}.accum": a, f"round{r}.count": c, f"round{r}.counters": counters_of(k)})
    i = g.info()
    out["info"] = np.array([i.n_nodes, i.max_depth, i.n_leaf_refs, i.const_light], np.uint32)
    g.close()
    return out


def round_case(family, name, spec):
    ROUNDS[name] = spec
    case(family, name)(lambda rd, spec=spec: run_round(rd, spec))


def _small():
    return small_scene(), small_camera()


for _cl in (0, 1):
    for _lv in (0, 1):
        for _beam in (0, 2):
            for _ep in (0, 1):
                round_case("rounds", f"round.small-const_light{_cl}-last_vertex{_lv}-beam{_beam}-entry_points{_ep}",
                           RoundSpec("small", _small, params(), rounds=2, tuning=dict(const_light=_cl, last_vertex=_lv, beam=_beam, entry_points=_ep)))
round_case("rounds", "round.small-two-sample-passes", RoundSpec("small", _small, params(), rounds=2, tuning=dict(batch_paths=W * H * SPP // 2)))
round_case("rounds", "round.small-5x3", RoundSpec("small-5x3", lambda: (small_scene(), small_camera(5, 3)), params(5, 3, 1, 1)))


def _zoo():
    from test_bdpt_cpu import zoo_builder, zoo_camera
    return zoo_builder(), zoo_camera(W, H)


def _deep():
    import test_gpu_exhaustive as EX
    assert (EX.ROUND_W, EX.ROUND_H) == (W, H)
    return EX._round_scene("deep")


def _cornell(light, size=0.0):
    def make():
        from test_bdpt_cpu import cornell_builder, cornell_camera
        return cornell_builder(light, size), cornell_camera(W, H)
    return make


def _envmap():
    from test_gpu_parity import envmap_sky_scene
    return envmap_sky_scene(), make_camera((2.5, 1.8, 3.0), (0, 0.4, 0), (0, 1, 0), fov=50, xres=W, yres=H)


round_case("rounds", "round.zoo-lens-depth8-no-roulette", RoundSpec("zoo", _zoo, params(depth=8, russian=-1.0)))
round_case("rounds", "round.deep-overflow-area", RoundSpec("deep", _deep, params(), builder_name="host-sah-stack256-lds16"))
round_case("rounds", "round.small-padded-P60-K3", RoundSpec("small-padded", lambda: (PAD.pad(small_scene(), 60, 3), small_camera()), params()))
round_case("rounds", "round.cornell-sphere-light", RoundSpec("cornell-sphere", _cornell("point", 0.15), params()))
round_case("rounds", "round.cornell-emissive-quad", RoundSpec("cornell-quad", _cornell("quad"), params()))
round_case("rounds", "round.envmap-float-sky", RoundSpec("envmap", _envmap, params()))



def _refitted_point_scene():
    c = RC.shade_case(point=True)
    return RC.with_mesh(c["make"], *c["mesh"]["111"]), c["camera"]


# a round on a refitted handle of the constant-light scene: the shading records k_refit_shade rewrote, on the refit's scratch
for _b in ("host-sah", "device"):
    round_case("rounds", f"round.refit-shade-{_b}", RoundSpec("refit-shade", _refitted_point_scene, params(), builder_name=_b,
                                                              refit_from=RC.shade_case(point=True)["make"]))

# bidirectional rounds: the splat order is not repeatable, so these are held to the oracle's terms, never to each other
round_case("bidirectional", "bidir.small-reverse3", RoundSpec("small-reverse3", _small, params(reverse=3)))


def _cornell64():
    from test_bdpt_cpu import cornell_builder, cornell_camera
    return cornell_builder(), cornell_camera(64, 64)


round_case("bidirectional", "bidir.cornell-reverse7-depth8", RoundSpec("cornell-reverse7", _cornell64, params(64, 64, 4, 8, reverse=7)))


# ======================================================================= post kernels
def every_other(tiles):
    sub = [tiles[i] for i in range(0, len(tiles), 2)]
    return (capi.Tile * len(sub))(*sub)


def tiles_mask(tiles, w, h):
    m = np.zeros((h, w), bool)
    for t in tiles:
        m[t.y0:t.y1, t.x0:t.x1] = True
    return m


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def poisoned_plane(*shape):
    """A caller's output buffer on the device that starts as 0xFF bytes."""
    import torch
    t = torch.from_numpy(np.full(shape, POISON_WORD, np.uint32).view(F)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def written(name, a):
    """No element of a fully written output may still hold the 0xFF pattern the buffer started with."""
    a = a.cpu().numpy()
    left = int((bits(a) == POISON_WORD).sum())
    assert left == 0, f"{name}: {left} elements were never written"
    return a


class PostInputs:
    """A fresh handle of the small scene with what the post entries read: two rounds with different seeds (total = both, half =
    the second), and the first-hit feature planes of the whole frame."""

    def __init__(self, rd):
        self.g = rd.Scene(small_scene())   # (the handle keeps the builder: the descriptor points into its arrays)
        cam, prm = small_camera(), params()
        self.cam, self.prm = cam, prm
        self.tiles = rd.generate_task_list(W, H)
        a0, c0, _ = self.g.render_round(cam, prm, self.tiles)
        a1, c1, _ = self.g.render_round(cam, prm, rd.generate_task_list(W, H, seedcount_base=len(self.tiles)))
        self.round = (a1, c1)
        self.total = ((a0 + a1).astype(F), c0 + c1)
        self.first = (a0, c0)
        self.albedo, self.normal, self.depth, self.tri = self.g.render_aov(cam, prm, self.tiles)


@case("post", "post.aov-every-other-tile")
def _aov(rd):
    g = rd.Scene(small_scene())
    tiles = every_other(rd.generate_task_list(W, H))
    alb, nrm, z, tri = g.render_aov(small_camera(), params(), tiles, sentinel=7)
    g.close()
    outside = ~tiles_mask(tiles, W, H)
    assert outside.any() and (alb[outside] == 7).all() and (nrm[outside] == 7).all() and (z[outside] == 7).all() and (tri[outside] == 7).all(), \
        "a pixel outside the tiles lost the sentinel"
    return {"albedo": alb, "normal": nrm, "depth": z, "tri": tri}


@case("post", "post.aov-chain-hall-8-hops")
def _aov_chain(rd):
    g = rd.Scene(CR.hall())
    tiles = every_other(rd.generate_task_list(CR.HALL_W, CR.HALL_H))
    alb, nrm, z, tri, hops = g.render_aov_chain(CR.hall_camera(), CR.hall_params(), tiles, 8, sentinel=7)
    g.close()
    outside = ~tiles_mask(tiles, CR.HALL_W, CR.HALL_H)
    assert outside.any() and (alb[outside] == 7).all() and (nrm[outside] == 7).all() and (z[outside] == 7).all() and (tri[outside] == 7).all() and (hops[outside] == 7).all(), \
        "a pixel outside the tiles lost the sentinel"
    return {"albedo": alb, "normal": nrm, "depth": z, "tri": tri, "hops": hops}


@case("post", "post.denoise")
def _denoise(rd):
    import torch
    p = PostInputs(rd)
    t = [up(x) for x in p.total + (p.albedo, p.normal, p.depth)]
    out = poisoned_plane(H, W, 3)
    level = float(np.max(p.total[0] / p.total[1][..., None].astype(F), axis=-1).astype(np.float64).mean())
    p.g.denoise_device(W, H, *[x.data_ptr() for x in t], capi.DenoiseParams(sigma_color=6.0 * level), out.data_ptr())
    torch.cuda.synchronize()
    res = {"rgb": written("denoise rgb", out)}
    p.g.close()
    return res


@case("post", "post.denoise-variance")
def _denoise_variance(rd):
    import torch
    p = PostInputs(rd)
    t = [up(x) for x in p.total + p.round + (p.albedo, p.normal, p.depth)]
    out, var = poisoned_plane(H, W, 3), poisoned_plane(H, W)
    p.g.denoise_variance_device(W, H, *[x.data_ptr() for x in t], capi.DenoiseVarParams(), out.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    res = {"rgb": written("denoise-variance rgb", out), "variance": written("denoise-variance variance", var)}
    p.g.close()
    return res


@case("post", "post.noise-estimate-tile5")
def _noise(rd):
    import torch
    p = PostInputs(rd)
    t = [up(x) for x in p.total + p.round]
    var = poisoned_plane(H, W)
    with_plane = p.g.noise_estimate_device(W, H, 5, *[x.data_ptr() for x in t], var.data_ptr())
    without = p.g.noise_estimate_device(W, H, 5, *[x.data_ptr() for x in t], None)
    torch.cuda.synchronize()
    res = {"variance": written("noise variance", var)}
    for name, tiles in (("with-plane", with_plane), ("without-plane", without)):
        for f in ("sum_var", "sum_sq", "n_estimable"):
            res[f"{name}.{f}"] = np.ascontiguousarray(tiles[f])
    p.g.close()
    return res


@case("post", "post.round-fold")
def _fold(rd):
    import torch
    p = PostInputs(rd)
    tiles = every_other(p.tiles)
    flags = (np.arange(len(tiles)) % 2).astype(np.uint8)
    rng = np.random.default_rng(45)
    half = ((rng.random((H, W, 3)) * 3).astype(F), rng.integers(1, 100, (H, W)).astype(np.uint32))   # (all six planes are read and written: none starts poisoned)
    t = [up(x) for x in p.round + p.first + half]
    torch.cuda.synchronize()
    p.g.round_fold_device(W, H, tiles, flags, *[x.data_ptr() for x in t])
    torch.cuda.synchronize()
    names = ("round.rgb", "round.count", "total.rgb", "total.count", "half.rgb", "half.count")
    res = {n: x.cpu().numpy() for n, x in zip(names, t)}
    p.g.close()
    return res


# ======================================================================= the device builder and the refit
DEVICE_BUILDERS = ("device", "device-karras", "device-karras-rotate4")


def _built(scene, builder):
    def run(rd):
        import test_gpu_exhaustive as EX
        ref = exhaustive_ref(scene)
        before = poisoned()
        g = EX.gpu_scene(rd, ref["sb"], builder)
        after = poisoned()
        i = g.info()
        out = {"info": np.array([i.n_nodes, i.max_depth, i.n_leaf_refs], np.uint32)}
        out.update(hit_arrays("closest", g.trace_closest(ref["rays"])[0]))
        out.update(hit_arrays("ignore-first", g.trace_closest(ref["rays"], ref["ignore"])[0]))
        out["visible"] = g.visibility(ref["a"], ref["b"])[0]
        out["_poisoned_by_create"] = np.array([after - before], np.uint64)
        g.close()
        return out
    return run


for _s in ("count257", "duplicates", "deep"):
    for _b in DEVICE_BUILDERS:
        case("builder", f"builder.{_s}-{_b}")(_built(_s, _b))


def refit_moves(scene):
    """(() -> builder, [(step, vertices, normals or None, tangents or None)]) of a refit case: a scene of trace_ref.SCENES under the
    twist and swell of refit_cases.py, positions only; "shade" and "lights" of refit_cases.py, with their normals and tangents."""
    if scene == "shade":
        c = RC.shade_case()
        return c["make"], [("moved",) + c["mesh"]["111"], ("back",) + c["mesh"]["000"]]
    if scene == "lights":
        c = RC.lights_case()
        return c["make"], [("moved",) + c["mesh"]["11"], ("back",) + c["mesh"]["00"]]
    V0 = T.SCENES[scene]().finalize().V.copy()
    return T.SCENES[scene], [("moved", RC.twist_and_swell(V0), None, None), ("back", V0, None, None)]


@functools.lru_cache(maxsize=None)
def refit_setup(scene):
    """The moved / back refit of test_refitted_tree_equals_the_exhaustive_search_on_the_moved_mesh, made once per process:
    (builder, [(step, vertices, oracle scene of the moved mesh, rays, a, b)])."""
    from oracle import rgk_oracle as O
    make, moves = refit_moves(scene)
    sb = make()
    sb.finalize()
    ctr = sb.V.mean(axis=0)
    steps = []
    n = 4097
    for step, V, N, Tn in moves:
        moved = RC.with_mesh(make, V, N, Tn)
        osc = O.OracleScene(moved.to_desc())
        kw = dict(inside=(tuple(ctr), 0.5)) if scene == "closed" else {}
        rays = T.ray_mix(osc, n, seed=7, targets=T.targets_of(moved), **kw)
        a, b = T.visibility_pairs(osc, n, seed=8)
        steps.append((step, V, osc, rays, a, b))
    return sb, steps


def _refitted(scene, builder):
    def run(rd):
        import test_gpu_exhaustive as EX
        sb, steps = refit_setup(scene)
        attrs = {step: (N, Tn) for step, _, N, Tn in refit_moves(scene)[1]}
        g = EX.gpu_scene(rd, sb, builder)
        i = g.info()
        out = {"info": np.array([i.n_nodes, i.max_depth, i.n_leaf_refs], np.uint32)}
        for step, V, osc, rays, a, b in steps:
            before = poisoned()
            g.refit(V, *attrs[step])
            out[f"_poisoned_by_refit.{step}"] = np.array([poisoned() - before], np.uint64)
            out.update(hit_arrays(f"{step}.closest", g.trace_closest(rays)[0]))
            out[f"{step}.visible"] = g.visibility(a, b)[0]
        g.close()
        return out
    return run


REFITS = [(s, b) for s in ("closed", "count257", "shade", "lights") for b in ("host-sah", "device")]
for _s, _b in REFITS:
    case("builder", f"refit.{_s}-{_b}")(_refitted(_s, _b))


# ======================================================================= stale contents
def _two_small_renders(rd, g):
    """The 33 x 31 x 5 spp depth 3 round, then the 5 x 3 x 1 spp depth 1 round."""
    out = {}
    for name, (w, h, spp, depth) in (("33x31", (33, 31, 5, 3)), ("5x3", (5, 3, 1, 1))):
        a, c, k = g.render_round(small_camera(w, h), params(w, h, spp, depth), rd.generate_task_list(w, h))
        out.update({f"{name}.accum": a, f"{name}.count": c, f"{name}.counters": counters_of(k)})
    return out


@case("stale", "stale.after-a-larger-frame")
def _stale(rd):
    """On one handle: a 100 x 70 x 16 spp depth 8 bidirectional round, an 8-hop feature chain and a 4097-ray probe -- every buffer of
    the scene then holds their leftovers and DevBuf::alloc keeps it for the smaller requests that follow."""
    g = rd.Scene(small_scene())
    w, h = 100, 70
    cam, tiles = small_camera(w, h), rd.generate_task_list(w, h)
    g.render_round(cam, params(w, h, 16, 8, reverse=3), tiles)
    g.render_aov_chain(cam, params(w, h, 1, 8), tiles, 8)
    i = g.info()
    rng = np.random.default_rng(46)
    lo, hi = np.array(list(i.bbox_min), np.float64), np.array(list(i.bbox_max), np.float64)
    o, d = T.random_rays(rng, lo, hi, 4097)
    rays = np.concatenate([o, d, np.zeros((4097, 1), F), np.full((4097, 1), 10000.0, F)], axis=1).astype(F)
    hits, _ = g.trace_closest(rays, count=True)
    g.visibility(o, np.roll(o, 1, axis=0))   # (distinct random points: no pair is a == b)
    assert (hits["tri"] >= 0).mean() > 0.5
    out = _two_small_renders(rd, g)
    g.close()
    return out


@case("stale", "stale.fresh-handle")
def _fresh(rd):
    g = rd.Scene(small_scene())
    out = _two_small_renders(rd, g)
    g.close()
    return out


# ======================================================================= running cases
def run_cases(rd, names, report=None):
    """{case: {key: array}}; report(case, poisoned bytes so far) behind each."""
    out = {}
    for name in names:
        out[name] = CASES[name](rd)
        if report:
            report(name, poisoned())
    return out


def flatten(results, poison):
    flat = {}
    for name, arrays in results.items():
        for key, a in arrays.items():
            flat[f"{name}::{key}"] = np.ascontiguousarray(a)
        flat[f"{name}::_poisoned_total"] = np.array([poison[name]], np.uint64)
    return flat


def unflatten(npz):
    out = {}
    for full in npz.files:
        name, key = full.split("::", 1)
        out.setdefault(name, {})[key] = npz[full]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default="")
    ap.add_argument("--family", default="")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    names = [c for c in args.cases.split(",") if c] + (FAMILIES[args.family] if args.family else [])
    unknown = [c for c in names if c not in CASES]
    if unknown or not names:
        ap.error(f"unknown or no cases: {unknown}")
    from rgk_amd import render_driver as rd
    lib = capi.load_product()
    assert lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    poison_on = "RGK_POISON" in os.environ
    if poison_on:   # a poison run that poisoned nothing proves nothing: checked behind the first scene that is created, and every later one
        create = rd.Scene.__init__

        def checked(self, *a, **kw):
            create(self, *a, **kw)
            assert poisoned() > 0, "RGK_POISON is set and rgk_scene_create filled nothing"
        rd.Scene.__init__ = checked
    else:
        assert poisoned() == 0
    poison = {}

    def report(name, total):
        poison[name] = total
        print(f"{name}: rgk_debug_poisoned_bytes() = {total}", flush=True)
    results = run_cases(rd, names, report)
    assert (poisoned() > 0) == poison_on
    np.savez(args.out, **flatten(results, poison))
    print("memstate ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
