"""GPU suite (-m gpu): the HIP walkers against the exhaustive-search reference, with no excuse list.

The walkers' contract (rgk_amd/csrc/rgk_trace.h) names no tree: the nearest accepted hit with t in [t0 - eps, t1 + eps], [t0, t1]
the ray's [near, far] clipped to the epsilon-padded scene box, exact ties to the higher triangle id, any-hit in the same window.
OracleScene.trace_closest_exhaustive / visibility_exhaustive test every triangle under exactly that rule with the kernels' own
triangle test, so for every builder, tree, stack variant and ray count the bar is

    tri equal for every ray; t, a, b, c equal bit for bit (a miss is t = +inf, a = b = c = 0 on both sides);
    visibility bytes equal for every pair -- no tie band, no `unexplained` allowance.

Scenes (tests/trace_ref.py) are the small and degenerate ones the other traversal tests never build: 1 ... 257 triangles, a flat
scene, one centroid for every triangle, coincident runs, a closed mesh hit at its vertices and edges, a deep tree from 1 200
triangles, the same soup at 1e-3 and at 1e3 far from the origin.  Every test records rays, hits and differing (0).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params

from conftest import record_parity
import trace_ref as T

pytestmark = pytest.mark.gpu

N_RAYS = 20000
SMALLER = {"deep": (10000, 10000)}    # (rays, pairs): 1 200 triangles -- three exhaustive traces + the pairs stay under 5e7 triangle tests
BUILDERS = {   # name -> (build flags, environment of rgk_scene_create)
    "host-sah": (capi.BUILD_HOST_SAH, {}),
    "device": (capi.BUILD_DEVICE, {}),                                                              # clustering (the default)
    "device-karras": (capi.BUILD_DEVICE, {"RGK_LBVH_PLOC": "0", "RGK_LBVH_ROTATE": "0"}),
    "device-karras-rotate4": (capi.BUILD_DEVICE, {"RGK_LBVH_PLOC": "0", "RGK_LBVH_ROTATE": "4"}),
    # the walkers' <STACK, LDSN> variants (rgk_plan.h rgk_walker_variant): 256/16 is what the four above run
    "host-sah-stack256-lds16": (capi.BUILD_HOST_SAH, {"RGK_STACK_OVF": "1", "RGK_STACK_LDS": "16"}),
    "host-sah-stack256-lds32": (capi.BUILD_HOST_SAH, {"RGK_STACK_OVF": "1", "RGK_STACK_LDS": "32"}),
    # all-LDS 32/32: taken only where max_stack + 1 + RGK_ENTRY_K <= 32 (rgk_round_plan.h rgk_stack_plan), else 256/16 runs without a
    # word.  Which one ran cannot be read through the C ABI; max_depth can, and max_stack <= 3 (max_depth + 1): see the test.
    "host-sah-stack32-lds32": (capi.BUILD_HOST_SAH, {"RGK_STACK_OVF": "0"}),
}
CASES = [(s, b) for s in T.SCENES for b in ("host-sah", "device", "device-karras", "device-karras-rotate4")]
CASES += [("deep", "host-sah-stack256-lds16"), ("deep", "host-sah-stack256-lds32"), ("count65", "host-sah-stack32-lds32"),
          ("duplicates", "host-sah-stack32-lds32"), ("closed", "host-sah-stack32-lds32"), ("closed", "host-sah-stack256-lds32")]
MAXLEAF_DEV = 2   # rgk_commit.h BuildOptions::max_leaf_dev: at or below it a device request is answered by the host builder


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def gpu_scene(rd, sb, builder):
    """rd.Scene of `sb` by `builder`; the build switches are read once, in rgk_scene_create, and restored here."""
    flags, env = BUILDERS[builder]
    old = {k: os.environ.get(k) for k in env}
    keep = getattr(sb, "build_flags", None)
    os.environ.update(env)
    sb.build_flags = flags
    try:
        return rd.Scene(sb.to_desc())
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        if keep is None:
            del sb.build_flags
        else:
            sb.build_flags = keep


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Per scene, once: the builder, the oracle scene, the rays and pairs, and the exhaustive answers every builder must equal."""
    from oracle import rgk_oracle as O
    sb = T.SCENES[name]()
    osc = O.OracleScene(sb.to_desc())
    n_rays, n_pairs = SMALLER.get(name, (N_RAYS, N_RAYS))
    kw = {}
    if name == "flat":                                  # (the box is a slab: origins inside it would only see the triangles edge-on)
        kw.update(in_plane_y=0.0, inside=((0.0, 0.0, 0.0), 6.0))
    if name == "closed":
        kw.update(inside=((0.0, 0.0, 0.0), 0.6), within=0.9)   # rays start inside the mesh (inradius 0.97): every one must come out through a triangle
    rays = T.ray_mix(osc, n_rays, seed=100 + len(name), targets=T.targets_of(sb), **kw)
    ex = osc.trace_closest_exhaustive(rays)
    ig = ex["tri"].astype(np.int32)
    ex2 = osc.trace_closest_exhaustive(rays, ig)
    a, b = T.visibility_pairs(osc, n_pairs, seed=200 + len(name))
    vis = osc.visibility_exhaustive(a, b)
    return dict(sb=sb, osc=osc, rays=rays, ex=ex, ignore=ig, ex2=ex2, a=a, b=b, vis=vis)


def assert_same_frame(g, osc):
    """The window of the rule is made of epsilon and the padded box: the two sides must hold the same floats."""
    gi, oi = g.info(), osc.info()
    assert gi.epsilon == oi.epsilon and list(gi.bbox_min) == list(oi.bbox_min) and list(gi.bbox_max) == list(oi.bbox_max)


def assert_equal_hits(name, rays, got, want):
    bad = T.differing(got, want)
    record_parity(name, rays=len(rays), hits=int((want["tri"] >= 0).sum()), differing=int(bad.sum()))
    assert not bad.any(), f"{name}: {int(bad.sum())} of {len(rays)} rays differ: " + T.describe(rays, got, want, bad)


@pytest.mark.parametrize("scene,builder", CASES, ids=[f"{s}-{b}" for s, b in CASES])
def test_closest_hit_and_visibility_equal_the_exhaustive_search(rd, scene, builder):
    """rgk_trace_closest (k_trace_closest), without and with `ignore` = the first hit, and rgk_trace_visibility against the
    exhaustive reference.  rgk_trace_visibility launches k_trace_shadow only (any-hit, 48-byte records): the constant-light
    kernels (k_trace_shadow_cl, k_trace_shadow_first_cl), k_trace_shadow_first and k_trace_shadow_jobs are reached through
    rgk_render_round alone and stay with the switches-never-change-a-result tests, whose base this pins."""
    ref = _reference(scene)
    g = gpu_scene(rd, ref["sb"], builder)
    assert_same_frame(g, ref["osc"])
    n_tri = len(ref["sb"].F)
    if builder.startswith("device") and n_tri <= MAXLEAF_DEV:
        assert g.info().n_nodes >= 1       # the host builder answered: the scene builds and (below) answers
    if scene == "deep" and builder.startswith("host-sah"):
        assert g.info().max_depth >= 11, g.info().max_depth      # 3 pushes per level: more than 32 stack entries possible
    if builder == "host-sah-stack32-lds32":   # 3 pushes per level and RGK_ENTRY_K = 6 entry nodes: max_depth <= 7 means at most 31 entries, the 32/32 walker
        assert g.info().max_depth <= 7, g.info().max_depth
    tag = f"gpu_exhaustive[{scene}-{builder}]"
    rays = ref["rays"]
    assert (ref["ex"]["tri"] >= 0).mean() > 0.25
    hg, _ = g.trace_closest(rays)
    assert_equal_hits(tag + ":closest", rays, hg, ref["ex"])
    hg2, _ = g.trace_closest(rays, ref["ignore"])
    assert_equal_hits(tag + ":ignore-first", rays, hg2, ref["ex2"])
    vg, _ = g.visibility(ref["a"], ref["b"])
    differ = int((vg != ref["vis"]).sum())
    record_parity(tag + ":visibility", pairs=len(vg), visible=float(ref["vis"].mean()), differing=differ)
    assert differ == 0, (differ, np.nonzero(vg != ref["vis"])[0][:10])
    g.close()


@functools.lru_cache(maxsize=None)
def _dense_order(scene):
    """An order of the scene's rays in which three of every four hit: position i with i % 4 == 1 holds a miss, every other one a
    hit, those that also hit with the first hit ignored first.  So the prefixes of 1, 63, 64 and 65 rays end in a hit."""
    ref = _reference(scene)
    rng = np.random.default_rng(17)
    hit, second = ref["ex"]["tri"] >= 0, ref["ex2"]["tri"] >= 0
    hits = np.concatenate([rng.permutation(np.nonzero(hit & second)[0]), rng.permutation(np.nonzero(hit & ~second)[0])])
    misses = rng.permutation(np.nonzero(~hit)[0])
    n = min(len(hits) * 4 // 3, len(misses) * 4, len(hit))
    order = np.empty(n, np.int64)
    is_miss = np.arange(n) % 4 == 1
    order[is_miss] = misses[:is_miss.sum()]
    order[~is_miss] = hits[:(~is_miss).sum()]
    return order


@pytest.mark.parametrize("scene", ["count65", "duplicates"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_ray_counts_at_the_edges_of_a_wave_and_of_the_refill(rd, scene, n):
    """The first n rays of an order dense in hits (three of four; on `duplicates` the first ~2 000 of them hit again with the
    first hit ignored): one lane, a wave less one, a full wave, a wave and one, and more than one static slice of the persistent
    walker's queue -- the last ray of each is a hit, so a lane that is dropped, swapped or mis-indexed at the end of a partial
    wave shows.  n = 0: rgk_trace_closest and rgk_trace_visibility return before any launch."""
    ref = _reference(scene)
    sel = _dense_order(scene)[:n]
    assert len(sel) == n
    rays, ig, ex, ex2 = ref["rays"][sel], ref["ignore"][sel], ref["ex"][sel], ref["ex2"][sel]
    if n:
        assert ex["tri"][-1] >= 0 and ex["tri"][0] >= 0 and (ex["tri"] >= 0).sum() >= (3 * n) // 4
        assert len(np.unique(ex["tri"][ex["tri"] >= 0])) >= min(n // 4, 8) or n == 1      # not one triangle over and over
        if scene == "duplicates":
            assert (ex2["tri"] >= 0).sum() >= n // 4 and (n > 65 or ex2["tri"][-1] >= 0)      # (about 2 300 rays hit twice: 4 097 outruns them)
    g = gpu_scene(rd, ref["sb"], "host-sah")
    hg, _ = g.trace_closest(rays)
    assert_equal_hits(f"gpu_exhaustive[ray-count {scene} {n}]:closest", rays, hg, ex)
    hg, _ = g.trace_closest(rays, ig)
    assert_equal_hits(f"gpu_exhaustive[ray-count {scene} {n}]:ignore-first", rays, hg, ex2)
    # pairs: every other one blocked as far as the scene has blocked pairs, the last one of the prefix among them
    blocked, free = np.nonzero(ref["vis"] == 0)[0], np.nonzero(ref["vis"] == 1)[0]
    m = min(n, 2 * len(blocked) - 1)
    pick = np.empty(m, np.int64)
    pick[(m - 1) % 2::2] = blocked[:len(pick[(m - 1) % 2::2])]
    pick[m % 2::2] = free[:len(pick[m % 2::2])]
    if m:
        assert ref["vis"][pick[-1]] == 0
    vg, _ = g.visibility(ref["a"][pick], ref["b"][pick])
    differ = int((vg != ref["vis"][pick]).sum())
    record_parity(f"gpu_exhaustive[ray-count {scene} {n}]:visibility", pairs=m, blocked=int((ref["vis"][pick] == 0).sum()), differing=differ)
    assert differ == 0
    g.close()


@pytest.mark.parametrize("builder", ["host-sah", "device"])
@pytest.mark.parametrize("scene", ["closed", "count257"])
def test_refitted_tree_equals_the_exhaustive_search_on_the_moved_mesh(rd, oracle, scene, builder):
    """rgk_scene_refit (k_refit_recs, k_qbvh_refit: new reference boxes, node boxes and 8-bit codes on the old topology): the
    vertices twisted about the vertical axis and swollen by a few per cent of the scene size, then moved back.  After each
    step the refitted scene must answer like the exhaustive search over the vertices it now holds -- aimed at their vertices
    and edge midpoints, where a node box one step too tight drops the hit."""
    sb = T.SCENES[scene]()
    sb.finalize()
    import refit_cases as RC
    V0 = sb.V.copy()
    ctr = V0.mean(axis=0)
    V1 = RC.twist_and_swell(V0)
    g = gpu_scene(rd, sb, builder)
    for step, V in (("moved", V1), ("back", V0)):
        g.refit(V)
        sb.vertices = [V]
        osc = oracle.OracleScene(sb.to_desc())
        assert_same_frame(g, osc)
        kw = dict(inside=(tuple(ctr), 0.5)) if scene == "closed" else {}
        rays = T.ray_mix(osc, N_RAYS, seed=7, targets=T.targets_of(sb), **kw)
        ex = osc.trace_closest_exhaustive(rays)
        assert (ex["tri"] >= 0).mean() > 0.25
        hg, _ = g.trace_closest(rays)
        assert_equal_hits(f"gpu_exhaustive[refit {scene}-{builder} {step}]", rays, hg, ex)
        a, b = T.visibility_pairs(osc, N_RAYS, seed=8)
        assert np.array_equal(g.visibility(a, b)[0], osc.visibility_exhaustive(a, b))
    g.close()


# ----------------------------------------------------------------------- the device builder's trees, pinned
FINGERPRINT_BUILDERS = ("device", "device-karras", "device-karras-rotate4")
FINGERPRINT_CASES = [(s, b) for s in T.SCENES for b in FINGERPRINT_BUILDERS]
FINGERPRINT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_tree_fingerprint.json")


def tree_fingerprint(rd, scene, builder):
    """({n_nodes, max_depth, n_leaf_refs}, {the four traversal counters}) of one build of `scene` on its fixed rays and pairs."""
    ref = _reference(scene)
    g = gpu_scene(rd, ref["sb"], builder)
    i = g.info()
    info = dict(n_nodes=int(i.n_nodes), max_depth=int(i.max_depth), n_leaf_refs=int(i.n_leaf_refs))
    _, c = g.trace_closest(ref["rays"], count=True)
    _, s = g.visibility(ref["a"], ref["b"], count=True)
    g.close()
    return info, dict(node_visits=int(c.node_visits), tri_tests=int(c.tri_tests), shadow_node_visits=int(s.shadow_node_visits),
                      shadow_tri_tests=int(s.shadow_tri_tests))


@functools.lru_cache(maxsize=None)
def _fingerprints():
    import json
    with open(FINGERPRINT_FILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("scene,builder", FINGERPRINT_CASES, ids=[f"{s}-{b}" for s, b in FINGERPRINT_CASES])
def test_device_built_tree_keeps_its_fingerprint(rd, scene, builder):
    """The trees of the device builder (rgk_build.hip), as far as the C ABI shows them: node count, depth and leaf references of
    rgk_scene_get_info, and the node visits and triangle tests that the scene's fixed rays and pairs cost -- a different tree,
    child box or 8-bit code changes what a ray visits.  The expected numbers (tests/golden/device_tree_fingerprint.json) were
    recorded on the MI355X from the commit BEFORE the builder's pieces moved into rgk_tree.h, three builds per case; a refactor
    of the builder must leave them as they are.  The device build numbers its nodes with atomics: a case whose counters were
    not the same in all three builds has no "counters" entry (the file lists those cases under "unstable") and is held to the
    three info numbers alone.  (Atomics, not a read of something unwritten: every scratch array of the build is written before
    it is read -- DESIGN.md 16, "Written before read" -- and with the builder's scratch filled with 0xFF bytes the same three
    builders give the info numbers and, for every ray, the answers they give on fresh memory: tests/test_gpu_memstate.py.)"""
    want = _fingerprints()[f"{scene}-{builder}"]
    info, counters = tree_fingerprint(rd, scene, builder)
    assert info == want["info"], (info, want["info"])
    if "counters" in want:
        assert counters == want["counters"], (counters, want["counters"])


# ----------------------------------------------------------------------- the feature pass: camera rays made on the device
def _camera_case(name, W, H):
    from rgk_amd.workloads import Workload
    if name == "cornell":
        sb = Workload("cornell-256", scale=1.0, spp=1).builder
        c = sb.extra["camera"]
        return sb, make_camera(c["pos"], c["lookat"], c["up"], fov=c["fov"], xres=W, yres=H)
    if name == "closed":     # from inside the mesh: every pixel sees a triangle, many pixel centres fall on shared edges
        return T.SCENES["closed"](), make_camera((0.1, 0.2, 0.3), (1.0, 0.3, -0.2), (0, 1, 0), fov=70, xres=W, yres=H)
    return T.SCENES["count65"](), make_camera((0.0, 0.0, 7.0), (0, 0, 0), (0, 1, 0), fov=75, xres=W, yres=H)   # (from among the triangles: 11 % of the pixels see one)


@pytest.mark.parametrize("name", ["closed", "count65", "cornell"])
@pytest.mark.parametrize("size", [(67, 45), (100, 70)])
def test_feature_pass_equals_the_exhaustive_search_on_every_pixel(rd, oracle, name, size):
    """rgk_render_aov with only tri and depth asked for, against the exhaustive reference on orc_camera_ray's pixel-centre rays,
    for EVERY pixel of the frame.  The pass makes its rays on the device (k_aov_raygen: camera_ray, the function k_trace_camera
    uses) and walks them with k_trace_closest; k_trace_camera, the beam walker and the entry-point lists are reached through
    rgk_render_round alone.  At Cornell 100 x 70 this includes the 14 pixels on the back wall's diagonal that
    test_features_equal_the_oracle_composition leaves out: the tie rule decides them."""
    W, H = size
    sb, cam = _camera_case(name, W, H)
    osc = oracle.OracleScene(sb.to_desc())
    rays = T.camera_rays(oracle, cam, W, H)
    ex = osc.trace_closest_exhaustive(rays)
    for builder in ("host-sah", "device"):
        g = gpu_scene(rd, sb, builder)
        assert_same_frame(g, osc)
        prm = make_params(W, H, 1, 1)
        tiles = rd.generate_task_list(W, H)
        depth = np.full((H, W), 7.5, np.float32)
        tri = np.full((H, W), 7, np.int32)
        capi.check(g.lib, g.lib.rgk_render_aov(g.h, C.byref(cam), C.byref(prm), tiles, len(tiles), None, None, depth.ctypes.data, tri.ctypes.data))
        want_z = np.where(ex["tri"] >= 0, ex["t"], np.float32(0)).astype(np.float32).reshape(H, W)
        bad = (tri != ex["tri"].reshape(H, W)) | (T.bits(depth) != T.bits(want_z))
        record_parity(f"gpu_exhaustive[aov {name} {W}x{H} {builder}]", rays=W * H, hits=int((ex["tri"] >= 0).sum()), differing=int(bad.sum()))
        assert not bad.any(), (name, size, builder, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        g.close()
    assert (ex["tri"] >= 0).mean() > (0.9 if name != "count65" else 0.08)


# ----------------------------------------------------------------------- rounds under every stack variant
ROUND_W, ROUND_H, ROUND_SPP, ROUND_DEPTH = 67, 45, 8, 5     # ragged in x and y; 8 spp: gshift = 3, the beam walker is taken when asked
ROUND_VARIANTS = {   # scene -> the variants held to the default ("host-sah": 256/16)
    "small": ("host-sah-stack256-lds32", "host-sah-stack32-lds32"),
    "deep": ("host-sah-stack256-lds16", "host-sah-stack256-lds32"),     # 68 stack entries: the two that overflow into global memory
}


def _round_scene(name):
    """(builder, camera): small_scene() of test_gpu_const_light.py, or trace_ref's `deep` scene lit by one point light."""
    import test_gpu_const_light as CL
    if name == "small":
        return CL.small_scene(), make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=ROUND_W, yres=ROUND_H, focus_plane=5.0)
    sb = T.SCENES["deep"]()
    sb.add_point_light((0.7, 1.2, 0.9), (1.0, 0.95, 0.8), 6.0, 0.0)
    sb.set_skybox_color((0.55, 0.7, 0.9), 0.8)
    # looking down the progression from beyond its coarse end: the levels line up behind each other, 40 % of the pixels see a triangle
    return sb, make_camera((1.3, 0.02, 0.05), (0, 0, 0), (0, 1, 0), fov=70, xres=ROUND_W, yres=ROUND_H)


def _round_params(reverse=0):
    return make_params(ROUND_W, ROUND_H, ROUND_SPP, ROUND_DEPTH, clamp=30.0, russian=0.7, bumpscale=2.0, reverse=reverse)


def _variant_scene(rd, scene, sb, builder):
    g = gpu_scene(rd, sb, builder)
    depth = g.info().max_depth
    if scene == "deep":
        assert depth >= 11, depth          # 3 pushes per level: more than 32 stack entries possible
    else:
        assert depth <= 7, depth           # shallow enough for the all-LDS 32/32 walker (see CASES above)
    return g


def _two_rounds(g, cam, prm, tiles, **tuning):
    """Two rounds of one frame in separate accumulators: the second runs on capped entry lists."""
    g.set_tuning(**tuning)
    out = [g.render_round(cam, prm, tiles) for _ in range(2)]
    g.close()
    return out


ROUND_CASES = [(scene, cl, beam, 0) for scene in ("small", "deep") for cl in (0, 1) for beam in (0, 2)] + [("small", 1, 1, 3)]


@functools.lru_cache(maxsize=None)
def _small_scene_split(oracle):
    """Once: the oracle's bidirectional round on the small scene, split into its terms, every ray answered by exhaustive search."""
    sb, cam = _round_scene("small")
    return oracle.OracleScene(sb.to_desc()).render_round_split(cam, _round_params(reverse=3), oracle.generate_task_list(ROUND_W, ROUND_H), exhaustive=True)


@pytest.mark.parametrize("scene,const_light,beam,reverse", ROUND_CASES, ids=[f"{s}-const_light{c}-beam{b}-reverse{r}" for s, c, b, r in ROUND_CASES])
def test_rounds_do_not_depend_on_the_stack_variant(rd, oracle, scene, const_light, beam, reverse):
    """The walkers that only rounds reach -- k_trace_camera, k_trace_camera_beam (beam = 2: in both rounds), k_trace_shadow_first,
    the two constant-light kernels and, with reverse = 3, k_trace_shadow_jobs and the splat mode of k_trace_shadow -- under the
    <STACK, LDSN> variants that the tests above reach through k_trace_closest and k_trace_shadow alone.  Two rounds of one frame
    per variant, the second on capped entry lists.  (32/32 has no overflow area and never takes the beam walker, rgk_plan.h
    rgk_beam_taken: its camera rays go through k_trace_camera under either switch value.)

    reverse = 0: accumulator, sample counts and the path / ray counters of both rounds are the default variant's, bit for bit.

    reverse = 3 (small scene, every variant, the default included): splat order is not repeatable, so two GPU runs are not
    compared bit for bit; each round is held per pixel to the oracle's terms (tests/bdpt_ref.py check_round, as
    test_gpu_bdpt.check_case does): no pixel outside the summation-order bound, the bit-exact classes exact, sample counts,
    paths and path_rays the oracle's, shadow_rays at most the oracle's, and all three counters equal between the variants.  The
    oracle's rays are answered by exhaustive search, the rule the walkers are pinned to: on this scene's bump-mapped surfaces the
    kd-tree oracle decides some in-surface connection rays inside its epsilon band
    (test_gpu_const_light.test_bidirectional_round_on_an_eligible_scene), which says nothing about a stack."""
    import bdpt_ref as B
    sb, cam = _round_scene(scene)
    prm, tiles = _round_params(reverse), rd.generate_task_list(ROUND_W, ROUND_H)
    runs = {}
    for builder in ("host-sah",) + ROUND_VARIANTS[scene]:
        g = _variant_scene(rd, scene, sb, builder)
        assert g.info().const_light == 1
        runs[builder] = _two_rounds(g, cam, prm, tiles, const_light=const_light, beam=beam)
    base = runs["host-sah"]
    assert base[0][2].path_rays > ROUND_W * ROUND_H * ROUND_SPP and base[0][2].shadow_rays > 1000 and float(base[0][0].max()) > 0.0
    tag = f"gpu_exhaustive[rounds {scene} const_light{const_light} beam{beam} reverse{reverse}"
    for builder, rounds in runs.items():
        for r, ((a0, c0, k0), (a1, c1, k1)) in enumerate(zip(base, rounds)):
            assert (k0.paths, k0.path_rays, k0.shadow_rays) == (k1.paths, k1.path_rays, k1.shadow_rays), (builder, r)
            if reverse:
                split = _small_scene_split(oracle)
                planes, s = B.check_split(a1, c1, split)
                record_parity(f"{tag} {builder} round {r}]", **B.record_fields(s), path_rays_delta=int(k1.path_rays) - int(split.counters.path_rays))
                assert split.n_splats > 0 and s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["exact_n0"] == s["exact_n1"] == 1.0, (builder, r, s)
                assert k1.path_rays == split.counters.path_rays and k1.paths == split.counters.paths and k1.shadow_rays <= split.counters.shadow_rays, (builder, r)
            elif builder != "host-sah":
                differ = int((a0.view(np.uint32) != a1.view(np.uint32)).any(axis=2).sum())
                record_parity(f"{tag} {builder} round {r}]", pixels=ROUND_W * ROUND_H, differing=differ)
                assert differ == 0 and np.array_equal(c0, c1), (builder, r, differ)
