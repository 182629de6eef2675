"""GPU suite (-m gpu): what include/rgk.h promises of the per-scene tuning switches, the round flags and the tree builders --
none of them changes a result.  Every variant renders in a fresh scene and is compared BIT FOR BIT (RGB sums, sample counts,
path and shadow ray counts) with the same frame rendered by a fresh scene at default switches and batch_paths = 0; that
baseline is compared once with the oracle, so the matrix is tied to the reference and not only to itself.

The batch sizes are picked from rgk_render_round's sizing loop so that the pass plans hit the edges: pixel ranges that need
several sample passes (an odd number of them too), pixel ranges that are no multiple of the 8-pixel entry group
(RGK_ENTRY_PIX), and several pixel ranges that each need several sample passes."""
import math
import os

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_params
from rgk_amd.scene import SceneBuilder

from conftest import make_rays, record_parity
from test_gpu_parity import check_closest, image_metrics, random_rays

pytestmark = pytest.mark.gpu

FLAG_COUNT, FLAG_TIME = 1, 2   # RGK_FLAG_COUNT_TRAVERSAL, RGK_FLAG_TIME_KERNELS


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def render_fresh(rd, wl, prm, tiles, rounds=1, **tuning):
    """[(accum, count, counters)] of `rounds` rounds of one frame in a fresh scene with the given switches."""
    g = rd.Scene(wl.builder.to_desc())
    if tuning:
        g.set_tuning(**tuning)
    out = [g.render_round(wl.camera, prm, tiles) for _ in range(rounds)]
    g.close()
    return out


def assert_same_bits(base, got, what):
    (a0, c0, k0), (a1, c1, k1) = base, got
    assert np.array_equal(c0, c1), (what, "sample counts")
    differ = int((a0.view(np.uint32) != a1.view(np.uint32)).any(axis=2).sum())
    assert differ == 0, (what, f"{differ} pixels differ", float(np.linalg.norm(a1 - a0) / np.linalg.norm(a0)))
    assert (k0.path_rays, k0.shadow_rays) == (k1.path_rays, k1.shadow_rays), (what, "ray counts")


def against_oracle(oracle, wl, prm, tiles, acc, cnt, n_tiles, name, rel_max=1e-3, within_min=0.999):
    """The first n_tiles tiles of a GPU round against the oracle's round of the same tiles (SURVEY 8(d)'s gate)."""
    sub = (capi.Tile * n_tiles)(*tiles[:n_tiles])
    o = oracle.OracleScene(wl.builder.to_desc())
    ao = np.zeros_like(acc); co = np.zeros_like(cnt)
    o.render_round(wl.camera, prm, sub, ao, co)
    m = co > 0
    assert m.sum() > 0 and np.array_equal(cnt[m], co[m])
    img, ref = (acc[m] / cnt[m][:, None])[None], (ao[m] / co[m][:, None])[None]
    rel, within = image_metrics(img, ref, name)
    assert rel <= rel_max and within >= within_min, (name, rel, within)


# ----------------------------------------------------------------------- pass plans
# Cornell 512 x 512 x 16 (P = 262 144 pixels).  Pass plans:
#   2 097 152: the whole list x 2 sample passes (8 spp each)
#   1 572 864: the whole list x 3 sample passes (6, 6, 4 spp): an odd count
#     524 288: the whole list x 8 sample passes (2 spp each)
#     200 006: 2 pixel ranges (the first no multiple of the 8-pixel entry group) x 16 single-sample passes
CORNELL_BATCHES = (2097152, 1572864, 524288, 200006)


def test_pass_plans_do_not_change_the_image_cornell(rd, oracle):
    from rgk_amd.workloads import Workload
    wl = Workload("cornell-1024", scale=0.5, spp=16)
    assert (wl.xres, wl.yres, wl.multisample, wl.reverse) == (512, 512, 16, 0) and wl.depth <= 12
    prm = wl.params()
    tiles = rd.generate_task_list(wl.xres, wl.yres)
    base = render_fresh(rd, wl, prm, tiles, rounds=2)
    assert (base[0][1] == 16).all()
    assert_same_bits(base[0], base[1], "baseline: second round of the frame")
    against_oracle(oracle, wl, prm, tiles, base[0][0], base[0][1], 64, "test_pass_plans_do_not_change_the_image_cornell:baseline-vs-oracle")
    variants = [dict(batch_paths=b) for b in CORNELL_BATCHES]
    variants += [dict(batch_paths=1572864, sample_group=grp) for grp in (0, 6)]   # k_resolve / k_resolve_tiled
    for tv in variants:
        for r, got in enumerate(render_fresh(rd, wl, prm, tiles, rounds=2, **tv)):
            assert_same_bits(base[r], got, (tv, "round", r))
    record_parity("test_pass_plans_do_not_change_the_image_cornell", variants=len(variants), size="512x512x16", bit_identical=1.0)


def test_pass_plans_do_not_change_the_image_sponza(rd, oracle):
    """Point light, all per-frame lists on (camera entry nodes, their caps from the frame's second round on, light-side entry
    nodes and their boxes): sample passes split or pixel ranges that straddle entry groups, and every camera
    walker (beam 0: per ray, 1: bundles while uncapped, 2: bundles against capped lists too)."""
    from rgk_amd.workloads import Workload
    wl = Workload("sponza-1080p", scale=0.5, spp=16)
    assert (wl.xres, wl.yres, wl.reverse) == (960, 540, 0) and wl.xres * wl.yres * wl.multisample >= 1 << 22
    prm = wl.params()
    tiles = rd.generate_task_list(wl.xres, wl.yres)
    base = render_fresh(rd, wl, prm, tiles, rounds=2)
    assert_same_bits(base[0], base[1], "baseline: second round of the frame")
    against_oracle(oracle, wl, prm, tiles, base[0][0], base[0][1], 64, "test_pass_plans_do_not_change_the_image_sponza:baseline-vs-oracle")
    n = 0
    # 2 097 152: the whole list x 4 sample passes of 4 spp; 200 006: 3 pixel ranges (200 006 pixels: no multiple of 8) x 16
    # single-sample passes
    for batch in (2097152, 200006):
        for beam in (0, 1, 2):
            tv = dict(batch_paths=batch, beam=beam, entry_points=1, entry_cap=1, light_entry=1)
            for r, got in enumerate(render_fresh(rd, wl, prm, tiles, rounds=2, **tv)):
                assert_same_bits(base[r], got, (tv, "round", r))
            n += 1
    record_parity("test_pass_plans_do_not_change_the_image_sponza", variants=n, size="960x540x16", bit_identical=1.0)


def test_deep_paths_small_batches(rd, oracle):
    """depth > 12: the round reads the next queue's length back every other bounce (`track`) to shorten the launches and stop
    early; with passes split over pixels and samples that path runs once per pass."""
    from rgk_amd.workloads import Workload
    wl = Workload("cornell-256", spp=32)
    prm = make_params(wl.xres, wl.yres, wl.multisample, 16, wl.clamp, wl.russian, wl.bumpscale)
    tiles = rd.generate_task_list(wl.xres, wl.yres)
    base = render_fresh(rd, wl, prm, tiles)[0]
    assert (base[1] == 32).all()
    against_oracle(oracle, wl, prm, tiles, base[0], base[1], 32, "test_deep_paths_small_batches:baseline-vs-oracle")
    # 50 000 paths: ranges of 50 000 pixels (no multiple of 8), 32 single-sample passes each; 300 000: 8 sample passes of 4
    for tv in (dict(batch_paths=50000), dict(batch_paths=300000)):
        assert_same_bits(base, render_fresh(rd, wl, prm, tiles, **tv)[0], tv)


# ----------------------------------------------------------------------- flags
@pytest.mark.parametrize("shape", ["cornell", "sponza"])
def test_counting_and_timing_flags_do_not_change_the_image(rd, oracle, shape):
    """RGK_FLAG_COUNT_TRAVERSAL (counting kernel variants, a read-back after every traversal launch) and RGK_FLAG_TIME_KERNELS
    (events around every launch) -- what bench.py --full and the profiling tools render with -- give the image of flags = 0."""
    from rgk_amd.workloads import Workload
    if shape == "cornell":
        wl, tuning, n_tiles = Workload("cornell-256", spp=16), {}, 64
    else:
        wl, tuning, n_tiles = Workload("sponza-1080p", scale=0.25, spp=16), dict(entry_points=1, entry_cap=1, light_entry=1), 32
    tiles = rd.generate_task_list(wl.xres, wl.yres)
    base = render_fresh(rd, wl, wl.params(), tiles, rounds=2, **tuning)
    against_oracle(oracle, wl, wl.params(), tiles, base[0][0], base[0][1], n_tiles, f"test_counting_and_timing_flags:{shape}:baseline-vs-oracle")
    for flags in (FLAG_COUNT, FLAG_TIME, FLAG_COUNT | FLAG_TIME):
        got = render_fresh(rd, wl, wl.params(flags=flags), tiles, rounds=2, **tuning)
        for r in range(2):
            assert_same_bits(base[r], got[r], (shape, flags, "round", r))
            k = got[r][2]
            if flags & FLAG_COUNT:
                assert k.node_visits > 0 and k.shadow_node_visits > 0, (shape, flags)
            if flags & FLAG_TIME:
                assert k.ms_trace > 0 and k.n_trace_launches > 0, (shape, flags)
        if flags == FLAG_COUNT:
            record_parity(f"test_counting_and_timing_flags:{shape}", node_visits_per_path=got[0][2].node_visits / got[0][2].paths,
                          shadow_node_visits_per_path=got[0][2].shadow_node_visits / got[0][2].paths)


# ----------------------------------------------------------------------- bidirectional
def test_bidirectional_small_batches(rd, oracle):
    """reverse = 2 with passes split over pixels and samples: splats are float atomics (any pixel, any order), so every plan is
    held per pixel to the oracle's terms (tests/bdpt_ref.py; extra_terms = multisample, as for every plan that may split the
    samples).  At 256 x 256 x 16 the kd-tree oracle itself differs from the GPU in two pixels WITHOUT reverse (epsilon-band ties:
    5 of 2.5 M path rays), so against it the project's gate of 99.9 % of the pixels holds (measured: 3 outside of 65 536), and
    against the oracle's round with every ray answered by exhaustive search -- the rule the traversal is pinned to -- no pixel is
    outside and path_rays is exact; counts and ray counts stay exact between the plans."""
    from rgk_amd.workloads import Workload
    import bdpt_ref as B
    wl = Workload("cornell-256", spp=16)
    prm = make_params(wl.xres, wl.yres, wl.multisample, 5, clamp=20.0, russian=0.7, reverse=2)
    tiles = rd.generate_task_list(wl.xres, wl.yres)
    a0, c0, k0 = render_fresh(rd, wl, prm, tiles)[0]
    o = oracle.OracleScene(wl.builder.to_desc())
    split = o.render_round_split(wl.camera, prm, oracle.generate_task_list(wl.xres, wl.yres))
    ao, co, ko = o.render_round(wl.camera, prm, oracle.generate_task_list(wl.xres, wl.yres))
    rel_o = float(np.linalg.norm(a0 - ao) / np.linalg.norm(ao))
    planes, s0 = B.check_split(a0, c0, split, extra_terms=wl.multisample)
    assert np.array_equal(c0, co) and s0["outside"] <= 1e-3 * s0["pixels"] and s0["bad_values"] == 0, s0
    assert abs(int(k0.path_rays) - int(ko.path_rays)) <= 1e-5 * ko.path_rays and k0.shadow_rays <= ko.shadow_rays, (k0.path_rays, ko.path_rays)
    exact = o.render_round_split(wl.camera, prm, oracle.generate_task_list(wl.xres, wl.yres), exhaustive=True)
    planes, sx = B.check_split(a0, c0, exact, extra_terms=wl.multisample)
    assert sx["outside"] == 0 and sx["exact_n0"] == 1.0 and sx["bad_values"] == 0, sx
    assert k0.path_rays == exact.counters.path_rays and k0.shadow_rays <= exact.counters.shadow_rays, (k0.path_rays, exact.counters.path_rays)
    worst, worst_ratio = 0.0, sx["worst_ratio"]
    for batch in (20000, 300000):    # 20 000: ranges of 20 000 pixels x 16 single-sample passes; 300 000: 4 sample passes of 4
        a1, c1, k1 = render_fresh(rd, wl, prm, tiles, batch_paths=batch)[0]
        assert np.array_equal(c0, c1) and (k0.path_rays, k0.shadow_rays) == (k1.path_rays, k1.shadow_rays), batch
        rel = float(np.linalg.norm(a1 - a0) / np.linalg.norm(a0))
        worst = max(worst, rel)
        planes, s1 = B.check_split(a1, c1, exact, extra_terms=wl.multisample)
        worst_ratio = max(worst_ratio, s1["worst_ratio"])
        assert s1["outside"] == 0 and s1["exact_n0"] == 1.0 and s1["bad_values"] == 0, (batch, s1)
    record_parity("test_bidirectional_small_batches", rel_l2_vs_oracle=rel_o, rel_l2_small_batches=worst, size="256x256x16 reverse=2",
                  outside_vs_kd_oracle=s0["outside"], **{k: v for k, v in B.record_fields(sx).items() if k != "worst_err_over_bound"},
                  worst_err_over_bound=worst_ratio)


# ----------------------------------------------------------------------- tree builders
def coincident_runs_scene(runs=(2, 300, 1000, 5000)):
    """A random triangle soup (an ordinary mesh) plus runs of k coincident copies of one non-degenerate triangle, each run in
    its own place: equal boxes in a row of the Morton order, the worst case of a clustering builder's tie-breaks."""
    rng = np.random.default_rng(51)
    n = 3000
    c = rng.uniform(-5, 5, (n, 1, 3))
    soup = (c + rng.normal(scale=0.4, size=(n, 3, 3))).astype(np.float32)
    tris = [soup]
    centres = []
    for i, k in enumerate(runs):
        ctr = np.array([-3.0 + 2.0 * i, 0.5 * (i % 2), 1.0 - i], np.float32)
        t = ctr + np.array([[-0.9, -0.6, 0.1], [0.8, -0.5, -0.2], [0.05, 0.9, 0.15]], np.float32)
        tris.append(np.repeat(t[None], k, axis=0))
        centres.append(t.mean(axis=0))
    tri = np.concatenate(tris)
    sb = SceneBuilder(); sb.register_material(sb.new_material("m", capi.BXDF_DIFFUSE))
    pos = tri.reshape(-1, 3)
    nrm = np.tile([0, 1, 0], (len(pos), 1)).astype(np.float32)
    sb.add_mesh(pos, nrm, np.zeros((len(pos), 2), np.float32), np.tile([1, 0, 0], (len(pos), 1)).astype(np.float32),
                np.arange(len(pos)).reshape(-1, 3), 0)
    return sb, len(tri), np.array(centres)


def test_device_builder_on_runs_of_identical_boxes(rd, oracle):
    """Coincident duplicate triangles (runs of 2 ... 5000 identical boxes) through the device builder with clustering (PLOC),
    without it (the Karras hierarchy, RGK_LBVH_PLOC=0) and through the host SAH builder: every build succeeds, hits are the
    oracle's (any of a run's copies is a tie inside the epsilon band), the device tree stays shallow, and the build is
    deterministic."""
    sb, n_tris, centres = coincident_runs_scene()

    def scene(flags, env=None):
        sb.build_flags = flags
        if env:
            os.environ.update(env)     # (read once, in rgk_scene_create)
        try:
            return rd.Scene(sb.to_desc())
        finally:
            for k in env or ():
                del os.environ[k]
    gd = scene(capi.BUILD_DEVICE)
    gd2 = scene(capi.BUILD_DEVICE)
    gk = scene(capi.BUILD_DEVICE, {"RGK_LBVH_PLOC": "0"})
    gh = scene(capi.BUILD_HOST_SAH)
    o = oracle.OracleScene(sb.to_desc())
    ih, idv, idk = gh.info(), gd.info(), gk.info()
    assert idv.n_leaf_refs == ih.n_leaf_refs == idk.n_leaf_refs and idv.epsilon == ih.epsilon
    rng = np.random.default_rng(52)
    lo, hi = np.array(list(ih.bbox_min)), np.array(list(ih.bbox_max))
    oo, dd = random_rays(rng, lo, hi, 150000)
    # ... and rays aimed at the runs' triangles from anywhere in the box
    src = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (50000, 3))).astype(np.float32)
    tgt = centres[rng.integers(0, len(centres), 50000)] + rng.normal(scale=0.1, size=(50000, 3))
    d2 = (tgt - src); d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    rays = np.concatenate([make_rays(oo, dd), make_rays(src, d2.astype(np.float32))])
    for g, tag in ((gd, "device"), (gk, "device-karras"), (gh, "host-sah")):
        check_closest(g, o, rays, ih.epsilon, max_unexplained=5e-5, name=f"test_device_builder_on_runs_of_identical_boxes:{tag}:vs-oracle")
    n_refs = ih.n_leaf_refs
    bound = 1.5 * math.log2(n_refs)     # measured 14 (Karras hierarchy: 11) at 9 307 references; a run that chains is hundreds deep
    record_parity("test_device_builder_on_runs_of_identical_boxes", refs=n_refs, device_depth=idv.max_depth, device_karras_depth=idk.max_depth,
                  host_depth=ih.max_depth, depth_bound=round(bound, 1))
    assert idv.max_depth <= bound and idk.max_depth <= bound, (idv.max_depth, idk.max_depth, bound)
    # deterministic: a second device build of the same input is the same tree
    i2 = gd2.info()
    assert (i2.n_nodes, i2.max_depth, i2.n_leaf_refs) == (idv.n_nodes, idv.max_depth, idv.n_leaf_refs)
    h1, _ = gd.trace_closest(rays)
    h2, _ = gd2.trace_closest(rays)
    assert np.array_equal(h1.view(np.uint8), h2.view(np.uint8))
    for g in (gd, gd2, gk, gh):
        g.close()
