"""GPU suite (-m gpu): bidirectional rounds (reverse > 0) pinned PER PIXEL to the oracle's round split into its terms.

rgk_bdpt.h, the BDPT branch of k_shade, k_connect, k_trace_shadow_jobs and the RGK_SHADOW_SPLAT mode of k_trace_shadow were held
to whole-image relative-L2 bars that let lost border splats, and on the material zoo ALL splats lost, pass
(tests/test_bdpt_cpu.py shows both).  Here every pixel of a small render is held to tests/bdpt_ref.py's check_round: pixels no
splat lands on equal the oracle's own-pixel sum bit for bit, pixels with one splat equal float32(main + splat) bit for bit, every
other pixel lies inside the summation-order bound gamma(n) (|main| + sum |splat|) -- the splats are float atomics, their order is
the only freedom.  Sample counts and path_rays are exactly the oracle's; shadow_rays may only be fewer (zero-radiance rays are
not traced).

All-diffuse Cornell scenes: ZERO pixels outside, and the same seeds at reverse = 0 are bit-identical to the oracle first, so a
failure points at the bidirectional code.  The material zoo (fast and generic BxDF routes side by side) is not bit-identical
even without reverse -- ties inside the traversal's epsilon band, 0.9999 of the pixels -- so there up to 0.1 % of the pixels
(SURVEY 8(d)'s gate) may fall outside; the number that did is recorded -- and against the oracle's round with every ray answered
by exhaustive search instead of the kd-tree (render_round_split(exhaustive=True)) none may.  Every case records its class shares, the worst
error / bound and the pixels outside (conftest.record_parity)."""
import ctypes as C

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_params

from conftest import record_parity
import bdpt_ref as B
from test_bdpt_cpu import (cornell_builder, cornell_camera, every_other_tile, generic_route_vertices, inside_camera, zoo_builder,
                           zoo_camera)

pytestmark = pytest.mark.gpu

ZOO_CAP = 1e-3     # 99.9 % of the pixels


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


class Pairs:
    """One GPU scene and one oracle scene per builder, shared by the cases that change no tuning switch."""

    def __init__(self, rd, oracle):
        self.rd, self.O, self.made = rd, oracle, {}

    def get(self, key):
        if key not in self.made:
            sb = {"cornell": cornell_builder, "point": lambda: cornell_builder("point", 0.0), "sphere": lambda: cornell_builder("point", 0.15),
                  "zoo": zoo_builder}[key]()
            desc = sb.to_desc()
            self.made[key] = (sb, self.rd.Scene(desc), self.O.OracleScene(desc))
        return self.made[key]


@pytest.fixture(scope="module")
def pairs(rd, oracle):
    return Pairs(rd, oracle)


def params(W, H, spp, depth=5, reverse=3, clamp=20.0, russian=0.7):
    return make_params(W, H, spp, depth, clamp=clamp, russian=russian, reverse=reverse)


def with_reverse(prm, reverse):
    p = capi.Params.from_buffer_copy(prm)
    p.reverse = reverse
    return p


def check_case(name, g, o, cam, prm, tiles_g, tiles_o, extra_terms=0, cap=0.0, unidirectional_first=True):
    """One bidirectional round on the GPU against the oracle's split round: the per-pixel check, the counters, the record.
    cap: the share of pixels that may fall outside (0 on the all-diffuse scenes).  Where cap > 0 the round is ALSO held to the
    oracle's round with every ray answered by exhaustive search (the rule the GPU's traversal is pinned to, without the
    kd-tree's own epsilon-band decisions): there no pixel may fall outside and path_rays is exact.
    Returns (gpu accum, split, summary)."""
    if unidirectional_first:   # the same seeds without the bidirectional code: the oracle's bits
        p0 = with_reverse(prm, 0)
        a0, c0, k0 = g.render_round(cam, p0, tiles_g)
        r0, rc0, rk0 = o.render_round(cam, p0, tiles_o)
        assert np.array_equal(c0, rc0) and np.array_equal(a0.view(np.uint32), r0.view(np.uint32)), (name, "reverse = 0 differs from the oracle")
        assert k0.path_rays == rk0.path_rays, (name, "reverse = 0", k0.path_rays, rk0.path_rays)
    ag, cg, kg = g.render_round(cam, prm, tiles_g)
    split = o.render_round_split(cam, prm, tiles_o)
    planes, s = B.check_split(ag, cg, split, extra_terms)
    ko = split.counters
    print(f"[{name}] {s}  path_rays {kg.path_rays} / {ko.path_rays}  shadow_rays {kg.shadow_rays} / {ko.shadow_rays}")
    record_parity(f"test_gpu_bdpt:{name}", **B.record_fields(s), path_rays_delta=int(kg.path_rays) - int(ko.path_rays),
                  shadow_rays_gpu_over_oracle=kg.shadow_rays / max(1, ko.shadow_rays))
    assert split.n_splats > 0, name
    assert s["counts_equal"], (name, "sample counts")
    assert s["bad_values"] == 0, (name, s)
    assert s["outside"] <= cap * s["pixels"], (name, s)
    if cap == 0.0:
        assert s["exact_n0"] == 1.0 and s["exact_n1"] == 1.0, (name, s)
        assert kg.path_rays == ko.path_rays, (name, kg.path_rays, ko.path_rays)
        assert kg.paths == ko.paths
    assert kg.shadow_rays <= ko.shadow_rays, (name, kg.shadow_rays, ko.shadow_rays)
    if cap > 0.0:
        ex = o.render_round_split(cam, prm, tiles_o, exhaustive=True)
        planes, sx = B.check_split(ag, cg, ex, extra_terms)
        record_parity(f"test_gpu_bdpt:{name}:exhaustive-rays", **B.record_fields(sx), path_rays_delta=int(kg.path_rays) - int(ex.counters.path_rays))
        assert sx["outside"] == 0 and sx["exact_n0"] == sx["exact_n1"] == 1.0 and sx["counts_equal"] and sx["bad_values"] == 0, (name, sx)
        assert kg.path_rays == ex.counters.path_rays and kg.shadow_rays <= ex.counters.shadow_rays, (name, kg.path_rays, ex.counters.path_rays)
    return ag, split, s


def cornell_case(name, rd, oracle, pairs, W=64, H=64, spp=4, key="cornell", cam=None, select=None, **kw):
    sb, g, o = pairs.get(key)
    prm = params(W, H, spp, **kw)
    tg, to = rd.generate_task_list(W, H), oracle.generate_task_list(W, H)
    if select:
        tg, to = select(tg), select(to)
    return check_case(name, g, o, cam or cornell_camera(W, H), prm, tg, to)


# ----------------------------------------------------------------------- all-diffuse Cornell: zero pixels outside
@pytest.mark.parametrize("reverse,depth", [(1, 5), (2, 5), (3, 5), (7, 5), (7, 8), (3, 1), (3, 2)])
def test_reverse_and_depth(rd, oracle, pairs, reverse, depth):
    """reverse 1 .. 7 (the largest the host accepts: light-vertex bit 6 beside the generic-route flag 0x80, connection ray 7 on
    mask bit 7); depth 1 and 2 under reverse 3: more light vertices than camera vertices."""
    cornell_case(f"reverse-{reverse}-depth-{depth}", rd, oracle, pairs, reverse=reverse, depth=depth)


def test_reverse_8_is_refused_and_leaves_the_accumulator_alone(rd, product_lib, pairs):
    sb, g, o = pairs.get("cornell")
    W = H = 64
    tiles = rd.generate_task_list(W, H)
    rng = np.random.default_rng(3)
    acc = rng.random((H, W, 3), dtype=np.float32); cnt = rng.integers(0, 9, (H, W)).astype(np.uint32)
    acc0, cnt0 = acc.copy(), cnt.copy()
    prm = params(W, H, 4, reverse=8)
    cam = cornell_camera(W, H)
    rc = product_lib.rgk_render_round(g.h, C.byref(cam), C.byref(prm), tiles, len(tiles), acc.ctypes.data, cnt.ctypes.data, None)
    assert rc == -5 and b"reverse 8 > 7 light sub-path vertices" in product_lib.rgk_last_error()       # RGK_ERR_UNSUPPORTED
    assert np.array_equal(acc.view(np.uint32), acc0.view(np.uint32)) and np.array_equal(cnt, cnt0)


@pytest.mark.parametrize("case", ["clamp-0.5", "russian--1", "russian-0.7-depth-8", "spp-1-reverse-1", "spp-1", "spp-4"])
def test_clamp_russian_and_sample_counts(rd, oracle, pairs, case):
    """clamp = 0.5: the per-vertex and per-path clamps bind on sums that include connections.  russian -1: no roulette."""
    kw = {"clamp-0.5": dict(clamp=0.5), "russian--1": dict(russian=-1.0), "russian-0.7-depth-8": dict(russian=0.7, depth=8, reverse=2),
          "spp-1-reverse-1": dict(spp=1, reverse=1), "spp-1": dict(spp=1), "spp-4": dict(spp=4)}[case]
    ag, split, s = cornell_case(case, rd, oracle, pairs, **kw)
    if case == "clamp-0.5":
        assert float(split.main.max()) <= 4 * 0.5 and (split.main == np.float32(2.0)).any()     # the path clamp binds (4 spp x 0.5)
    if case == "spp-1-reverse-1":
        assert s["share_n0"] + s["share_n1"] >= 0.8, s          # most of this frame is in the bit-exact classes


@pytest.mark.parametrize("group", [0, 3])
def test_sample_groups_at_16_spp(rd, oracle, group):
    """16 spp with 1 and with 8 samples of a pixel side by side in the slot order (k_resolve / k_resolve_tiled)."""
    sb = cornell_builder()
    desc = sb.to_desc()
    g, o = rd.Scene(desc).set_tuning(sample_group=group), oracle.OracleScene(desc)
    W = H = 64
    check_case(f"sample-group-{group}", g, o, cornell_camera(W, H), params(W, H, 16), rd.generate_task_list(W, H), oracle.generate_task_list(W, H))


def test_ragged_frame(rd, oracle, pairs):
    """67 x 45: partial tiles in x and y, no multiple of the 8 x 8 slot blocks."""
    cornell_case("ragged-67x45", rd, oracle, pairs, W=67, H=45)


def test_half_the_tiles(rd, oracle, pairs):
    """Every other entry of the task list -- what every rank of a sharded frame renders.  The WHOLE image is compared: on the
    pixels that were not rendered the count is 0 and the value is the sum of the splats that landed there."""
    ag, split, s = cornell_case("half-the-tiles", rd, oracle, pairs, select=every_other_tile)
    off = split.count == 0
    assert off.sum() == 64 * 64 // 2 and int(split.splat_n[off].sum()) >= 1000
    assert not split.main[off].any()
    lone = off & (split.splat_n == 1)
    assert lone.any() and np.array_equal(ag[lone], split.splat_sum[lone].astype(np.float32))
    assert not ag[off & (split.splat_n == 0)].any()


def test_pixel_list_with_tiles_of_width_1_and_5(rd, oracle, pairs):
    W, H = 36, 20
    spans = []
    x = 0
    while x < W:
        for w in (1, 5):
            spans.append((x, x + w)); x += w
    rows = ((0, 13), (13, 20))
    tiles = (capi.Tile * (len(spans) * len(rows)))()
    for i, ((y0, y1), (x0, x1)) in enumerate((r, s) for r in rows for s in spans):
        tiles[i].x0, tiles[i].x1, tiles[i].y0, tiles[i].y1, tiles[i].seed = x0, x1, y0, y1, 42 + i
    assert x == W and sum((t.x1 - t.x0) * (t.y1 - t.y0) for t in tiles) == W * H
    sb, g, o = pairs.get("cornell")
    check_case("tiles-of-width-1-and-5", g, o, cornell_camera(W, H), params(W, H, 4), tiles, tiles)


def test_point_light_under_both_const_light_switches(rd, oracle):
    """One point light of size 0 and nothing else that emits: the scene the constant-light route is eligible for.  A
    bidirectional round stays on the per-path route under either switch value."""
    sb = cornell_builder("point", 0.0)
    desc = sb.to_desc()
    o = oracle.OracleScene(desc)
    W = H = 64
    out = []
    for switch in (0, 1):
        g = rd.Scene(desc).set_tuning(const_light=switch)
        assert g.info().const_light == 1
        ag, split, s = check_case(f"point-light-const-light-{switch}", g, o, cornell_camera(W, H), params(W, H, 4), rd.generate_task_list(W, H),
                                  oracle.generate_task_list(W, H))
        out.append(ag)
    few = split.splat_n <= 1
    assert few.any() and np.array_equal(out[0][few].view(np.uint32), out[1][few].view(np.uint32))


def test_sphere_light(rd, oracle, pairs):
    """The same light with size > 0: its surface is sampled, the sampled direction is its normal."""
    cornell_case("sphere-light", rd, oracle, pairs, key="sphere")
    assert pairs.get("sphere")[1].info().const_light == 0


def test_emissive_quad_starts_the_sub_path(rd, oracle, pairs):
    sb, g, o = pairs.get("cornell")
    assert not sb.pointlights and len(sb.areal) > 0
    cornell_case("emissive-quad-spp-8", rd, oracle, pairs, spp=8, reverse=2)


@pytest.mark.parametrize("which", ["square", "64x24"])
def test_camera_inside_the_box(rd, oracle, pairs, which):
    """Most light vertices project outside the frame or lie behind the camera (coords_from_direction refuses them); every one of
    the four frame edges receives splats in its outermost row or column."""
    cam, W, H = inside_camera(which)
    ag, split, s = cornell_case(f"camera-inside-{which}", rd, oracle, pairs, W=W, H=H, cam=cam)
    n = split.splat_n
    assert n[0].sum() > 0 and n[-1].sum() > 0 and n[:, 0].sum() > 0 and n[:, -1].sum() > 0
    assert split.n_splats < 0.5 * int(split.lv_kind.sum())          # most light vertices make no splat


def test_second_round_onto_the_first(rd, oracle, pairs):
    """Two rounds of a frame (the second with seedcount_base advanced) into one accumulator: the terms of both rounds in any
    order -- the second round's own-pixel part is one more order-free term of every pixel."""
    sb, g, o = pairs.get("cornell")
    W = H = 64
    cam, prm = cornell_camera(W, H), params(W, H, 4)
    n_tiles = len(rd.generate_task_list(W, H))
    acc = np.zeros((H, W, 3), np.float32); cnt = np.zeros((H, W), np.uint32)
    splits, rays_g, rays_o = [], 0, 0
    for r in range(2):
        _, _, k = g.render_round(cam, prm, rd.generate_task_list(W, H, seedcount_base=r * n_tiles), acc, cnt)
        splits.append(o.render_round_split(cam, prm, oracle.generate_task_list(W, H, seedcount_base=r * n_tiles)))
        rays_g += k.path_rays; rays_o += splits[-1].counters.path_rays
    a, b = splits
    assert not np.array_equal(a.main, b.main)
    main, ssum, sabs, sn = a.main, a.splat_sum + b.splat_sum + b.main.astype(np.float64), a.splat_abs + b.splat_abs + np.abs(b.main.astype(np.float64)), a.splat_n + b.splat_n + 1
    planes, s = B.check_round(acc, cnt, main, ssum, sabs, sn, a.count + b.count)
    print(f"[two-rounds] {s}")
    record_parity("test_gpu_bdpt:two-rounds", **B.record_fields(s), path_rays_delta=int(rays_g) - int(rays_o))
    assert s["counts_equal"] and s["outside"] == 0 and s["bad_values"] == 0 and s["exact_n1"] == 1.0 and s["share_n1"] > 0, s
    assert rays_g == rays_o


@pytest.mark.parametrize("batch", [0, 20000, 3000])
def test_pass_plans_at_16_spp(rd, oracle, batch):
    """64 x 64 x 16 in one pass, in 4 sample passes of 4 (batch_paths 20 000) and in 2 pixel ranges x 16 single-sample passes
    (3000); extra_terms = multisample for all three."""
    sb = cornell_builder()
    desc = sb.to_desc()
    g, o = rd.Scene(desc), oracle.OracleScene(desc)
    if batch:
        g.set_tuning(batch_paths=batch)
    W = H = 64
    check_case(f"batch-paths-{batch}", g, o, cornell_camera(W, H), params(W, H, 16, reverse=2), rd.generate_task_list(W, H),
               oracle.generate_task_list(W, H), extra_terms=16)


# ----------------------------------------------------------------------- material zoo: both BxDF routes, thin lens
@pytest.mark.parametrize("W,H,reverse", [(64, 48, 2), (67, 45, 7)])
def test_material_zoo_with_the_lens(rd, oracle, pairs, W, H, reverse):
    """Mirror, dielectric, transparent, mix and LTC materials on both sub-paths: lvmask bit 7 set on some slots and clear on
    others, the camera position per sample.  Up to 0.1 % of the pixels may fall outside (epsilon-band ties, as without
    reverse); the oracle's own image stays at 0 (tests/test_bdpt_cpu.py)."""
    sb, g, o = pairs.get("zoo")
    prm = params(W, H, 4, depth=6, reverse=reverse, clamp=30.0)
    ag, split, s = check_case(f"zoo-{W}x{H}-reverse-{reverse}", g, o, zoo_camera(W, H), prm, rd.generate_task_list(W, H), oracle.generate_task_list(W, H),
                              cap=ZOO_CAP, unidirectional_first=False)
    assert generic_route_vertices(split.lv_kind) > 0 and int(split.lv_kind.sum()) > generic_route_vertices(split.lv_kind)
    assert split.lv_none > 0                                         # slots without any light vertex
