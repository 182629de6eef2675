"""CPU suite: the tests of the bidirectional test (tests/bdpt_ref.py, OracleScene.render_round_split).

The oracle's round split into its terms must recombine to orc_render_round's image bit for bit; check_round must accept the
oracle's own image and every re-ordering of its float32 sum; and it must reject what the whole-image relative-L2 bars it
replaces let through: lost border splats, all splats lost, splats on the wrong pixel, lost connections, ONE lost splat, one
splat wrong in its 10th mantissa bit.  The scenes and cases here are the ones tests/test_gpu_bdpt.py renders on the GPU."""
import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params

import bdpt_ref as B

OLD_BAR_CORNELL, OLD_BAR_ZOO = 2e-3, 3e-2   # the whole-image relative-L2 bars test_bidirectional_reverse_parity had


# ----------------------------------------------------------------------- scenes (shared with tests/test_gpu_bdpt.py)
def cornell_builder(light="quad", size=0.0):
    """The all-diffuse Cornell box.  light = "quad": as shipped, the emissive quad under the ceiling (an areal light starts the
    light sub-path); "point": the quad switched off and one point light of the given size in its place (size 0: a point, the
    constant-light route's eligible scene; size > 0: a sphere that is sampled)."""
    from rgk_amd.workloads import Workload
    sb = Workload("cornell-256", scale=0.25).builder
    assert all(m["kind"] == capi.BXDF_DIFFUSE for m in sb.materials) and len(sb.areal) > 0 and not sb.pointlights
    if light == "point":
        for m in sb.materials:
            m["emission"] = (0.0, 0.0, 0.0)
        sb.areal = []
        sb.add_point_light((0.1, 1.7, -0.1), (1.0, 0.9, 0.7), 3.0, size)
    return sb


def cornell_camera(W, H):
    return make_camera((0.0, 1.0, 6.8), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), fov=19.5, xres=W, yres=H)


def inside_camera(which):
    """Cameras INSIDE the box (x in [-1, 1], y in [0, 2], z in [-1, 1]) looking at a wall: most light vertices project outside
    the frame or lie behind the camera, and splats land on all four frame edges.  (camera, W, H)"""
    if which == "square":
        return make_camera((0.0, 1.0, 0.5), (0.99, 1.0, 0.3), (0, 1, 0), fov=70, xres=64, yres=64), 64, 64
    return make_camera((0.2, 1.2, 0.3), (-0.99, 0.9, -0.4), (0, 1, 0), fov=80, xres=64, yres=24), 64, 24


def zoo_builder():
    from test_gpu_parity import material_zoo    # mirror, dielectric, transparent, mix and LTC materials, an emissive quad
    return material_zoo()


def zoo_camera(W, H):
    return make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=W, yres=H, focus_plane=5.0, lens_size=0.05)


def every_other_tile(tiles):
    sub = [tiles[i] for i in range(0, len(tiles), 2)]
    return (capi.Tile * len(sub))(*sub)


def generic_route_vertices(lv_kind):
    """How many light sub-path vertices lie on a material the kernels send down the generic BxDF route (mat_is_fast is false:
    mirror, dielectric, transparent, mix)."""
    return int(sum(lv_kind[k] for k in (capi.BXDF_MIRROR, capi.BXDF_DIELECTRIC, capi.BXDF_TRANSPARENT, capi.BXDF_MIX)))


# name: (scene, W, H, spp, depth, reverse, clamp, russian, tiles)
CASES = {
    "cornell-r1": ("cornell", 64, 64, 4, 5, 1, 20.0, 0.7, "all"),
    "cornell-r2": ("cornell", 64, 64, 4, 5, 2, 20.0, 0.7, "all"),
    "cornell-r3": ("cornell", 64, 64, 4, 5, 3, 20.0, 0.7, "all"),
    "cornell-r7": ("cornell", 64, 64, 4, 5, 7, 20.0, 0.7, "all"),
    "zoo-r2": ("zoo", 64, 48, 4, 6, 2, 30.0, 0.7, "all"),
    "zoo-r7": ("zoo", 67, 45, 4, 6, 7, 30.0, 0.7, "all"),
    "clamp-0.5": ("cornell", 64, 64, 4, 5, 3, 0.5, 0.7, "all"),
    "depth-2": ("cornell", 64, 64, 4, 2, 3, 20.0, 0.7, "all"),
    "half-tiles": ("cornell", 64, 64, 4, 5, 3, 20.0, 0.7, "half"),
}


class Rounds:
    """The oracle's rounds of CASES, made once and shared (never modified) by the tests of this module."""

    def __init__(self, oracle):
        self.O, self.scenes, self.done = oracle, {}, {}

    def scene(self, key):
        if key not in self.scenes:
            sb = cornell_builder() if key == "cornell" else zoo_builder()
            self.scenes[key] = self.O.OracleScene(sb.to_desc())
        return self.scenes[key]

    def get(self, name, reverse=None):
        scene, W, H, spp, depth, R, clamp, russian, which = CASES[name]
        R = R if reverse is None else reverse
        if (name, R) not in self.done:
            cam = cornell_camera(W, H) if scene == "cornell" else zoo_camera(W, H)
            prm = make_params(W, H, spp, depth, clamp=clamp, russian=russian, reverse=R)
            tiles = self.O.generate_task_list(W, H)
            if which == "half":
                tiles = every_other_tile(tiles)
            o = self.scene(scene)
            split = o.render_round_split(cam, prm, tiles, want_list=True)
            img, cnt, k = o.render_round(cam, prm, tiles)
            for a in (img, cnt, split.main, split.splat_sum, split.splat_abs, split.splat_n, split.count, split.splats):
                a.setflags(write=False)
            self.done[(name, R)] = (split, tiles, img, cnt, k)
        return self.done[(name, R)]


@pytest.fixture(scope="module")
def rounds(oracle):
    return Rounds(oracle)


def rejected(img, cnt, split):
    planes, s = B.check_split(img, cnt, split)
    return s["outside"], planes, s


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def image_of(split, tiles, main=None, splats=None):
    """The float32 image orc_render_round would form of these (possibly perturbed) terms."""
    class Terms:
        pass
    t = Terms()
    t.main, t.splats = split.main if main is None else main, split.splats if splats is None else splats
    return B.resum_in_round_order(t, tiles)


# ----------------------------------------------------------------------- the split is the round
@pytest.mark.parametrize("name", sorted(CASES))
def test_terms_recombine_to_the_round_bit_for_bit(rounds, name):
    split, tiles, img, cnt, k = rounds.get(name)
    W, H, R = CASES[name][1], CASES[name][2], CASES[name][5]
    assert split.n_splats == len(split.splats) > 0 and int(split.splat_n.sum()) == split.n_splats
    assert np.array_equal(split.count, cnt)
    assert (k.path_rays, k.shadow_rays, k.paths) == (split.counters.path_rays, split.counters.shadow_rays, split.counters.paths)
    assert np.array_equal(B.resum_in_round_order(split, tiles).view(np.uint32), img.view(np.uint32))
    s, a, n = B.planes_from_list(split.splats, (H, W))
    assert np.array_equal(n, split.splat_n) and np.array_equal(s, split.splat_sum) and np.array_equal(a, split.splat_abs)
    assert int(split.lv_kind.sum()) > 0 and int(split.lv_kind.sum()) <= R * int(split.counters.paths)
    planes, summ = B.check_split(img, cnt, split)
    assert summ["outside"] == 0 and summ["counts_equal"] and summ["bad_values"] == 0, summ
    assert summ["exact_n0"] == summ["exact_n1"] == 1.0 and summ["worst_ratio"] <= 1.0, summ
    assert summ["share_n0"] > 0 and summ["share_n1"] > 0 and summ["share_bound"] > 0, summ      # every class is exercised
    if name == "half-tiles":
        off = split.count == 0
        assert off.sum() == W * H // 2 and int(split.splat_n[off].sum()) >= 1000
        assert not split.main[off].any()
    if name.startswith("zoo"):
        assert generic_route_vertices(split.lv_kind) > 0 and split.lv_none > 0      # both BxDF routes, and slots without a light vertex


def test_a_round_without_reverse_has_no_splats(rounds):
    split, tiles, img, cnt, k = rounds.get("cornell-r3", reverse=0)
    assert split.n_splats == 0 and not split.splat_n.any() and int(split.lv_kind.sum()) == 0
    assert np.array_equal(split.main.view(np.uint32), img.view(np.uint32))
    assert B.check_split(img, cnt, split)[1]["share_n0"] == 1.0


def test_exhaustive_rays_give_the_same_round_where_no_ray_meets_the_epsilon_band(rounds, oracle):
    """render_round_split(exhaustive=True) answers every ray by testing every triangle under the walkers' stated rule.  On the
    64 x 64 Cornell box that is the kd-tree's round bit for bit; on a bump-mapped floor, where connections run IN the surface
    they join and still carry radiance, a few rays are decided inside the kd-tree's epsilon band and a few pixels differ."""
    split, tiles, img, cnt, k = rounds.get("cornell-r3")
    scene, W, H, spp, depth, R, clamp, russian, which = CASES["cornell-r3"]
    ex = rounds.scene("cornell").render_round_split(cornell_camera(W, H), make_params(W, H, spp, depth, clamp=clamp, russian=russian, reverse=R),
                                                    tiles, want_list=True, exhaustive=True)
    assert np.array_equal(ex.main.view(np.uint32), split.main.view(np.uint32)) and np.array_equal(ex.splats, split.splats)
    assert (ex.counters.path_rays, ex.counters.shadow_rays) == (k.path_rays, k.shadow_rays)
    import test_gpu_const_light as CL
    sb = CL.small_scene()
    o = oracle.OracleScene(sb.to_desc())
    prm, t2 = CL.params(4, reverse=2), oracle.generate_task_list(CL.W, CL.H)
    kd, ex = o.render_round_split(CL.camera(), prm, t2), o.render_round_split(CL.camera(), prm, t2, exhaustive=True)
    differ = int((kd.main != ex.main).any(axis=2).sum()) + int((kd.splat_n != ex.splat_n).sum())
    assert 0 < differ <= 0.05 * CL.W * CL.H and kd.counters.path_rays == ex.counters.path_rays
    assert B.check_split(ex.main + ex.splat_sum.astype(np.float32), ex.count, kd)[1]["outside"] > 0


@pytest.mark.parametrize("name", ["cornell-r3", "zoo-r7", "half-tiles"])
def test_any_summation_order_is_inside_the_bound(rounds, name):
    split, tiles, img, cnt, k = rounds.get(name)
    rng = np.random.default_rng(11)
    differ, worst = 0, 0.0
    for _ in range(20):
        re = B.resum_in_random_order(split, rng)
        planes, summ = B.check_split(re, cnt, split)
        assert summ["outside"] == 0, summ
        differ += int((re.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())
        worst = max(worst, summ["worst_ratio"])
    assert differ > 0 and 0.0 < worst <= 1.0, (differ, worst)          # the orders DO change bits, inside the bound


def test_check_round_extra_terms_and_counts(rounds):
    split, tiles, img, cnt, k = rounds.get("cornell-r3")
    s0 = B.check_split(img, cnt, split)[1]
    s16 = B.check_split(img, cnt, split, extra_terms=16)[1]
    assert s16["share_n1"] == 0.0 and s16["share_n0"] == s0["share_n0"] and s16["outside"] == 0 and s16["worst_ratio"] < s0["worst_ratio"]
    assert not B.check_split(img, cnt + 1, split)[1]["counts_equal"]
    bad = img.copy(); bad[3, 5, 1] = np.nan; bad[7, 9, 2] = -1.0
    planes, s = B.check_split(bad, cnt, split)
    assert s["bad_values"] == 2 and not planes["ok"][3, 5] and not planes["ok"][7, 9] and s["outside"] == 2
    # a second round: its own-pixel part is one more order-free term; two rounds without splats have ONE possible sum
    m, ss, sa, sn = B.add_term(split, split.main)
    two = np.where((split.splat_n == 0)[..., None], split.main + split.main, 0).astype(np.float32)
    planes, s = B.check_round(two, cnt, m, ss, sa, sn, cnt)
    assert planes["ok"][split.splat_n == 0].all() and (planes["cls"][split.splat_n == 0] == 1).all()


# ----------------------------------------------------------------------- sensitivity: what the old bars let through
@pytest.mark.parametrize("name", ["cornell-r2", "cornell-r3", "cornell-r7"])
def test_lost_border_splats_pass_the_old_bar_and_are_rejected(rounds, name):
    split, tiles, img, cnt, k = rounds.get(name)
    H, W = split.splat_n.shape
    sp = split.splats
    ring = (sp["x"] == 0) | (sp["x"] == W - 1) | (sp["y"] == 0) | (sp["y"] == H - 1)
    assert ring.sum() > 0
    bad = image_of(split, tiles, splats=sp[~ring])
    assert rel_l2(bad, img) <= OLD_BAR_CORNELL                         # shipped under the old bar ...
    n_out, planes, s = rejected(bad, cnt, split)
    hit = np.zeros((H, W), bool); hit[sp["y"][ring], sp["x"][ring]] = True
    assert n_out > 0 and planes["ok"][~hit].all()
    assert (~planes["ok"])[hit].mean() >= 0.99, s                      # ... and nearly every ring pixel that lost one is now outside


@pytest.mark.parametrize("name", ["zoo-r2", "zoo-r7"])
def test_all_splats_lost_on_the_zoo_pass_the_old_bar_and_are_rejected(rounds, name):
    split, tiles, img, cnt, k = rounds.get(name)
    bad = image_of(split, tiles, splats=split.splats[:0])
    assert rel_l2(bad, img) <= OLD_BAR_ZOO
    n_out, planes, s = rejected(bad, cnt, split)
    got = split.splat_abs.sum(axis=2) > 0
    assert n_out > 0 and (~planes["ok"])[got].mean() >= 0.99, s


@pytest.mark.parametrize("name", ["cornell-r3", "zoo-r7"])
def test_splats_on_the_wrong_pixel_are_rejected(rounds, name):
    split, tiles, img, cnt, k = rounds.get(name)
    H, W = split.splat_n.shape
    sp = split.splats
    shifted = sp.copy(); shifted["x"] += 1
    shifted = shifted[shifted["x"] < W]
    flipped = sp.copy(); flipped["y"] = H - 1 - flipped["y"]
    for what, lst in (("x + 1", shifted), ("y flipped", flipped)):
        n_out, planes, s = rejected(image_of(split, tiles, splats=lst), cnt, split)
        assert n_out >= 0.5 * (split.splat_n > 0).sum(), (what, s)


@pytest.mark.parametrize("name", ["cornell-r3", "cornell-r7", "zoo-r7"])
def test_lost_connections_are_rejected(rounds, name):
    """main of reverse R replaced by main of reverse 1: the connections through light vertices >= 2 are lost (the camera path
    and light vertex 1 are the same: the sub-paths' sampler dimensions are pinned)."""
    split, tiles, img, cnt, k = rounds.get(name)
    one = rounds.get(name, reverse=1)[0]
    assert not np.array_equal(one.main, split.main)
    n_out, planes, s = rejected(image_of(split, tiles, main=one.main), cnt, split)
    changed = (one.main != split.main).any(axis=2)
    assert n_out > 0 and (~planes["ok"])[changed].mean() >= 0.99, s


@pytest.mark.parametrize("name", ["cornell-r1", "cornell-r3", "cornell-r7", "zoo-r2", "half-tiles"])
def test_one_splat_lost_or_off_by_2_to_the_minus_10_is_rejected(rounds, name):
    """ONE splat of the frame's median size dropped: its pixel is outside, no other is.  One splat scaled by 1 + 2^-10: the
    bound grows with the pixel's splat count, so the error of one splat shows while it is more than gamma(n) * 2^10 (n * 6e-5)
    of the pixel's magnitude; the median-sized one of those splats is scaled."""
    split, tiles, img, cnt, k = rounds.get(name)
    sp = split.splats
    size = sp["rgb"].sum(axis=1)
    y, x = sp["y"], sp["x"]
    bound = B.gamma(split.splat_n.astype(np.float64))[..., None] * (np.abs(split.main.astype(np.float64)) + split.splat_abs)
    shows = (sp["rgb"].astype(np.float64) * 2.0 ** -10 > 2.0 * bound[y, x]).any(axis=1) | (split.splat_n[y, x] == 1)
    assert shows.any()                  # (a third of the splats at reverse 7, where a pixel collects 11 on average; most at reverse 1)
    order = np.argsort(size)
    j_drop = int(order[len(order) // 2])
    cand = order[shows[order]]
    j_scale = int(cand[len(cand) // 2])
    scaled = sp.copy(); scaled["rgb"][j_scale] *= np.float32(1.0 + 2.0 ** -10)
    for what, j, lst in (("dropped", j_drop, np.delete(sp, j_drop)), ("scaled", j_scale, scaled)):
        n_out, planes, s = rejected(image_of(split, tiles, splats=lst), cnt, split)
        assert n_out == 1 and not planes["ok"][y[j], x[j]], (what, s, int(split.splat_n[y[j], x[j]]), float(shows.mean()))
