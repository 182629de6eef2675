"""GPU suite (-m gpu): per-sample demodulated accumulation -- rgk_render_round_demod_device, rgk_remodulate_device, the driver's
track_demod route and --demod -- held to the plain round entry and to the numpy restatement (tests/demod_ref.py).  Every comparison
is np.array_equal on the arrays (on their uint32 words where a NaN could hide), no tolerance, no pixel left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi

import demod_cases as DC
import demod_ref as D
import memstate_ref as M
import post_ref as PR
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED = -1, -5
FLOOR = DC.FLOOR


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def differing(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((M.bits(a) != M.bits(b)).sum())


_RUNS = {}


def run_of(rd, name):
    """A case of demod_cases, run once in this process on fresh memory and never changed afterwards (the memstate test's baseline)."""
    if name not in _RUNS:
        assert "RGK_POISON" not in os.environ
        res = DC.run_all(rd, [name])[name]
        for a in res.values():
            a.setflags(write=False)
        _RUNS[name] = res
    return _RUNS[name]


# ----------------------------------------------------------------------- 1. the main accumulator is unchanged
GROUPS = sorted({n.rsplit(" ", 1)[0].rsplit("x", 1)[0] for n in DC.ROUND_CASES})  # "<scene> <w>x<h>"


@pytest.mark.parametrize("group", GROUPS)
def test_accumulator_count_and_counters_are_the_plain_entrys(rd, group):
    """cornell-box-spheres and rubiks-bump at 24 x 24 and 37 x 19, 1 / 4 / 8 / 16 spp; sample_group 0 and 3, beam 0 and 1, a lens, and
    a batch of two samples per pass (spp / 2 sample passes, at sample_group 0 too).  The smallest batch a scene takes is 1024 paths,
    above both frames' pixel counts, so the case with two pixel ranges (x one sample pass per sample) runs at 41 x 29.  accum, count
    and the counters of rgk_render_round_demod_device equal rgk_render_round_device's on a fresh scene; the pass split is the one
    the case names, read from rgk_scene_get_progress' stage count; D and A are finite and A is at least half of count x floor (a sanity bound, not the check)."""
    names = [n for n in DC.ROUND_CASES if n.startswith(group + "x")]
    assert len(names) >= 2
    bad = []
    for name in names:
        case, r = DC.ROUND_CASES[name], run_of(rd, name)
        d = differing(r["plain.accum"], r["demod.accum"]) + int((r["plain.count"] != r["demod.count"]).sum()) + int((r["plain.counters"] != r["demod.counters"]).sum())
        passes = (int(r["plain.passes"][0]), int(r["demod.passes"][0]))
        sane = (np.isfinite(r["demod.D"]).all() and np.isfinite(r["demod.A"]).all() and (r["demod.count"] == case.spp).all() and
                (r["demod.A"] >= F(0.5) * F(case.spp) * F(FLOOR)).all() and float(r["demod.accum"].max()) > 0 and int(r["demod.counters"][1]) > case.size[0] * case.size[1] * case.spp)
        if d or passes != (case.passes, case.passes) or not sane:
            bad.append((name, d, passes, case.passes, bool(sane)))
    record_parity(f"gpu_demod.accumulator[{group}]", cases=len(names), bad=len(bad))
    assert not bad, bad


# ----------------------------------------------------------------------- 2. / 3. A and D against the restatement
_REF = {}


def oracle_scene(oracle, scene):
    if scene not in _REF:  # (a builder of its own: the descriptor points into the builder's arrays, which the next to_desc() replaces)
        from rgk_amd.workloads import SceneFixture
        sb = SceneFixture(os.path.join(ROOT, "tests", "golden", DC.FIXTURES[scene])).builder
        desc = sb.to_desc()
        _REF[scene] = (desc, oracle.OracleScene(desc), sb)
    return _REF[scene][:2]


@pytest.mark.parametrize("name", list(DC.SUM_CASES))
def test_divisor_sum_equals_the_restatement_on_every_pixel(rd, oracle, name):
    """One round at 8 spp, pinhole and lens: A == the float32 sum in sample order of div_s from demod_ref.sample_divisors (pixel
    seeds, sampler, camera rays, exhaustive-rule first hits, texture fetches: each pinned bit for bit by earlier tests).  The main
    accumulator of that round is the plain entry's (test 1)."""
    scene, (w, h), lens = DC.SUM_CASES[name]
    r = run_of(rd, name)
    desc, osc = oracle_scene(oracle, scene)
    div, covered = D.sample_divisors(oracle, osc, desc, DC.camera_of(scene, w, h, lens), oracle.generate_task_list(w, h), w, h, DC.SUM_SPP, FLOOR)
    want = D.divisor_sum(div, covered)
    d = differing(r["spp8.A"], want)
    textured = float((np.abs(want - F(DC.SUM_SPP)) > 0).any(axis=-1).mean())
    mixed = float(((div != div[:, :, :1]).any(axis=(2, 3))).mean())
    print(f"A [{name}]: {d} of {want.size} words differ; pixels with a divisor other than 1: {textured:.3f}; pixels whose samples disagree: {mixed:.3f}")
    record_parity(f"gpu_demod.A[{name}]", words=int(want.size), differing=d, share_not_one=textured, share_mixed=mixed)
    assert covered.all() and textured > 0.05 and mixed > 0.01, "the case must see surfaces, and footprints that straddle two albedos"
    assert d == 0


@pytest.mark.parametrize("name", [n for n in DC.ROUND_CASES if n.endswith("pixel-ranges")])
def test_divisor_sum_across_pixel_ranges_equals_the_restatement(rd, oracle, name):
    """The 41 x 29 cases of test 1 (two pixel ranges x one sample pass per sample, 4 and 8 spp): A == the restatement's sum on every
    pixel, those of the second range (j0 = 1024) included, so pixels, seeds and carried sums are indexed by j0 + j."""
    case, r = DC.ROUND_CASES[name], run_of(rd, name)
    (w, h), (desc, osc) = case.size, oracle_scene(oracle, case.scene)
    div, covered = D.sample_divisors(oracle, osc, desc, DC.camera_of(case.scene, w, h), oracle.generate_task_list(w, h), w, h, case.spp, FLOOR)
    want = D.divisor_sum(div, covered)
    d = differing(r["demod.A"], want)
    record_parity(f"gpu_demod.A[{name}]", words=int(want.size), differing=d, passes=int(r["demod.passes"][0]))
    assert covered.all() and int(r["demod.passes"][0]) == 2 * case.spp and w * h > 1024 and (want != F(case.spp)).any()
    assert d == 0


@pytest.mark.parametrize("name", list(DC.SUM_CASES))
def test_demodulated_sum_at_one_sample_per_round(rd, oracle, name):
    """Four rounds of a frame at multisample = 1.  L_r: round r's image from rgk_render_round_device into a zeroed accumulator (the
    pinned code).  D == sum over r of fl(L_r / div_r) in round order and A == sum of div_r, on every pixel; the frame's accumulator
    is the sum of the L_r."""
    scene, (w, h), lens = DC.SUM_CASES[name]
    r = run_of(rd, name)
    desc, osc = oracle_scene(oracle, scene)
    cam = DC.camera_of(scene, w, h, lens)
    n_tiles = len(oracle.generate_task_list(w, h))
    Dw, Aw, Sw = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
    for k in range(DC.SUM_ROUNDS):
        div, covered = D.sample_divisors(oracle, osc, desc, cam, oracle.generate_task_list(w, h, 42, k * n_tiles), w, h, 1, FLOOR)
        L = r[f"round{k}.L"]
        Dw = (Dw + D.demod_sum(L[:, :, None, :], div, covered)).astype(F)
        Aw = (Aw + D.divisor_sum(div, covered)).astype(F)
        Sw = (Sw + L).astype(F)
    dD, dA, dS = differing(r["rounds.D"], Dw), differing(r["rounds.A"], Aw), differing(r["rounds.accum"], Sw)
    lit = float((Dw != Sw).any(axis=-1).mean())
    print(f"D [{name}]: D {dD}, A {dA}, accum {dS} of {Dw.size} words differ; pixels where D is not the accumulator: {lit:.3f}")
    record_parity(f"gpu_demod.D[{name}]", words=int(Dw.size), differing_D=dD, differing_A=dA, differing_accum=dS, share_demodulated=lit)
    assert (r["rounds.count"] == DC.SUM_ROUNDS).all() and lit > 0.05
    assert dD == 0 and dA == 0 and dS == 0


# ----------------------------------------------------------------------- 4. many samples: exact scalings
UNIFORM_SIZE = (37, 19)
_UNIFORM = {}


def uniform_builder(v):
    if v not in _UNIFORM:
        _UNIFORM[v] = D.uniform_albedo(DC.fixture("box6").builder, v)
    return _UNIFORM[v]


@pytest.mark.parametrize("spp", [8, 16])
@pytest.mark.parametrize("v", [1.0, 0.5])
def test_uniform_albedo_scales_exactly(rd, v, spp):
    """box6 with every material diffuse of one solid colour v under a black sky, the tuning variants of test 1: at 37 x 19 sample_group
    0 and 3, beam 0 and 1, a lens and two samples per pass; at 41 x 29 -- above the smallest batch of 1024 paths, as in test 1 -- two
    pixel ranges x one sample pass per sample (batch_paths = 1024), so the second range's pixels (j0 = 1024) are held to an
    expectation too.  The pass count is asserted.  v = 1: every divisor is 1, so D == accum and A == count.  v = 0.5: D == 2 x accum --
    doubling is exact, and a sample that misses adds 0 either way -- and A == count / 2 where every sample of a pixel hits."""
    import torch
    bad = []
    cases = [(UNIFORM_SIZE,) + var for var in DC.variants(UNIFORM_SIZE, spp)] + [(DC.SPLIT_SIZE, "pixel-ranges", dict(batch_paths=1024), False, 2 * spp)]
    for (w, h), tag, tuning, lens, passes in cases:
        g, pl = DC.fresh_scene(rd, uniform_builder(v), tuning), DC.Planes(w, h)
        cam, prm = DC.camera_of("box6", w, h, lens), DC.params_of("box6", w, h, spp)
        torch.cuda.synchronize()
        g.render_round_demod_device(cam, prm, rd.generate_task_list(w, h), pl.accum.data_ptr(), pl.count.data_ptr(), pl.demod.data_ptr(), pl.div.data_ptr(), FLOOR)
        r = pl.host()
        got_passes = DC.passes_of(g, prm.depth)
        g.close()
        scale = F(1) / F(v)
        d = differing(r["demod"], (r["accum"] * scale).astype(F))
        n = r["count"].astype(F)[..., None]
        a_ok = np.array_equal(r["div"], np.broadcast_to(n, r["div"].shape)) if v == 1.0 else bool(((r["div"] >= n * F(v)) & (r["div"] <= n)).all() and (r["div"] == n * F(v)).any())
        if d or not a_ok or got_passes != passes or not float(r["accum"].max()) > 0 or not (r["count"] == spp).all():
            bad.append((tag, d, a_ok, got_passes, passes))
    record_parity(f"gpu_demod.uniform[v {v}, {spp} spp]", variants=len(cases), bad=len(bad))
    assert not bad, bad


# ----------------------------------------------------------------------- 5. rgk_remodulate_device, and both entries' refusals
@pytest.mark.parametrize("size", [(67, 45), (1, 1)])
def test_remodulate_equals_the_restatement(rd, size):
    import torch
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    img = (rng.standard_normal((h, w, 3)) * 10.0 ** rng.uniform(-3, 3, (h, w, 3))).astype(F)
    A = rng.uniform(0, 40, (h, w, 3)).astype(F)
    n = rng.integers(0, 33, (h, w)).astype(np.uint32)
    alb = rng.uniform(-0.2, 1.3, (h, w, 3)).astype(F)
    alb[rng.random((h, w, 3)) < 0.2] = 0.0
    alb[rng.random((h, w, 3)) < 0.2] *= F(0.01)
    if size == (1, 1):
        n[...] = 0
    g = rd.Scene(DC.fixture("rubiks").builder.to_desc())
    up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")
    d_img, d_A, d_n, d_alb = up(img), up(A), up(n), up(alb)
    for floor in (0.0, 0.02, 0.25):
        for tag, div, cnt, want in (("count", d_A, d_n, D.remodulate(img, A, n, floor)), ("albedo", d_alb, None, D.remodulate(img, alb, None, floor))):
            out = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            g.remodulate_device(w, h, d_img.data_ptr(), div.data_ptr(), None if cnt is None else cnt.data_ptr(), out.data_ptr(), floor)
            torch.cuda.synchronize()
            assert differing(out.cpu().numpy(), want) == 0, (size, floor, tag)
    # refusals on a live scene: the stated status, nothing launched, the planes as they were
    lib, cam, prm = g.lib, DC.camera_of("rubiks", w, h), DC.params_of("rubiks", w, h, 1)
    tiles = rd.generate_task_list(w, h)
    pl = DC.Planes(w, h)
    call = lambda **kw: lib.rgk_render_round_demod_device(g.h, C.byref(cam), C.byref(kw.get("prm", prm)), tiles, len(tiles), pl.accum.data_ptr(), pl.count.data_ptr(),
                                                          kw.get("demod", pl.demod.data_ptr()), kw.get("div", pl.div.data_ptr()), kw.get("floor", FLOOR), None)
    assert call(demod=None) == INVALID and call(div=None) == INVALID and call(floor=-1.0) == INVALID and call(floor=float("nan")) == INVALID and call(floor=float("inf")) == INVALID
    rev = capi.Params.from_buffer_copy(prm)
    rev.reverse = 2
    assert call(prm=rev) == UNSUPPORTED and b"reverse" in lib.rgk_last_error()
    deep = capi.Params.from_buffer_copy(prm)
    deep.depth = 63
    assert call(prm=deep) == UNSUPPORTED
    assert lib.rgk_remodulate_device(g.h, w, h, d_img.data_ptr(), d_A.data_ptr(), d_n.data_ptr(), -0.5, pl.demod.data_ptr()) == INVALID
    assert lib.rgk_remodulate_device(g.h, w, h, d_img.data_ptr(), d_A.data_ptr(), d_n.data_ptr(), FLOOR, d_img.data_ptr()) == INVALID
    torch.cuda.synchronize()
    r = pl.host()
    assert not r["accum"].any() and not r["count"].any() and not r["demod"].any() and not r["div"].any()
    g.close()


def test_timing_slots(rd):
    """rgk_scene_get_post_timing 8 (the remodulate launch) and 9 (a demodulated round's divisor launches and second resolves, summed
    over its passes): filled only while "time_post" is on, and the timed round's planes are the untimed round's."""
    import torch
    w, h, spp = 37, 19, 8
    cam, prm, tiles = DC.camera_of("spheres", w, h), DC.params_of("spheres", w, h, spp), rd.generate_task_list(w, h)
    res = []
    for timed in (0, 1):
        g, pl = DC.fresh_scene(rd, DC.fixture("spheres").builder, dict(batch_paths=2 * w * h, time_post=timed)), DC.Planes(w, h)
        torch.cuda.synchronize()
        g.render_round_demod_device(cam, prm, tiles, pl.accum.data_ptr(), pl.count.data_ptr(), pl.demod.data_ptr(), pl.div.data_ptr(), FLOOR)
        out = torch.empty_like(pl.demod)
        g.remodulate_device(w, h, pl.demod.data_ptr(), pl.div.data_ptr(), pl.count.data_ptr(), out.data_ptr(), FLOOR)
        t8, t9 = g.post_timing(8), g.post_timing(9)
        assert (len(t8), len(t9)) == ((1, 2) if timed else (0, 0)) and all(0 < t < 100 for t in t8 + t9), (timed, t8, t9)
        res.append(pl.host())
        g.close()
    for k in res[0]:
        assert differing(res[0][k], res[1][k]) == 0, k


# ----------------------------------------------------------------------- 6. the driver
LOW, FULL, DRV_SPP = (24, 24), (48, 48), 8


@pytest.fixture(scope="module")
def drivers(rd):
    """Two drivers of cornell-box-spheres at 24 x 24 x 8 spp on scenes of their own, with and without track_demod, two rounds each."""
    import upsample_cases as UC
    sc = UC.SceneSet("spheres")
    g, gp = rd.Scene(sc.builder.to_desc()), rd.Scene(sc.builder.to_desc())
    drv = rd.RenderDriver(g, sc.cfg(*LOW, DRV_SPP), sc.camera(*LOW), track_demod=True, albedo_floor=FLOOR)
    plain = rd.RenderDriver(gp, sc.cfg(*LOW, DRV_SPP), sc.camera(*LOW))
    for d in (drv, plain):
        d.render_round()
        d.render_round()
    return sc, g, drv, plain


def host(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def test_driver_total_ob_is_byte_identical(drivers):
    _, _, drv, plain = drivers
    assert host(drv.total_ob.data).tobytes() == host(plain.total_ob.data).tobytes() and host(drv.total_ob.count).tobytes() == host(plain.total_ob.count).tobytes()
    assert (host(drv.total_ob.count) == 2 * DRV_SPP).all() and [c.as_dict()["path_rays"] for c in drv.counters] == [c.as_dict()["path_rays"] for c in plain.counters]
    n = host(drv.total_ob.count).astype(F)[..., None]
    assert differing(host(drv.irradiance()), (host(drv.demod_ob.data) / n).astype(F)) == 0 and differing(host(drv.albedo_mean()), (host(drv.div_ob.data) / n).astype(F)) == 0


def test_driver_denoise_filters_the_irradiance_and_multiplies_back(drivers):
    """denoise() == post_ref.atrous_ref(D, n, ..., demodulate = 0) followed by demod_ref.remodulate with A / n -- whatever the
    parameters' demodulate says -- and the default sigma_color is taken from D / n."""
    _, _, drv, plain = drivers
    a = {k: host(v) for k, v in drv.render_aov().items()}
    Dp, Ap, n = host(drv.demod_ob.data), host(drv.div_ob.data), host(drv.total_ob.count)
    dp = capi.DenoiseParams(iterations=3, sigma_color=1.5, demodulate=1)
    got = host(drv.denoise(dp))
    filtered = PR.atrous_ref(Dp, n, a["albedo"], a["normal"], a["depth"], iterations=3, sigma_color=1.5, sigma_depth=dp.sigma_depth,
                             normal_power_log2=dp.normal_power_log2, demodulate=0)
    want = D.remodulate(filtered, Ap, n)
    d = differing(got, want)
    record_parity("gpu_demod.driver.denoise", words=int(want.size), differing=d)
    assert d == 0 and differing(got, host(plain.denoise(dp))) > 0
    p = drv.default_denoise_params()
    assert p.demodulate == 0 and p.sigma_color == pytest.approx(PR.default_sigma_color(Dp, n, 6.0), rel=1e-5)
    assert plain.default_denoise_params().demodulate == 1


@pytest.mark.parametrize("denoise", [False, True])
def test_driver_upsample_reconstructs_the_irradiance_and_multiplies_back(drivers, denoise):
    """upsample() == upsample_ref on D as the low accumulator with demodulate = 0 [, the filter at demodulate = 0 with the full planes
    and counts of 1], then demod_ref.remodulate with the full grid's albedo plane through the floor rule."""
    import upsample_ref as U
    sc, _, drv, _ = drivers
    cam = sc.camera(*FULL)
    up = capi.UpsampleParams(plane_tol=0.05, normal_cos=-1.0, demodulate=1, albedo_floor=0.3)  # (demodulate is overruled; the floor is the driver's)
    dp = capi.DenoiseParams(iterations=2, sigma_color=1.5, demodulate=1)
    got, sup = drv.upsample(cam, *FULL, params=up, denoise=dp if denoise else None)
    got, sup = host(got), host(sup)
    low = {k: host(v) for k, v in drv.render_aov().items()}
    full = {k: host(v) for k, v in drv._up_aov.items()}
    Dp, n = host(drv.demod_ob.data), host(drv.total_ob.count)
    m, want_sup = U.upsample_ref(cam, full["albedo"], full["normal"], full["depth"], drv.camera, Dp, n, low["albedo"], low["normal"], low["depth"],
                                 plane_tol=0.05, normal_cos=-1.0, demodulate=0, albedo_floor=0.3)
    if denoise:
        m = PR.atrous_ref(m, np.ones(FULL[::-1], np.uint32), full["albedo"], full["normal"], full["depth"], iterations=2, sigma_color=1.5,
                          sigma_depth=dp.sigma_depth, normal_power_log2=dp.normal_power_log2, demodulate=0)
    want = D.remodulate(m, full["albedo"], None, FLOOR)
    d = differing(got, want)
    record_parity(f"gpu_demod.driver.upsample[denoise {denoise}]", words=int(want.size), differing=d, support_differing=int((sup != want_sup).sum()))
    assert d == 0 and (sup == want_sup).all() and float(want.max()) > 0


def test_driver_checkpoint_carries_both_sums(rd, drivers, tmp_path):
    """2 rounds + save + load + 2 rounds == 4 rounds for D and A (and the accumulator); a checkpoint without `.demod` is refused."""
    sc, _, drv, _ = drivers
    path = str(tmp_path / "frame.ckpt")
    drv.save_checkpoint(path)
    assert sorted(os.listdir(str(tmp_path))) == ["frame.ckpt", "frame.ckpt.demod", "frame.ckpt.div"]
    g2, g4 = rd.Scene(sc.builder.to_desc()), rd.Scene(sc.builder.to_desc())
    resumed = rd.RenderDriver(g2, sc.cfg(*LOW, DRV_SPP), sc.camera(*LOW), track_demod=True, albedo_floor=FLOOR)
    resumed.load_checkpoint(path)
    assert (resumed.rounds_done, resumed.seedcount) == (drv.rounds_done, drv.seedcount) == (2, 2)
    whole = rd.RenderDriver(g4, sc.cfg(*LOW, DRV_SPP), sc.camera(*LOW), track_demod=True, albedo_floor=FLOOR)
    for _ in range(2):
        resumed.render_round()
    for _ in range(4):
        whole.render_round()
    for name in ("total_ob", "demod_ob", "div_ob"):
        assert differing(host(getattr(resumed, name).data), host(getattr(whole, name).data)) == 0, name
    assert (host(resumed.total_ob.count) == 4 * DRV_SPP).all()
    os.remove(path + ".demod")
    again = rd.RenderDriver(g2, sc.cfg(*LOW, DRV_SPP), sc.camera(*LOW), track_demod=True)
    with pytest.raises(RuntimeError, match="demod"):
        again.load_checkpoint(path)
    assert again.rounds_done == 0 and not host(again.total_ob.data).any()
    for kw, word in ((dict(track_noise=True), "track_noise"), (dict(history=rd.TemporalHistory()), "history"), (dict(aov_hops=1), "aov_hops"),
                     (dict(world_size=2), "world_size"), (dict(track_noise=True, adaptive=capi.AdaptParams(0.1, 4)), "track_noise")):
        with pytest.raises(ValueError, match=word):
            rd.RenderDriver(g2, sc.cfg(*LOW, DRV_SPP), sc.camera(*LOW), track_demod=True, **kw)
    bidirectional = sc.cfg(*LOW, DRV_SPP)
    bidirectional.get_params().reverse = 2  # (the configuration hands out one parameter object)
    with pytest.raises(ValueError, match="reverse"):
        rd.RenderDriver(g2, bidirectional, sc.camera(*LOW), track_demod=True)


# ----------------------------------------------------------------------- the command line
def test_cli_demod_writes_the_irradiance_and_leaves_the_plain_output(rd, tmp_path):
    """--denoise --demod on a 50 x 42 textureless configuration, two rounds: `<out>.exr` byte-identical to the run without --demod,
    `<out>.irradiance.exr` and `<out>.denoised.exr` what the driver's irradiance() and denoise() give, scaled like `<out>`."""
    from rgk_amd.config import load_config
    from test_gpu_upsample import SCENE
    cfg_path = tmp_path / "s.json"
    cfg_path.write_text(SCENE)
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir(); b.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for d, extra in ((a, ["--demod"]), (b, [])):
        r = subprocess.run([sys.executable, "-m", "rgk_amd", str(cfg_path), "-D", str(d), "-q", "--denoise"] + extra, cwd=str(tmp_path), env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
    assert sorted(os.listdir(str(b))) == ["t.denoised.exr", "t.exr"] and sorted(os.listdir(str(a))) == ["t.denoised.exr", "t.exr", "t.irradiance.exr"]
    assert (a / "t.exr").read_bytes() == (b / "t.exr").read_bytes()
    assert (a / "t.denoised.exr").read_bytes() != (b / "t.denoised.exr").read_bytes()
    cfg = load_config(str(cfg_path))
    g = rd.Scene(cfg.build_scene().to_desc())
    drv = rd.RenderDriver(g, cfg, cfg.get_camera(0.0), track_demod=True)
    drv.render_round()
    drv.render_round()
    scale = drv.total_ob.write(str(tmp_path / "again.exr"), getattr(cfg, "output_scale", -1.0))
    assert (tmp_path / "again.exr").read_bytes() == (a / "t.exr").read_bytes()
    rd.write_exr(str(tmp_path / "irr.exr"), (drv.irradiance() * scale).cpu().numpy())
    rd.write_exr(str(tmp_path / "den.exr"), (drv.denoise() * scale).cpu().numpy())
    assert (tmp_path / "irr.exr").read_bytes() == (a / "t.irradiance.exr").read_bytes()
    assert (tmp_path / "den.exr").read_bytes() == (a / "t.denoised.exr").read_bytes()
