"""The half-buffer noise estimate (rgk_noise_estimate_device) and the variance-guided filter (rgk_denoise_variance_device) against
their numpy restatement (tests/noise_ref.py), bit for bit, and both end to end through RenderDriver and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera
from rgk_amd.workloads import Workload

import noise_ref as N
import post_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

SIZES = [(96, 96), (67, 45), (1, 1)]
# estimated relative noise / measured rel-L2 of the noisy image against 256 spp, measured on the CPU with the oracle's Cornell
# 96 x 96 images from the raw variance plane (tools/noise_sweep.py).  Below 1 because the estimate divides by |c|,
# the noisy image's own norm, and rel-L2 by the reference's: |c|^2 ~ |ref|^2 (1 + 0.41^2); sum(v) / sum|c - ref|^2 itself is 0.996.
ORACLE_RATIO = 0.9189


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cornell_camera(wl, W, H):
    c = wl.builder.extra["camera"]
    return make_camera(c["pos"], c["lookat"], c["up"], fov=c["fov"], xres=W, yres=H)


@pytest.fixture(scope="module")
def frames(rd):
    """The GPU's own rounds of 2 spp of the Cornell box at the three sizes, with the driver's seeds, as three feeds each:
    "2+2" (two rounds, the second is the half), "4+2" (three rounds: n_A != n_B) and "holes" (2+2 with a block of pixels whose odd
    half is empty, one pixel whose odd half holds everything and one pixel without samples), and the feature planes."""
    wl = Workload("cornell-256", spp=2)
    g, out = rd.Scene(wl.builder.to_desc()), {}
    for W, H in SIZES:
        cam, prm = cornell_camera(wl, W, H), wl.params()
        prm.xres, prm.yres = W, H
        rounds, base = [], 0
        for _ in range(3):
            tiles = rd.generate_task_list(W, H, rd.SEEDSTART, base)
            base += len(tiles)
            rounds.append(g.render_round(cam, prm, tiles)[:2])
        (s0, n0), (s1, n1), (s2, n2) = rounds
        feeds = {"2+2": (s0 + s1, n0 + n1, s1.copy(), n1.copy()), "4+2": ((s0 + s1) + s2, n0 + n1 + n2, s1.copy(), n1.copy())}
        S, n, SB, nB = [a.copy() for a in feeds["2+2"]]
        if (W, H) != (1, 1):
            SB[10:20, 5:15], nB[10:20, 5:15] = 0, 0
            SB[3, 40], nB[3, 40] = S[3, 40], n[3, 40]
            S[5, 7], n[5, 7], SB[5, 7], nB[5, 7] = 0, 0, 0, 0
        else:
            SB[:], nB[:] = 0, 0
        feeds["holes"] = (S, n, SB, nB)
        out[(W, H)] = (feeds, g.render_aov(cam, prm, rd.generate_task_list(W, H))[:3])
    return g, out


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def gpu_denoise_var(g, feed, alb, nrm, z, dp, want_variance=True):
    import torch
    H, W = z.shape
    t = [up(a) for a in feed + (alb, nrm, z)]
    out = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
    var = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g.denoise_variance_device(W, H, *[x.data_ptr() for x in t], dp, out.data_ptr(), var.data_ptr() if want_variance else None)
    return out.cpu().numpy(), var.cpu().numpy()


def ref_denoise_var(feed, alb, nrm, z, dp):
    return N.variance_atrous_ref(*feed, alb, nrm, z, dp.iterations, dp.sigma_k, dp.sigma_depth, dp.normal_power_log2, dp.demodulate, dp.albedo_floor)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("demodulate", [0, 1])
def test_variance_guided_filter_equals_the_numpy_restatement(frames, size, demodulate):
    """np.array_equal on the image and on the output variance, the GPU's own accumulators and feature planes on both sides.
    67 x 45 is narrower than the last iteration's reach (2 * 16 pixels each way) and no multiple of the 32 x 8 workgroup."""
    g, data = frames
    feeds, (alb, nrm, z) = data[size]
    for name, feed in feeds.items():
        dp = capi.DenoiseVarParams(demodulate=demodulate)
        got, gvar = gpu_denoise_var(g, feed, alb, nrm, z, dp)
        want, wvar = ref_denoise_var(feed, alb, nrm, z, dp)
        differ = int((bits(got) != bits(want)).any(axis=-1).sum())
        vdiffer = int((bits(gvar) != bits(wvar)).sum())
        c = R.mean_color(feed[0], feed[1])
        record_parity(f"gpu_noise.denoise[{size[0]}x{size[1]},demod={demodulate},{name}]", pixels_differ=differ, variance_differs=vdiffer,
                      pixels_changed=float((got != c).any(axis=-1).mean()))
        assert differ == 0 and vdiffer == 0, name
        if size != (1, 1):
            assert (got != c).any(axis=-1).mean() > 0.5 and (gvar > 0).mean() > 0.5  # it filtered, and the variance is carried
    feed = feeds["holes"]
    # without the variance output the image is the same
    dp = capi.DenoiseVarParams(demodulate=demodulate)
    assert np.array_equal(bits(gpu_denoise_var(g, feed, alb, nrm, z, dp, want_variance=False)[0]), bits(ref_denoise_var(feed, alb, nrm, z, dp)[0]))
    # iterations 0: the image itself and the raw variance, with or without demodulation
    dp0 = capi.DenoiseVarParams(iterations=0, demodulate=demodulate)
    got, gvar = gpu_denoise_var(g, feed, alb, nrm, z, dp0)
    assert np.array_equal(bits(got), bits(R.mean_color(feed[0], feed[1]))) and np.array_equal(bits(gvar), bits(N.raw_variance(*feed)))
    # fewer iterations (the LDS form alone, then one gather step), other widths, no floor: the restatement follows
    for it in (2, 3):
        dp2 = capi.DenoiseVarParams(iterations=it, sigma_k=1.5, sigma_depth=0.1, normal_power_log2=1, demodulate=demodulate, albedo_floor=0.0)
        got, gvar = gpu_denoise_var(g, feeds["4+2"], alb, nrm, z, dp2)
        want, wvar = ref_denoise_var(feeds["4+2"], alb, nrm, z, dp2)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(gvar), bits(wvar))


def test_a_frame_of_misses_comes_back_as_c(frames):
    g, data = frames
    feed = data[(67, 45)][0]["4+2"]
    zero3, zero = np.zeros_like(feed[0]), np.zeros(feed[1].shape, np.float32)
    for demodulate in (0, 1):
        got, gvar = gpu_denoise_var(g, feed, zero3, zero3, zero, capi.DenoiseVarParams(demodulate=demodulate))
        assert np.array_equal(bits(got), bits(R.mean_color(feed[0], feed[1])))
        assert np.array_equal(bits(gvar), bits(N.raw_variance(*feed)))  # (black albedo divides by 1)


@pytest.mark.parametrize("size,tile_size", [((96, 96), 32), ((67, 45), 32), ((67, 45), 5), ((1, 1), 32)], ids=["96x96/32", "67x45/32", "67x45/5", "1x1/32"])
def test_noise_estimate_equals_the_restatement(frames, size, tile_size):
    """The raw variance plane bit for bit, n_estimable exactly, and the per-tile doubles within 1e-9 relative of numpy's float64
    sums of the same float32 terms: a tile is at most 2^22 additions in double, each within 2^-53 relative of non-negative
    terms, whatever the order -- 2^-31 < 1e-9.  67 x 45: ragged tiles at the right and bottom edges."""
    import torch
    g, data = frames
    W, H = size
    for name, feed in data[size][0].items():
        t = [up(a) for a in feed]
        var = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        tiles = g.noise_estimate_device(W, H, tile_size, *[x.data_ptr() for x in t], var.data_ptr())
        tiles2 = g.noise_estimate_device(W, H, tile_size, *[x.data_ptr() for x in t], None)  # without the plane; and the same bits every run
        assert tiles.tobytes() == tiles2.tobytes()
        sums, ne = N.noise_tiles(*feed, tile_size)
        assert tiles.shape == ne.shape == (-(-H // tile_size), -(-W // tile_size))
        assert np.array_equal(bits(var.cpu().numpy()), bits(N.raw_variance(*feed))), name
        assert np.array_equal(tiles["n_estimable"], ne), name
        got = np.stack([tiles["sum_var"], tiles["sum_sq"]], axis=-1)
        err = float(np.max(np.abs(got - sums) / np.where(sums > 0, sums, 1.0)))
        record_parity(f"gpu_noise.tiles[{W}x{H}/{tile_size},{name}]", max_rel_err=err, estimable=int(ne.sum()), rel_noise=N.rel_noise(got))
        assert err <= 1e-9 and np.all(got[sums == 0] == 0), name
        if name == "holes" and size != (1, 1):
            assert int(ne.sum()) == W * H - 100 - 2
        elif size != (1, 1):
            assert int(ne.sum()) == W * H
        else:
            assert int(ne.sum()) == (0 if name == "holes" else 1)


# ----------------------------------------------------------------------- end to end
def _driver(rd, wl, scene=None, rounds=1, **kw):
    class Cfg:
        xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, rounds, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    return rd.RenderDriver(scene or rd.Scene(wl.builder.to_desc()), Cfg, wl.camera, **kw)


@pytest.fixture(scope="module")
def cornell_2_2(rd):
    """Cornell 96 x 96: a tracked driver after two rounds of 2 spp, an untracked one after the same rounds, and the 256-spp image."""
    lo, hi = Workload("cornell-256", scale=0.375, spp=2), Workload("cornell-256", scale=0.375, spp=256)
    ref_drv = _driver(rd, hi)
    ref_drv.render_round()
    ref = ref_drv.total_ob.get_pixels().cpu().numpy()
    scene = rd.Scene(lo.builder.to_desc())
    drv, plain = _driver(rd, lo, scene, track_noise=True), _driver(rd, lo, scene)
    drv.render_round()
    first = drv.noise()
    drv.render_round()
    for _ in range(2):
        plain.render_round()
    return lo, scene, drv, plain, ref, first


def test_tracking_keeps_the_accumulators_bits_and_needs_two_rounds(rd, cornell_2_2):
    lo, scene, drv, plain, ref, first = cornell_2_2
    assert first is None  # after one round
    assert np.array_equal(bits(drv.total_ob.data.cpu().numpy()), bits(plain.total_ob.data.cpu().numpy()))
    assert np.array_equal(drv.total_ob.count.cpu().numpy(), plain.total_ob.count.cpu().numpy())
    assert plain.noise() is None and plain.half_ob is None
    with pytest.raises(ValueError):
        plain.denoise(variance=True)
    # the half is the second round alone
    one = _driver(rd, lo, scene)
    one.render_round()
    S, SB = drv.total_ob.data.cpu().numpy(), drv.half_ob.data.cpu().numpy()
    assert np.allclose(S - SB, one.total_ob.data.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert (drv.half_ob.count.cpu().numpy() == 2).all() and (drv.total_ob.count.cpu().numpy() == 4).all()
    nz = drv.noise()
    assert set(nz) == {"rel", "tiles", "variance"} and nz["tiles"].shape == (3, 3) and tuple(nz["variance"].shape) == (96, 96)
    feed = (S, drv.total_ob.count.cpu().numpy().view(np.uint32), SB, drv.half_ob.count.cpu().numpy().view(np.uint32))
    assert np.array_equal(bits(nz["variance"].cpu().numpy()), bits(N.raw_variance(*feed)))
    assert abs(nz["rel"] / N.rel_noise(N.noise_tiles(*feed, 32)[0]) - 1) < 1e-9
    assert drv.noise(tile_size=5)["tiles"].shape == (20, 20)


def test_the_estimate_is_calibrated_against_256_spp(cornell_2_2):
    """Estimated relative noise over the measured rel-L2(c, image at 256 spp), on the GPU's own images: within a factor of 1.25
    either way of the ratio the oracle's images give on the CPU.  The 256-spp image itself carries 4/256 of the variance; the
    rest is the spread of a one-degree-of-freedom estimator summed over about 9 k pixels."""
    lo, scene, drv, plain, ref, _ = cornell_2_2
    est = drv.noise()["rel"]
    measured = R.rel_l2(drv.total_ob.get_pixels().cpu().numpy(), ref)
    record_parity("gpu_noise.calibration[cornell 96x96, 2+2 vs 256 spp]", estimated=est, measured=measured, ratio=est / measured, oracle_ratio=ORACLE_RATIO)
    assert ORACLE_RATIO / 1.25 <= est / measured <= ORACLE_RATIO * 1.25


def test_variance_guided_denoise_beats_the_fixed_filter(cornell_2_2):
    lo, scene, drv, plain, ref, _ = cornell_2_2
    fixed = drv.denoise().cpu().numpy()
    guided = drv.denoise(variance=True).cpu().numpy()
    assert np.array_equal(bits(fixed), bits(plain.denoise().cpu().numpy()))  # the fixed filter does not see the tracking
    img, var = drv.denoise_variance()
    assert np.array_equal(bits(guided), bits(img.cpu().numpy())) and float(var.min()) >= 0 and float(var.max()) > 0
    noisy = drv.total_ob.get_pixels().cpu().numpy()
    a, b, c = R.rel_l2(noisy, ref), R.rel_l2(fixed, ref), R.rel_l2(guided, ref)
    record_parity("gpu_noise.end_to_end[cornell 96x96, 2+2 vs 256 spp]", noisy_rel_l2=a, fixed_rel_l2=b, guided_rel_l2=c)
    assert c < b < a


def test_calls_between_rounds_change_no_bit_and_one_round_falls_back(rd, cornell_2_2):
    lo, scene, _, _, _, _ = cornell_2_2
    drv = _driver(rd, lo, scene, track_noise=True)
    drv.render_round()
    assert np.array_equal(bits(drv.denoise(variance=True).cpu().numpy()), bits(drv.denoise().cpu().numpy()))  # fewer than two rounds: the fixed filter
    drv.render_round()
    drv.noise()
    drv.denoise(variance=True)
    drv.render_round()
    drv.noise(tile_size=7)
    drv.denoise_variance(capi.DenoiseVarParams(iterations=3, demodulate=0))
    drv.render_round()
    quiet, plain = _driver(rd, lo, scene, track_noise=True), _driver(rd, lo, scene)
    for _ in range(4):
        quiet.render_round()
        plain.render_round()
    for a, b in ((drv.total_ob, quiet.total_ob), (drv.half_ob, quiet.half_ob), (drv.total_ob, plain.total_ob)):
        assert np.array_equal(bits(a.data.cpu().numpy()), bits(b.data.cpu().numpy())) and np.array_equal(a.count.cpu().numpy(), b.count.cpu().numpy())
    assert (drv.half_ob.count.cpu().numpy() == 4).all()


def test_render_frame_stops_at_a_noise_level(rd, cornell_2_2):
    lo, scene, _, _, _, _ = cornell_2_2
    probe = _driver(rd, lo, scene, track_noise=True)
    for _ in range(4):
        probe.render_round()
    X = 0.7 * probe.noise()["rel"]
    drv = _driver(rd, lo, scene, rounds=64, track_noise=True)
    seen = []
    drv.render_frame(rounds=64, until_noise=X, on_noise=lambda r, rel: seen.append((r, rel)))
    rel = drv.noise()["rel"]
    record_parity("gpu_noise.until_noise[cornell 96x96, 2 spp rounds]", target=X, rounds=drv.rounds_done, rel=rel)
    assert 2 <= drv.rounds_done < 64 and drv.rounds_done != 4 and rel <= X  # (after 4 rounds it was X / 0.7)
    assert [r for r, _ in seen] == list(range(2, drv.rounds_done + 1)) and all(v > X for _, v in seen[:-1]) and seen[-1][1] == rel
    # `rounds` still bounds it
    short = _driver(rd, lo, scene, rounds=3, track_noise=True)
    short.render_frame(rounds=3, until_noise=1e-6)
    assert short.rounds_done == 3
    with pytest.raises(ValueError):
        _driver(rd, lo, scene).render_frame(rounds=1, until_noise=0.1)


def test_checkpoints_carry_the_half_buffer(rd, cornell_2_2, tmp_path):
    """Saved beside the checkpoint as `<file>.half`; a resumed driver continues with the same bits, and a checkpoint written
    without tracking is refused by a tracking driver."""
    lo, scene, drv, plain, _, _ = cornell_2_2
    ck = str(tmp_path / "f.ck")
    drv.save_checkpoint(ck)
    assert sorted(os.listdir(str(tmp_path))) == ["f.ck", "f.ck.half"]
    back = _driver(rd, lo, scene, track_noise=True)
    back.load_checkpoint(ck)
    assert (back.rounds_done, back.seedcount) == (drv.rounds_done, drv.seedcount) == (2, 18)
    for a, b in ((back.total_ob, drv.total_ob), (back.half_ob, drv.half_ob)):
        assert np.array_equal(bits(a.data.cpu().numpy()), bits(b.data.cpu().numpy())) and np.array_equal(a.count.cpu().numpy(), b.count.cpu().numpy())
    assert back.noise()["rel"] == drv.noise()["rel"]
    _driver(rd, lo, scene).load_checkpoint(ck)  # an untracked driver takes the total and ignores the half
    ck2 = str(tmp_path / "plain.ck")
    plain.save_checkpoint(ck2)
    assert not os.path.exists(ck2 + ".half")
    with pytest.raises(RuntimeError, match="plain.ck.half"):
        _driver(rd, lo, scene, track_noise=True).load_checkpoint(ck2)


SCENE = '''{
    "output-file": "post.exr", "output-width": 48, "output-height": 40, "multisample": 4, "rounds": 3, "recursion-max": 3, "clamp": 20,
    "camera": {"position": [0,1.2,5], "lookat": [0,0.8,0], "fov": 35},
    "materials": [{"name": "m", "brdf": "diffuse", "diffuse255": [255, 128, 0]},
                  {"name": "g", "brdf": "ltc_ggx_diffuse", "exponent": 200, "specular": [0.3,0.3,0.3], "diffuse": [0.4,0.4,0.5]},
                  {"name": "l", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5], "emission": [9,9,8]}],
    "scene": [{"primitive": "cube", "material": "m", "translate": [0,0.5,0]},
              {"primitive": "plane", "material": "g", "scale": [4,1,4]},
              {"primitive": "plane", "material": "l", "scale": [0.5,1,0.5], "translate": [0,3,0], "rotate": [180, 0, 0]}],
    "sky": {"color": [0.3, 0.4, 0.6], "intensity": 0.5}
}'''


def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([sys.executable, "-m", "rgk_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def test_cli_writes_the_noise_image_and_the_half_beside_an_unchanged_output(rd, tmp_path):
    cfg = tmp_path / "s.json"
    cfg.write_text(SCENE)
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir(); b.mkdir()
    r = run_cli([str(cfg), "-D", str(a), "--noise", "--denoise", "--checkpoint", str(a / "f.ck"), "-q"], str(tmp_path))
    assert r.returncode == 0, r.stderr + r.stdout
    rels = [float(ln.split()[-1]) for ln in r.stdout.splitlines() if "relative noise" in ln]
    assert len(rels) == 2 and all(0 < v < 1 for v in rels), r.stdout  # after rounds 2 and 3
    r = run_cli([str(cfg), "-D", str(b), "--denoise", "-q"], str(tmp_path))
    assert r.returncode == 0, r.stderr + r.stdout
    assert "relative noise" not in r.stdout
    assert sorted(os.listdir(str(b))) == ["post.denoised.exr", "post.exr"]
    assert sorted(os.listdir(str(a))) == ["f.ck", "f.ck.half", "post.denoised.exr", "post.exr", "post.noise.exr"]
    assert (a / "post.exr").read_bytes() == (b / "post.exr").read_bytes()
    noise, plain = rd.read_exr(str(a / "post.noise.exr")), rd.read_exr(str(a / "post.exr"))
    assert noise.shape == (40, 48, 4) and (noise[..., 3] == 1).all() and np.isfinite(noise).all() and (noise[..., :3] >= 0).all() and noise[..., :3].max() > 0
    assert np.array_equal(noise[..., 0], noise[..., 1]) and np.array_equal(noise[..., 0], noise[..., 2])
    # --denoise took the variance-guided filter
    da, db = rd.read_exr(str(a / "post.denoised.exr")), rd.read_exr(str(b / "post.denoised.exr"))
    assert np.isfinite(da).all() and not np.array_equal(da, db) and not np.array_equal(da[..., :3], plain[..., :3])
