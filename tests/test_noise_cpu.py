"""Half-buffer noise estimate and variance-guided filter, the part that needs no GPU: ABI, argument errors, the launch plans, the
numpy restatement (tests/noise_ref.py) on known answers and on the oracle's own images, and the command line's resume rule."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi

import noise_ref as N
import post_ref as R
from conftest import ROOT, record_parity

F = np.float32
INVALID = -1


def test_struct_layouts_and_defaults_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    vp = ["iterations", "sigma_k", "sigma_depth", "normal_power_log2", "demodulate", "albedo_floor"]
    nt = ["sum_var", "sum_sq", "n_estimable"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgk.h"\nint main(){printf("%zu %zu", sizeof(rgk_denoise_var_params), sizeof(rgk_noise_tile));'
                   + "".join(f'printf(" %zu", offsetof(rgk_denoise_var_params, {f}));' for f in vp)
                   + "".join(f'printf(" %zu", offsetof(rgk_noise_tile, {f}));' for f in nt) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    V, T = capi.DenoiseVarParams, capi.NoiseTile
    assert got == [C.sizeof(V), C.sizeof(T)] + [getattr(V, f).offset for f in vp] + [getattr(T, f).offset for f in nt]
    d = V()
    assert (d.iterations, d.normal_power_log2, d.demodulate) == (5, 6, 1) and abs(d.sigma_depth - 0.02) < 1e-9
    assert d.sigma_k == 3.0 and d.albedo_floor == 0.25  # the minimum of tools/noise_sweep.py
    for name in ("rgk_noise_estimate_device", "rgk_denoise_variance_device"):
        assert name in capi.EXPORTS


def test_argument_errors_of_both_entries_need_no_gpu(product_lib):
    """Reported before the scene or a device is touched: the `scene` below is 64 bytes of nothing."""
    lib = product_lib
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    bufs = [np.zeros(8 * 8 * 3, np.float32) for _ in range(9)]
    acc, cnt, hacc, hcnt, alb, nrm, z, out, var = [b.ctypes.data for b in bufs]
    tiles = (capi.NoiseTile * 4)()
    ne = lib.rgk_noise_estimate_device
    good = [scene, 8, 8, 4, acc, cnt, hacc, hcnt, tiles, var]
    for k in (0, 4, 5, 6, 7, 8):  # scene, accumulator, counts, half-buffer, its counts, tiles
        a = list(good)
        a[k] = None
        assert ne(*a) == INVALID, k
    for k, v in ((1, 0), (2, 0), (1, 65536), (2, 70000), (3, 0)):  # resolution, tile_size
        a = list(good)
        a[k] = v
        assert ne(*a) == INVALID, (k, v)
    assert b"tile_size" in lib.rgk_last_error()
    for k in (4, 5, 6, 7):  # the variance plane on top of an input
        a = list(good)
        a[9] = a[k]
        assert ne(*a) == INVALID, k
    assert ne(scene, 8, 8, 4, acc, cnt, acc, hcnt, tiles, var) == INVALID  # the half-buffer is the accumulator

    dv = lib.rgk_denoise_variance_device
    dp = capi.DenoiseVarParams()
    good = [scene, 8, 8, acc, cnt, hacc, hcnt, alb, nrm, z, C.byref(dp), out, var]
    for k in (0, 3, 4, 5, 6, 8, 9, 10, 11):  # everything but the albedo plane and out_variance
        a = list(good)
        a[k] = None
        assert dv(*a) == INVALID, k
    a = list(good)
    a[7] = None
    assert dv(*a) == INVALID and b"albedo" in lib.rgk_last_error()  # demodulate needs the albedo plane
    for k, v in ((1, 0), (2, 65536)):
        a = list(good)
        a[k] = v
        assert dv(*a) == INVALID, (k, v)
    for k in (3, 4, 5, 6, 7, 8, 9):  # no output on top of an input
        for o in (11, 12):
            a = list(good)
            a[o] = a[k]
            assert dv(*a) == INVALID, (k, o)
    a = list(good)
    a[12] = a[11]
    assert dv(*a) == INVALID
    for field, v in (("iterations", 17), ("normal_power_log2", 17), ("sigma_k", 0.0), ("sigma_k", -1.0), ("sigma_k", float("nan")),
                     ("sigma_k", float("inf")), ("sigma_k", 1e-30), ("sigma_depth", -1.0), ("albedo_floor", -0.5), ("albedo_floor", float("nan")),
                     ("albedo_floor", float("inf"))):  # (1e-30 squared is below the float range)
        bad = capi.DenoiseVarParams()
        setattr(bad, field, v)
        a = list(good)
        a[10] = C.byref(bad)
        assert dv(*a) == INVALID, (field, v)
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(scene, 4, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(scene, 3, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


def test_post_launch_plans(tmp_path):
    """rgk_plan.h on the CPU: the grids of the new launches, expected values written out by hand."""
    src = tmp_path / "p.cpp"
    src.write_text('#include "rgk_plan.h"\n#include <cstdio>\nint main(){int bad=0;\n#define CHECK(c) do{ if(!(c)){std::fprintf(stderr,"%s\\n",#c);bad++;} }while(0)\n'
                   "CHECK(rgk_post_pixel_grid(1)==1u); CHECK(rgk_post_pixel_grid(256)==1u); CHECK(rgk_post_pixel_grid(257)==2u); CHECK(rgk_post_pixel_grid((size_t)65535*65535)==16776705u);\n"
                   "RgkGrid2 g=rgk_post_filter_grid(67,45); CHECK(g.x==3u&&g.y==6u); g=rgk_post_filter_grid(1,1); CHECK(g.x==1u&&g.y==1u); g=rgk_post_filter_grid(1920,1080); CHECK(g.x==60u&&g.y==135u);\n"
                   "g=rgk_nz_tile_grid(67,45,32); CHECK(g.x==3u&&g.y==2u&&g.count()==6u); g=rgk_nz_tile_grid(67,45,5); CHECK(g.x==14u&&g.y==9u);\n"
                   "g=rgk_nz_tile_grid(65535,65535,1); CHECK(g.x==65535u&&g.y==65535u&&g.count()==(size_t)65535*65535); g=rgk_nz_tile_grid(65535,3,0xffffffffu); CHECK(g.x==1u&&g.y==1u);\n"
                   "return bad;}")
    exe = tmp_path / "p"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "rgk_amd", "csrc"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True).returncode == 0


def _flat(y=9, x=13):
    """One plane facing the viewer at one depth, albedo with a texel below the floor and a black one."""
    rng = np.random.default_rng(3)
    alb = (0.3 + 0.6 * rng.random((y, x, 3))).astype(F)
    alb[1, 2] = [1e-4, 0.5, 0.0]
    nrm = np.zeros((y, x, 3), F)
    nrm[..., 2] = 1
    return alb, nrm, np.full((y, x), 2.0, F)


def test_known_answer_two_constant_halves_of_unequal_size():
    """n_A = 2 n_B, every pixel a in the even rounds and b in the odd ones: v = |a - b|^2 * 2/9 and rel = sqrt(v / |c|^2) with
    c = (2a + b) / 3, whatever the tile size; the filter leaves the constant image alone and shrinks its variance."""
    y, x = 9, 13
    a, b = F([1.5, 3.0, 0.75]), F([0.5, 1.0, 0.25])
    nB = np.full((y, x), 2, np.uint32)
    n = np.full((y, x), 6, np.uint32)
    SB = np.broadcast_to(b * F(2), (y, x, 3)).astype(F)
    S = (np.broadcast_to(a * F(4), (y, x, 3)) + SB).astype(F)
    v = N.raw_variance(S, n, SB, nB)
    assert np.all(v == F(5.25) * (F(8) / F(36))) and np.allclose(v, 5.25 * 2 / 9, rtol=1e-6)  # |a - b|^2 = 1 + 4 + 0.25
    c = (2 * a.astype(np.float64) + b) / 3
    want = np.sqrt(5.25 * 2 / 9 / (c @ c))
    for ts in (32, 5, 1):
        sums, ne = N.noise_tiles(S, n, SB, nB, ts)
        assert ne.sum() == y * x and sums.shape[:2] == (-(-y // ts), -(-x // ts))
        assert abs(N.rel_noise(sums) / want - 1) < 1e-6
    # a pixel with an empty half is not estimable: variance 0, left out of every sum
    nB2 = nB.copy()
    nB2[4, 4] = 0
    sums, ne = N.noise_tiles(S, n, SB, nB2, 32)
    assert N.raw_variance(S, n, SB, nB2)[4, 4] == 0 and ne.sum() == y * x - 1 and abs(N.rel_noise(sums) / want - 1) < 1e-6
    nB2[4, 4] = 6  # ... and so is one whose odd half holds every sample
    assert N.raw_variance(S, n, SB, nB2)[4, 4] == 0
    _, nrm, z = _flat(y, x)
    alb = np.full((y, x, 3), 0.5, F)  # one albedo: the demodulated image is constant too, its variance 4 v
    for demod in (0, 1):
        img, var = N.variance_atrous_ref(S, n, SB, nB, alb, nrm, z, demodulate=demod)
        assert np.allclose(img, c, rtol=1e-5)
        # d2 = 0 everywhere: wc = 1, and one iteration of the 5 x 5 kernel alone leaves (70 / 256)^2 < 0.075 of the variance
        assert np.all(var[2:-2, 2:-2] < 0.075 * v[0, 0] * (4 if demod else 1)) and np.all(var >= 0)
    img, var = N.variance_atrous_ref(S, n, SB, nB, alb, nrm, z, iterations=0)
    assert np.array_equal(img, R.mean_color(S, n)) and np.array_equal(var, v)


def test_identical_halves_give_variance_zero_and_the_image_back():
    """a == b in every pixel: v = 0, and with var_p + var_q = 0 a tap of another colour has wc = 1 / (1 + d2 / 1e-20), below
    2^-24 of the centre's weight, so every sum is the centre tap's: out = (w c) / w, which is c to two roundings (2^-23
    relative; three more with the division by and the multiplication with the albedo)."""
    rng = np.random.default_rng(9)
    y, x = 9, 13
    SB = (rng.random((y, x, 3)) * 8).astype(F)
    S = SB * F(2)
    n, nB = np.full((y, x), 8, np.uint32), np.full((y, x), 4, np.uint32)
    alb, nrm, z = _flat(y, x)
    c = R.mean_color(S, n)
    assert np.all(N.raw_variance(S, n, SB, nB) == 0)
    sums, ne = N.noise_tiles(S, n, SB, nB, 4)
    assert np.all(sums[..., 0] == 0) and ne.sum() == y * x and N.rel_noise(sums) == 0
    for demod, tol in ((0, 2.0 ** -22), (1, 2.0 ** -21)):
        img, var = N.variance_atrous_ref(S, n, SB, nB, alb, nrm, z, demodulate=demod)
        assert np.all(var == 0)
        assert np.allclose(img, c, rtol=tol, atol=0)


def test_the_divisor_is_floored_and_black_albedo_divides_by_one():
    y, x = 9, 13
    rng = np.random.default_rng(4)
    SB = (rng.random((y, x, 3)) * 4).astype(F)
    S = (SB + rng.random((y, x, 3)).astype(F) * 4).astype(F)
    n, nB = np.full((y, x), 4, np.uint32), np.full((y, x), 2, np.uint32)
    alb, nrm, z = _flat(y, x)
    nrm[:] = 0  # nothing is live: every pixel passes through, so the variance plane is prepare's
    _, var = N.variance_atrous_ref(S, n, SB, nB, alb, nrm, z, albedo_floor=0.25)
    h = (S[1, 2] - SB[1, 2]) / F(2) - SB[1, 2] / F(2)
    hd = h / F([0.25, 0.5, 1.0])  # 1e-4 -> the floor, 0.5 stays, 0 -> 1
    assert var[1, 2] == ((hd[0] * hd[0] + hd[1] * hd[1]) + hd[2] * hd[2]) * (F(4) / F(16))


SCENE = '{"output-file": "n.exr", "output-width": 16, "output-height": 16, "multisample": 1, "rounds": 2, "camera": {"position": [0,1,5], "lookat": [0,0,0]},' \
        ' "materials": [{"name": "m", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5]}], "scene": [{"primitive": "plane", "material": "m"}]}'


@pytest.mark.parametrize("switch", [["--noise"], ["--until-noise", "0.1"]], ids=["noise", "until-noise"])
def test_cli_refuses_a_resume_without_the_half_buffer(tmp_path, switch):
    """Decided from the files alone, before the scene is built or a GPU is asked for."""
    cfg = tmp_path / "s.json"
    cfg.write_text(SCENE)
    ck = tmp_path / "f.ck"
    ck.write_bytes(b"a checkpoint written without noise tracking")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rgk_amd", str(cfg), "-D", str(tmp_path), "--checkpoint", str(ck)] + switch, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot resume" in r.stdout and "f.ck.half" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["f.ck", "s.json"]


def test_variance_guided_beats_the_fixed_filter_on_the_oracles_cornell(oracle):
    """The quality gate: Cornell 96 x 96, halves of 2 + 2 spp (tile seeds from seedstart 42 and 100042) against 256 spp, features
    composed from the oracle.  The restatement at the shipped defaults must have strictly lower rel-L2 than atrous_ref at its
    shipped defaults (k = 6, demodulate 1).  Measured: 0.1165 against 0.1536 (noisy 0.4126)."""
    _, name, scale, lo, hi = N.CASES[0]
    (S, n, SB, nB), ref, (alb, nrm, z, _) = N.oracle_case(oracle, name, scale, lo, hi)
    assert S.shape == (96, 96, 3) and np.all(n == 4) and np.all(nB == 2)
    from rgk_amd import render_driver as rd
    d, dv = capi.DenoiseParams(), capi.DenoiseVarParams()
    fixed = R.atrous_ref(S, n, alb, nrm, z, d.iterations, R.default_sigma_color(S, n, rd.DENOISE_SIGMA_K), d.sigma_depth, d.normal_power_log2, d.demodulate)
    guided, _ = N.variance_atrous_ref(S, n, SB, nB, alb, nrm, z, dv.iterations, dv.sigma_k, dv.sigma_depth, dv.normal_power_log2, dv.demodulate, dv.albedo_floor)
    c = R.mean_color(S, n)
    e_fixed, e_guided = R.rel_l2(fixed, ref), R.rel_l2(guided, ref)
    sums, _ = N.noise_tiles(S, n, SB, nB, 32)
    record_parity("noise_cpu.quality[cornell 96x96, 2+2 vs 256 spp]", noisy_rel_l2=R.rel_l2(c, ref), fixed_rel_l2=e_fixed, guided_rel_l2=e_guided,
                  estimated_rel_noise=N.rel_noise(sums))
    assert e_guided < e_fixed
