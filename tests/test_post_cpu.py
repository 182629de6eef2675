"""Feature buffers and the a-trous denoiser, the part that needs no GPU: ABI, argument errors, and the filter's numpy restatement
(tests/post_ref.py) on the oracle's own images."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd import render_driver as rd
from rgk_amd.workloads import Workload

import post_ref as R
from conftest import ROOT, record_parity

NEW_ENTRIES = ["rgk_render_aov_device", "rgk_render_aov", "rgk_denoise_device", "rgk_scene_get_post_timing"]


def test_header_exports_and_library_agree_on_the_new_entries(product_lib):
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    declared = set(re.findall(r"\b(rgk_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS)
    for name in NEW_ENTRIES:
        assert name in declared and getattr(product_lib, name) is not None


def test_denoise_params_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgk.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rgk_denoise_params),'
                   "offsetof(rgk_denoise_params, iterations), offsetof(rgk_denoise_params, sigma_color), offsetof(rgk_denoise_params, sigma_depth),"
                   "offsetof(rgk_denoise_params, normal_power_log2), offsetof(rgk_denoise_params, demodulate));return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = capi.DenoiseParams
    assert got == [C.sizeof(P), P.iterations.offset, P.sigma_color.offset, P.sigma_depth.offset, P.normal_power_log2.offset, P.demodulate.offset]
    d = P()
    assert (d.iterations, d.normal_power_log2, d.demodulate) == (5, 6, 1) and abs(d.sigma_depth - 0.02) < 1e-9


def test_argument_errors_of_the_new_entries_need_no_gpu(product_lib):
    """Null and size errors are reported before the scene or a device is touched: the `scene` below is 64 bytes of nothing."""
    lib = product_lib
    INVALID = -1
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    cam, prm, tiles = capi.Camera(), capi.Params(), (capi.Tile * 1)()
    prm.xres, prm.yres = 8, 8
    tiles[0].x0, tiles[0].x1, tiles[0].y0, tiles[0].y1 = 0, 8, 0, 8
    buf = np.zeros(8 * 8 * 3, np.float32)
    p = buf.ctypes.data
    for fn in (lib.rgk_render_aov_device, lib.rgk_render_aov):
        assert fn(None, C.byref(cam), C.byref(prm), tiles, 1, p, p, p, p) == INVALID
        assert fn(scene, None, C.byref(prm), tiles, 1, p, p, p, p) == INVALID
        assert fn(scene, C.byref(cam), None, tiles, 1, p, p, p, p) == INVALID
        assert fn(scene, C.byref(cam), C.byref(prm), None, 1, p, p, p, p) == INVALID
        bad = capi.Params.from_buffer_copy(prm)
        bad.xres = 0
        assert fn(scene, C.byref(cam), C.byref(bad), tiles, 1, p, p, p, p) == INVALID
        bad.xres = 70000
        assert fn(scene, C.byref(cam), C.byref(bad), tiles, 1, p, p, p, p) == INVALID
        tiles[0].x1 = 9  # outside the frame
        assert fn(scene, C.byref(cam), C.byref(prm), tiles, 1, p, p, p, p) == INVALID
        assert b"outside the frame" in lib.rgk_last_error()
        tiles[0].x1 = 8
    dp = capi.DenoiseParams()
    dn = lib.rgk_denoise_device
    out = np.zeros(8 * 8 * 3, np.float32).ctypes.data
    assert dn(None, 8, 8, p, p, p, p, p, C.byref(dp), out) == INVALID
    for k in (3, 4, 6, 7, 8, 9):  # accum_rgb, accum_count, normal, depth, params, out_rgb
        a = [scene, 8, 8, p, p, p, p, p, C.byref(dp), out]
        a[k] = None
        assert dn(*a) == INVALID, k
    assert dn(scene, 8, 8, p, p, None, p, p, C.byref(dp), out) == INVALID  # demodulate needs the albedo plane
    assert dn(scene, 0, 8, p, p, p, p, p, C.byref(dp), out) == INVALID
    assert dn(scene, 8, 65536, p, p, p, p, p, C.byref(dp), out) == INVALID
    assert dn(scene, 8, 8, p, p, p, p, p, C.byref(dp), p) == INVALID  # in place
    for field, v in (("iterations", 17), ("normal_power_log2", 17), ("sigma_color", 0.0), ("sigma_color", float("nan")), ("sigma_depth", -1.0),
                     ("sigma_color", 1e-30)):  # (1e-30 squared is below the float range)
        bad = capi.DenoiseParams()
        setattr(bad, field, v)
        assert dn(scene, 8, 8, p, p, p, p, p, C.byref(bad), out) == INVALID, field
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(None, 0, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(scene, 2, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(scene, 0, None, None) == INVALID


def test_the_filter_restatement_on_hand_made_frames():
    rng = np.random.default_rng(5)
    y, x = 9, 13
    acc = rng.random((y, x, 3)).astype(np.float32) * 8
    cnt = np.full((y, x), 4, np.uint32)
    cnt[2, 3] = 0
    alb = rng.random((y, x, 3)).astype(np.float32)
    z = (1 + rng.random((y, x))).astype(np.float32)
    nrm = np.zeros((y, x, 3), np.float32)
    c = R.mean_color(acc, cnt)
    assert np.all(c[2, 3] == 0) and np.array_equal(c[0, 0], acc[0, 0] / np.float32(4))
    # no normals anywhere: every pixel passes through
    assert np.array_equal(R.atrous_ref(acc, cnt, alb, nrm, z, demodulate=0), c)
    assert np.array_equal(R.atrous_ref(acc, cnt, alb, nrm, z, iterations=0), c)
    # one plane, one depth, a constant image: the weighted mean of equal values is that value to rounding
    nrm[..., 2] = 1
    flat = np.broadcast_to(np.float32([2, 4, 6]), (y, x, 3)) * 4
    out = R.atrous_ref(flat, np.full((y, x), 4, np.uint32), alb, nrm, np.ones((y, x), np.float32), demodulate=0)
    assert np.allclose(out, [2, 4, 6], rtol=1e-6)
    # a normal edge separates: left half faces +z, right half +x, values 1 and 5 do not mix
    nrm[:, 7:] = [1, 0, 0]
    img = np.where(np.arange(x)[None, :, None] < 7, np.float32(1), np.float32(5)) * np.ones((y, x, 3), np.float32)
    out = R.atrous_ref(img * 4, np.full((y, x), 4, np.uint32), alb, nrm, np.ones((y, x), np.float32), sigma_color=100.0, demodulate=0)
    assert np.allclose(out[:, :7], 1, rtol=1e-6) and np.allclose(out[:, 7:], 5, rtol=1e-6)


CASES = [("cornell-256", 0.375, 4, 256, (96, 96)), ("sponza-1080p", 0.06, 4, 128, (115, 64))]


@pytest.mark.parametrize("name,scale,lo,hi,size", CASES, ids=["cornell", "sponza-proxy"])
def test_the_filter_lowers_the_error_of_the_oracles_images(oracle, name, scale, lo, hi, size):
    """relL2(denoised, hi) < relL2(noisy, hi) with the shipped defaults, on the oracle's own renders with features composed
    from orc_camera_ray + orc_trace_closest + orc_texture_sample.  Measured: Cornell 0.409 -> 0.134, Sponza proxy 0.267 -> 0.202."""
    imgs = {}
    for spp in (lo, hi):
        wl = Workload(name, scale=scale, spp=spp)
        assert (wl.xres, wl.yres) == size
        desc = wl.builder.to_desc()
        osc = oracle.OracleScene(desc)
        acc, cnt, _ = osc.render_round(wl.camera, wl.params(), oracle.generate_task_list(wl.xres, wl.yres))
        imgs[spp] = (acc, cnt)
        if spp == lo:
            alb, nrm, z, tri = R.oracle_features(oracle, osc, desc, wl.camera, wl.xres, wl.yres, wl.bumpscale)
    acc, cnt = imgs[lo]
    ref = R.mean_color(*imgs[hi])
    d = capi.DenoiseParams()
    sigma = R.default_sigma_color(acc, cnt, rd.DENOISE_SIGMA_K)
    den = R.atrous_ref(acc, cnt, alb, nrm, z, d.iterations, sigma, d.sigma_depth, d.normal_power_log2, d.demodulate)
    noisy, denoised = R.rel_l2(R.mean_color(acc, cnt), ref), R.rel_l2(den, ref)
    record_parity(f"post_cpu.denoise[{name}]", noisy_rel_l2=noisy, denoised_rel_l2=denoised, sigma_color=sigma)
    assert (tri >= 0).any() and np.all(z[tri < 0] == 0) and np.all(nrm[tri < 0] == 0)
    lens = np.linalg.norm(nrm[tri >= 0].astype(np.float64), axis=-1)
    assert np.all((np.abs(lens - 1) < 1e-5) | (lens == 0))
    assert denoised < noisy
