"""Temporal reuse, the part that needs no GPU: what tests/temporal_ref.py's restatement of the two kernels MEANS, on synthetic
planes whose answers are known from the geometry, and the ABI, parameter ranges and argument errors of the two entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rgk_amd import capi

import temporal_ref as T
from conftest import ROOT, record_parity

F = np.float32
INVALID = -1
W, H = 32, 24
XVIEW, YVIEW = 1.0, 0.75  # square pixels
DIFFUSE, MIRROR = 0, 1


def camera(pos=(0, 0, 0), lookat=None):
    pos = np.array(pos, np.float64)
    lookat = pos + [0, 0, -1] if lookat is None else lookat
    return T.pinhole_camera(pos, lookat, (0, 1, 0), XVIEW, YVIEW)


def planes(cam, surfaces):
    """Feature planes of `cam` over fronto-parallel rectangles: surfaces = [(z, x_lo, x_hi, tri)], nearest first; the normal
    of each is +z.  -> depth, normal, tri."""
    o, d = T.camera_rays(cam, W, H)
    depth, tri = np.zeros((H, W), F), np.full((H, W), -1, np.int32)
    for z, x_lo, x_hi, t in reversed(surfaces):  # nearer ones overwrite
        dist = (F(z) - o[2]) / d[..., 2]
        x = o[0] + d[..., 0] * dist
        on = (dist > 0) & (x >= x_lo) & (x <= x_hi)
        depth[on], tri[on] = dist[on].astype(F), t
    normal = np.where((tri >= 0)[..., None], F([0, 0, 1]), F(0)).astype(F)
    return depth, normal, tri


def history(value=None, length=4.0):
    """A history whose red channel is the pixel's column (or `value`) and whose length is a power of two: the weighted mean
    of equal lengths is then exact."""
    rgb = np.zeros((H, W, 3), F)
    rgb[..., 0] = np.arange(W, dtype=F)[None, :] if value is None else value
    rgb[..., 1] = np.arange(H, dtype=F)[:, None]
    return rgb, np.full((H, W), length, F)


def reproject(cur, prev, surfaces, kinds=(DIFFUSE, DIFFUSE), hist=None, **kw):
    zc, nc, tc = planes(cur, surfaces)
    zp, npv, tp = planes(prev, surfaces)
    rgb, length = hist or history()
    out = T.reproject_ref(cur, prev, zc, nc, tc, zp, npv, tp, rgb, length, np.array(kinds, np.uint32), want_taps=True, **kw)
    return out + (tc, tp)


WALL = [(-4.0, -100.0, 100.0, 0)]
# What a dozen float32 roundings can move a reprojected coordinate by, in pixels: each is at most 2^-24 of a quantity no larger
# than the view screen's corner distance (< 2 here), the last step multiplies by xres = 32: 12 * 2 * 2^-24 * 32 < 5e-5.
COORD_BOUND = 5e-5


def test_identical_cameras_find_every_pixel_where_it_was():
    cam = camera()
    zc, nc, tc = planes(cam, WALL)
    assert (tc >= 0).all()
    _, _, _, q, fx, fy = T.project_ref(cam, cam, zc, tc, W, H)
    ex = float(np.abs(fx - np.arange(W, dtype=F)[None, :]).max())
    ey = float(np.abs(fy - np.arange(H, dtype=F)[:, None]).max())
    print(f"identical cameras: |fx - x| <= {ex:.3g}, |fy - y| <= {ey:.3g} (bound {COORD_BOUND})")
    record_parity("temporal_cpu.identity", fx_err=ex, fy_err=ey)
    assert ex < COORD_BOUND and ey < COORD_BOUND
    rgb, length, ntaps, _, _ = reproject(cam, cam, WALL)
    assert (length > 0).all()
    full = ntaps == 4
    assert full.any() and np.array_equal(length[full], np.full(full.sum(), 4.0, F))
    # the colour comes from the pixel itself, up to the weight COORD_BOUND gives its neighbours (columns differ by 1)
    assert np.abs(rgb[..., 0] - np.arange(W)[None, :]).max() < 2 * COORD_BOUND * W and np.abs(rgb[..., 1] - np.arange(H)[:, None]).max() < 2 * COORD_BOUND * H


@pytest.mark.parametrize("k", [3, -2])
def test_a_sideways_shift_of_k_pixels_takes_history_from_k_columns_away(k):
    """The camera moves parallel to the wall by k pixel widths at the wall's depth (4 * XVIEW / W each): the wall point under
    column x was under column x + k before.  The |k| columns whose point was outside the previous frame get nothing.  (The
    first of them lands exactly one pixel past the previous frame's last pixel centre, fx == xres, which the rule excludes; the
    view is 1 wide, the wall 4 away and the frame 32 columns, so a pixel is 1/8 wide there and the shift is exact in binary.)"""
    pw = 4.0 * XVIEW / W
    prev, cur = camera(), camera(pos=(k * pw, 0, 0))
    rgb, length, ntaps, _, _ = reproject(cur, prev, WALL)
    cols = np.arange(W)
    entering = (cols + k >= W) | (cols + k < 0)
    assert entering.sum() == abs(k)
    assert (length[:, entering] == 0).all() and (rgb[:, entering] == 0).all()
    assert (length[:, ~entering] > 0).all()
    inner = ~entering & (cols + k + 1 < W) & (cols + k - 1 >= 0)
    assert (ntaps[1:-1, inner] == 4).all() and (length[1:-1, inner] == 4).all()
    assert np.abs(rgb[:, ~entering, 0] - (cols[~entering] + k)[None, :]).max() < 2 * COORD_BOUND * W


def test_disocclusion_behind_a_near_occluder():
    """An occluder at depth 2 over a wall at depth 6, the camera shifted: the wall pixels whose previous position was behind
    the occluder get nothing, the pixels still on the occluder keep their history."""
    scene = [(-2.0, -0.31, 0.17, 1), (-6.0, -100.0, 100.0, 0)]
    prev, cur = camera(), camera(pos=(0.21, 0, 0))
    rgb, length, ntaps, tc, tp = reproject(cur, prev, scene)
    # where each current pixel's point was in the previous frame, in float64 from the geometry alone
    o, d = (a.astype(np.float64) for a in T.camera_rays(cur, W, H))
    zc, _, _ = planes(cur, scene)
    x = o + d * zc[..., None].astype(np.float64)
    px = (x[..., 0] / -x[..., 2] / XVIEW + 0.5) * W - 0.5  # the previous camera sits at the origin
    py = (-x[..., 1] / -x[..., 2] / YVIEW + 0.5) * H - 0.5
    assert np.abs(py - np.arange(H)[:, None]).max() < 1e-4 and (tp == tp[0]).all()  # no vertical motion, and every row is the same
    ix = np.floor(px).astype(int)
    inside = (ix >= 0) & (ix + 1 < W) & (np.abs(px - np.round(px)) > 1e-3)
    cx = np.clip(ix, 0, W - 2)
    taps = np.stack([tp[0, cx], tp[0, cx + 1]], axis=-1)  # the two columns the four taps lie in
    uncovered = inside & (tc == 0) & (taps == 1).all(axis=-1)
    still_wall = inside & (tc == 0) & (taps == 0).all(axis=-1)
    still_occluder = inside & (tc == 1) & (taps == 1).all(axis=-1)
    assert uncovered.sum() >= H and still_wall.sum() > 4 * H and still_occluder.sum() >= 2 * H
    assert (length[uncovered] == 0).all() and (rgb[uncovered] == 0).all()
    assert (length[still_wall] == 4).all() and (length[still_occluder] == 4).all()
    rows = slice(1, H - 1)  # (the outermost rows may have their second tap row outside the frame)
    assert (ntaps[rows][still_wall[rows]] == 4).all() and (ntaps[rows][still_occluder[rows]] == 4).all()
    # with the plane test switched off by a huge tolerance the uncovered wall would take the occluder's colours
    _, loose, _, _, _ = reproject(cur, prev, scene, plane_tol=10.0)
    assert (loose[uncovered] == 4).all()


def test_a_camera_turned_around_reuses_nothing():
    prev = camera()
    cur = camera(lookat=np.array([0.0, 0.0, 1.0]))
    back = [(4.0, -100.0, 100.0, 0)]  # what the turned camera sees: a wall behind the first one
    zc, nc, tc = planes(cur, back)
    assert (tc >= 0).all()
    zp, npv, tp = planes(prev, WALL)
    rgb, length = history()
    out_rgb, out_len = T.reproject_ref(cur, prev, zc, nc, tc, zp, npv, tp, rgb, length, np.array([DIFFUSE], np.uint32))
    assert (out_len == 0).all() and (out_rgb == 0).all()
    # ... and so does open sky seen the other way (a miss is a direction)
    miss = np.full((H, W), -1, np.int32)
    zero, zero3 = np.zeros((H, W), F), np.zeros((H, W, 3), F)
    out_rgb, out_len = T.reproject_ref(cur, prev, zero, zero3, miss, zero, zero3, miss, rgb, length, np.zeros(0, np.uint32))
    assert (out_len == 0).all()
    # while sky under identical cameras is found again
    out_rgb, out_len = T.reproject_ref(prev, prev, zero, zero3, miss, zero, zero3, miss, rgb, length, np.zeros(0, np.uint32))
    assert (out_len > 0).all()


def test_specular_dropped_unknown_and_nan_pixels_get_no_history():
    cam = camera()
    zc, nc, tc = planes(cam, WALL)
    rgb, length = history()
    for kind in T.SPECULAR_KINDS:
        _, out_len = T.reproject_ref(cam, cam, zc, nc, tc, zc, nc, tc, rgb, length, np.array([kind], np.uint32))
        assert (out_len == 0).all(), kind
    tri2 = tc.copy()
    tri2[:, : W // 2] = 1  # left half mirror, right half diffuse
    _, out_len = T.reproject_ref(cam, cam, zc, nc, tri2, zc, nc, tri2, rgb, length, np.array([DIFFUSE, MIRROR], np.uint32))
    assert (out_len[:, : W // 2] == 0).all() and (out_len[:, W // 2:] > 0).all()
    n0 = nc.copy()
    n0[5, 7] = 0  # a dropped vertex
    _, out_len = T.reproject_ref(cam, cam, zc, n0, tc, zc, nc, tc, rgb, length, np.array([DIFFUSE], np.uint32))
    assert out_len[5, 7] == 0 and (out_len > 0).sum() == W * H - 1
    _, out_len = T.reproject_ref(cam, cam, zc, nc, tc + 5, zc, nc, tc, rgb, length, np.array([DIFFUSE], np.uint32))  # not the scene's triangle
    assert (out_len == 0).all()
    zn = zc.copy()
    zn[3, 3] = np.nan
    _, out_len = T.reproject_ref(cam, cam, zn, nc, tc, zc, nc, tc, rgb, length, np.array([DIFFUSE], np.uint32))
    assert out_len[3, 3] == 0
    # taps without history, or with another normal, do not count
    l0 = length.copy()
    l0[:, ::2] = 0
    out_rgb, out_len, ntaps = T.reproject_ref(cam, cam, zc, nc, tc, zc, nc, tc, rgb, l0, np.array([DIFFUSE], np.uint32), want_taps=True)
    assert (ntaps <= 2).all() and np.isfinite(out_rgb).all()
    tilted = np.broadcast_to(F([0.6, 0, 0.8]), nc.shape)
    _, out_len = T.reproject_ref(cam, cam, zc, nc, tc, zc, tilted, tc, rgb, length, np.array([DIFFUSE], np.uint32), plane_tol=10.0)
    assert (out_len == 0).all()  # 0.8 < normal_cos


def test_blend_rules():
    P = (2, 3)
    acc = np.full(P + (3,), 8.0, F)
    acc[..., 1] = 4.0
    cnt = np.full(P, 4, np.uint32)  # c = (2, 1, 2)
    alb = np.full(P + (3,), 0.5, F)
    h = np.full(P + (3,), 1.0, F)
    # no history: the frame itself, length 1
    m, L, out = T.blend_ref(acc, cnt, alb, h, np.zeros(P, F), alpha_min=0.1, max_len=10.0)
    assert np.array_equal(m, np.broadcast_to(F([4, 2, 4]), P + (3,))) and (L == 1).all() and np.array_equal(out, acc / 4)
    # length 1: the mean of the two
    m, L, out = T.blend_ref(acc, cnt, alb, h, np.ones(P, F), alpha_min=0.1, max_len=10.0)
    assert np.array_equal(m, np.broadcast_to(F([2.5, 1.5, 2.5]), P + (3,))) and (L == 2).all() and np.array_equal(out, m * F(0.5))
    # length 100: alpha = alpha_min, and the length stops at max_len
    m, L, _ = T.blend_ref(acc, cnt, alb, h, np.full(P, 100.0, F), alpha_min=0.1, max_len=10.0)
    want = (F([4, 2, 4]) - F(1)) * F(0.1) + F(1)
    assert np.array_equal(m, np.broadcast_to(want, P + (3,))) and (L == 10).all()
    # count 0: the history passes through, whatever its length
    c0 = cnt.copy()
    c0[0, 1] = 0
    Lin = np.full(P, 3.0, F)
    Lin[1, 1] = 0
    m, L, out = T.blend_ref(acc, c0, alb, h, Lin, alpha_min=0.1, max_len=10.0)
    assert np.array_equal(m[0, 1], h[0, 1]) and L[0, 1] == 3 and np.array_equal(out[0, 1], h[0, 1] * F(0.5))
    assert L[0, 0] == 4 and L[1, 1] == 1
    # the divisor: floored where the albedo is small, 1 where it is 0, 1 without demodulation
    a2 = alb.copy()
    a2[0, 0] = [0.001, 0.0, 0.5]
    m, _, out = T.blend_ref(acc, cnt, a2, h, np.zeros(P, F), albedo_floor=0.02)
    assert np.array_equal(m[0, 0], F([2, 1, 2]) / F([0.02, 1, 0.5])) and np.array_equal(out[0, 0], m[0, 0] * F([0.02, 1, 0.5]))
    m, _, out = T.blend_ref(acc, cnt, None, h, np.zeros(P, F), demodulate=0)
    assert np.array_equal(m, acc / 4) and np.array_equal(out, m)


# ----------------------------------------------------------------------- ABI, parameter ranges, argument errors
FIELDS = ["plane_tol", "normal_cos", "alpha_min", "max_len", "demodulate", "albedo_floor"]
BAD_PARAMS = [("plane_tol", -0.1), ("normal_cos", 1.5), ("normal_cos", -1.5), ("alpha_min", 0.0), ("alpha_min", -0.2), ("alpha_min", 1.5),
              ("max_len", 0.5), ("albedo_floor", -1.0)] + [(f, v) for f in FIELDS if f != "demodulate" for v in (float("nan"), float("inf"))]


def test_struct_layout_defaults_and_exports_match_the_header(tmp_path, product_lib):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgk.h"\nint main(){printf("%zu", sizeof(rgk_temporal_params));'
                   + "".join(f'printf(" %zu", offsetof(rgk_temporal_params, {f}));' for f in FIELDS) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = capi.TemporalParams
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS]
    for name in ("rgk_temporal_reproject_device", "rgk_temporal_blend_device"):
        assert name in capi.EXPORTS and getattr(product_lib, name) is not None
    capi.TemporalParams().check()


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_each_refused_parameter_is_refused_by_the_wrapper_and_by_both_entries(product_lib, field, value):
    bad = capi.TemporalParams()
    setattr(bad, field, value)
    with pytest.raises(ValueError):
        bad.check()
    lib, (scene, rp, bl) = product_lib, _good_calls()
    rp[13] = bl[8] = C.byref(bad)
    assert lib.rgk_temporal_reproject_device(*rp) == INVALID and lib.rgk_last_error()
    assert lib.rgk_temporal_blend_device(*bl) == INVALID and lib.rgk_last_error()


_KEEP = []


def _good_calls():
    """Argument lists both entries would accept, on a `scene` that is 64 bytes of nothing: every refusal below is reported
    before the scene or a device is touched."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    bufs = [np.zeros(8 * 8 * 3, np.float32) for _ in range(16)]
    cams = [capi.Camera(), capi.Camera()]
    tp = capi.TemporalParams()
    _KEEP.append((fake, bufs, cams, tp))
    p = [b.ctypes.data for b in bufs]
    rp = [scene, 8, 8, C.byref(cams[0]), C.byref(cams[1])] + p[:8] + [C.byref(tp), p[8], p[9]]
    bl = [scene, 8, 8] + p[:5] + [C.byref(tp)] + p[10:13]
    return scene, rp, bl


def test_argument_errors_of_both_entries_need_no_gpu(product_lib):
    lib = product_lib
    rp_fn, bl_fn = lib.rgk_temporal_reproject_device, lib.rgk_temporal_blend_device
    scene, rp, bl = _good_calls()
    for k in range(len(rp)):  # every pointer is needed
        if k in (1, 2):
            continue
        a = list(rp)
        a[k] = None
        assert rp_fn(*a) == INVALID, k
    for k in range(len(bl)):
        if k in (1, 2, 5):  # (the albedo: below)
            continue
        a = list(bl)
        a[k] = None
        assert bl_fn(*a) == INVALID, k
    a = list(bl)
    a[5] = None
    assert bl_fn(*a) == INVALID and b"albedo" in lib.rgk_last_error()
    for fn, good in ((rp_fn, rp), (bl_fn, bl)):
        for k, v in ((1, 0), (2, 0), (1, 65536), (2, 70000)):
            a = list(good)
            a[k] = v
            assert fn(*a) == INVALID and b"resolution" in lib.rgk_last_error(), (k, v)
    for i in range(5, 13):  # no output on top of an input, nor on the other output
        for o in (14, 15):
            a = list(rp)
            a[o] = a[i]
            assert rp_fn(*a) == INVALID and b"output" in lib.rgk_last_error(), (i, o)
    a = list(rp)
    a[15] = a[14]
    assert rp_fn(*a) == INVALID
    for i in range(3, 8):
        for o in (9, 10, 11):
            a = list(bl)
            a[o] = a[i]
            assert bl_fn(*a) == INVALID and b"output" in lib.rgk_last_error(), (i, o)
    for o, o2 in ((9, 10), (9, 11), (10, 11)):
        a = list(bl)
        a[o2] = a[o]
        assert bl_fn(*a) == INVALID
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(scene, 6, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(scene, 5, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


def test_driver_refuses_temporal_with_noise_tracking_and_the_cli_its_combinations(tmp_path):
    from rgk_amd import render_driver as rd
    from rgk_amd.__main__ import main

    class Cfg:
        xres, yres, render_rounds, render_minutes = 8, 8, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: capi.Params())
    with pytest.raises(ValueError, match="track_noise"):
        rd.RenderDriver(None, Cfg, None, device="cpu", track_noise=True, history=rd.TemporalHistory())
    with pytest.raises(ValueError):
        rd.TemporalHistory(capi.TemporalParams(alpha_min=0.0))
    h = rd.TemporalHistory()
    assert h.empty and h.params.max_len == capi.TemporalParams().max_len
    for extra in ([], ["--denoise", "--noise"], ["--denoise", "--until-noise", "0.1"], ["--denoise", "--until-noise", "0.1", "--adaptive"]):
        assert main([str(tmp_path / "absent.json"), "--temporal"] + extra) == 1  # refused before the file is looked at
