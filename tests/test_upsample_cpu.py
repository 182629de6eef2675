"""Guided upsampling, the part that needs no GPU: what tests/upsample_ref.py's restatement of the two kernels MEANS, on synthetic
planes whose answers are known from the geometry, and the ABI, parameter ranges, argument errors and command-line refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rgk_amd import capi

import temporal_ref as T
import upsample_ref as U
from conftest import ROOT

F = np.float32
INVALID = -1
W, H, WL, HL = 32, 24, 8, 6  # 4 x lower on each axis, the same view rectangle
XVIEW, YVIEW = 1.0, 0.75


def camera():
    return T.pinhole_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), XVIEW, YVIEW)


def planes(cam, w, h, surfaces, sky=False):
    """Feature planes of `cam` on a w x h grid over fronto-parallel surfaces [(distance in front of the camera, inside(u, v), id)],
    nearest first; u, v: where a ray crosses the view screen, in units of FULL-grid pixels (the centre of full pixel (x, y) is
    (x + 0.5, y + 0.5)), so one predicate serves both grids.  Normal +z, depth the ray's t.  -> depth, normal, id (-1: nothing)."""
    o, d = T.camera_rays(cam, w, h)
    u = (d[..., 0] / -d[..., 2] / F(XVIEW) + F(0.5)) * W
    v = (-d[..., 1] / -d[..., 2] / F(YVIEW) + F(0.5)) * H
    depth, sid = np.zeros((h, w), F), np.full((h, w), -1, np.int32)
    for dist, inside, k in reversed(surfaces):
        on = inside(u, v)
        depth[on], sid[on] = (F(dist) / -d[..., 2])[on], k
    normal = np.where((sid >= 0)[..., None], F([0, 0, 1]), F(0)).astype(F)
    return depth, normal, sid


EVERYWHERE = lambda u, v: np.ones(u.shape, bool)
ALBEDO = F(0.75)


def case(surfaces, radiance, count=4, **kw):
    """Both grids over `surfaces`; the low accumulator holds `count` samples of radiance[id] per pixel (radiance[-1]: where nothing
    is hit), every albedo is 0.75 on a surface and 0 beside it.  The radiances below are 0.75 x a power of two: m is a power of
    two, w * m is exact, so a weighted mean of equal m's is m itself bit for bit whatever the weights.
    -> (out, support, id plane of the full grid, id plane of the low grid, plain low image)."""
    cam = camera()
    zf, nf, sf = planes(cam, W, H, surfaces)
    zl, nl, sl = planes(cam, WL, HL, surfaces)
    rad = np.array([radiance[k] for k in sorted(radiance)], F)  # index id + 1
    c = np.repeat(rad[sl + 1][..., None], 3, axis=-1)
    cnt = np.full((HL, WL), count, np.uint32)
    af = np.where((sf >= 0)[..., None], ALBEDO, F(0)) * np.ones(3, F)
    al = np.where((sl >= 0)[..., None], ALBEDO, F(0)) * np.ones(3, F)
    out, sup = U.upsample_ref(cam, af.astype(F), nf, zf, cam, (c * F(count)).astype(F), cnt, al.astype(F), nl, zl, **kw)
    return out, sup, sf, sl, (cam, nf, zf, c)


def ulps(a, b):
    return np.abs(a.astype(F).view(np.int32).astype(np.int64) - np.asarray(b, F).view(np.int32).astype(np.int64))


def test_two_surfaces_at_different_depths_do_not_bleed_and_a_plain_upscale_does():
    """A near surface left of u = 13.3 over a far wall, constant radiance each.  No full pixel takes a tap from the other surface:
    each side is its constant to within 2 ulp; the bilinear upscale of the same low image mixes them along the edge."""
    scene = [(2.0, lambda u, v: u < 13.3, 1), (6.0, EVERYWHERE, 0)]
    rad = {-1: 0.0, 0: 0.375, 1: 3.0}
    out, sup, sf, sl, (cam, nf, zf, c) = case(scene, rad)
    assert (sup == 1).all()  # a straight edge: the next low centre of a pixel's own surface is always one of its four taps
    for k in (0, 1):
        want = np.full(3, rad[k], F)
        assert ulps(out[sf == k], want).max() <= 2, k
    plain = U.bilinear_ref(cam, nf, zf, cam, c)
    bleed = (np.abs(plain[..., 0] - np.where(sf == 1, F(3.0), F(0.375))) > 0.1)
    assert bleed[sf == 0].any() and bleed[sf == 1].any()
    # with the plane and normal tests switched off the guided stage bleeds as well
    loose, _, _, _, _ = case(scene, rad, plane_tol=10.0, normal_cos=-1.0)
    assert (np.abs(loose[..., 0] - np.where(sf == 1, F(3.0), F(0.375))) > 0.1).any()


def test_a_thin_strip_whose_ring_1_is_empty_resolves_through_ring_2():
    """A strip about one low pixel wide, running diagonally.  (An axis-aligned strip cannot empty ring 1: between a full pixel of the
    strip and the next low centre on it lies no other low centre, so that centre is one of the pixel's four taps.)  Along a diagonal
    there are full pixels on the strip none of whose four bracketing low centres is: they take the strip's radiance from the 4 x 4
    ring, support 2, and not the wall's."""
    strip = lambda u, v: np.abs((v - 12.0) + (u - 16.0) / 3.0) < 1.3
    out, sup, sf, sl, _ = case([(2.0, strip, 1), (6.0, EVERYWHERE, 0)], {-1: 0.0, 0: 0.375, 1: 3.0})
    on = sf == 1
    assert (sl == 1).sum() >= 2 and on.sum() > 40
    via2 = on & (sup == 2)
    assert via2.sum() >= 4
    assert ulps(out[via2], np.full(3, 3.0, F)).max() <= 2
    assert ulps(out[on & (sup == 1)], np.full(3, 3.0, F)).max() <= 2
    assert ulps(out[(sf == 0) & (sup > 0)], np.full(3, 0.375, F)).max() <= 2


def test_a_feature_no_low_centre_hits_gets_the_nearest_plain_colour():
    """A near blob between the low grid's centre rays (full columns 18.2 .. 19.8, rows 10.2 .. 11.8; low centres sit at 4 k + 2):
    no tap anywhere is on its surface, so its pixels get c of the nearest low pixel -- the wall's plain colour -- and support 0."""
    blob = lambda u, v: (u > 18.2) & (u < 19.8) & (v > 10.2) & (v < 11.8)
    out, sup, sf, sl, _ = case([(2.0, blob, 1), (6.0, EVERYWHERE, 0)], {-1: 0.0, 0: 0.375, 1: 3.0})
    assert (sl != 1).all() and (sf == 1).sum() == 4
    assert (sup[sf == 1] == 0).all() and (sup[sf == 0] == 1).all()
    assert np.array_equal(out[sf == 1], np.full((4, 3), 0.375, F))  # not demodulated, not re-modulated: c itself
    # a low pixel without samples is no tap, and as the nearest it gives 0
    out0, sup0, _, _, _ = case([(2.0, blob, 1), (6.0, EVERYWHERE, 0)], {-1: 0.0, 0: 0.375, 1: 3.0}, count=0)
    assert (sup0 == 0).all() and (out0 == 0).all()


def test_flat_pixels_take_only_flat_taps():
    """Sky (no normal, depth 0, albedo 0) right of u = 17.7 beside a wall: sky pixels are carried by direction and mix only sky,
    wall pixels only wall."""
    out, sup, sf, sl, _ = case([(4.0, lambda u, v: u < 17.7, 0)], {-1: 2.0, 0: 0.375})
    assert (sf == -1).any() and (sl == -1).any() and (sup > 0).all()
    assert np.array_equal(out[sf == -1], np.full(((sf == -1).sum(), 3), 2.0, F))  # div = 1 on both grids
    assert ulps(out[sf == 0], np.full(3, 0.375, F)).max() <= 2
    # a camera looking the other way finds nothing: !(qd > 0)
    cam, back = camera(), T.pinhole_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), XVIEW, YVIEW)
    z, n = np.zeros((H, W), F), np.zeros((H, W, 3), F)
    zl, nl = np.zeros((HL, WL), F), np.zeros((HL, WL, 3), F)
    o, s = U.upsample_ref(back, n, n, z, cam, np.ones((HL, WL, 3), F), np.ones((HL, WL), np.uint32), nl, nl, zl)
    assert (o == 0).all() and (s == 0).all()


def test_identical_grids_return_the_image():
    """Ratio 1, identical cameras: every pixel projects onto itself (to within float rounding of the coordinate) and the output
    is the low image to that accuracy."""
    cam = camera()
    z, n, s = planes(cam, W, H, [(4.0, EVERYWHERE, 0)])
    rng = np.random.default_rng(5)
    img = rng.uniform(0.5, 1.5, (H, W, 3)).astype(F)
    alb = np.full((H, W, 3), 0.5, F)
    out, sup = U.upsample_ref(cam, alb, n, z, cam, img * F(2), np.full((H, W), 2, np.uint32), alb, n, z)
    assert (sup == 1).all() and np.abs(out - img).max() < 1e-3


# ----------------------------------------------------------------------- ABI, parameter ranges, argument errors
FIELDS = ["plane_tol", "normal_cos", "demodulate", "albedo_floor"]
BAD_PARAMS = [("plane_tol", -0.1), ("normal_cos", 1.5), ("normal_cos", -1.5), ("albedo_floor", -1.0)] + [
    (f, v) for f in FIELDS if f != "demodulate" for v in (float("nan"), float("inf"))]


def test_struct_layout_defaults_and_exports_match_the_header(tmp_path, product_lib):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgk.h"\nint main(){printf("%zu", sizeof(rgk_upsample_params));'
                   + "".join(f'printf(" %zu", offsetof(rgk_upsample_params, {f}));' for f in FIELDS) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = capi.UpsampleParams
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS]
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    assert set(re.findall(r"\b(rgk_[a-z_]+)\s*\(", hdr)) == set(capi.EXPORTS)
    assert "rgk_upsample_device" in capi.EXPORTS and product_lib.rgk_upsample_device is not None
    proto = re.search(r"int rgk_upsample_device\s*\(([^;]*)\);", hdr).group(1)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]
    assert len(args) == len(product_lib.rgk_upsample_device.argtypes) == 18
    d = capi.UpsampleParams().check()
    assert (round(d.plane_tol, 6), round(d.normal_cos, 6), d.demodulate, round(d.albedo_floor, 6)) == (0.05, -1.0, 0, 0.02)  # the shipped values


_KEEP = []


def _good_call():
    """An argument list the entry would accept, on a `scene` that is 64 bytes of nothing: every refusal below is reported before
    the scene or a device is touched."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    bufs = [np.zeros(8 * 8 * 3, np.float32) for _ in range(10)]
    cams = [capi.Camera(), capi.Camera()]
    cams[0].xsize, cams[0].ysize, cams[1].xsize, cams[1].ysize = 8, 8, 2, 2
    up = capi.UpsampleParams(demodulate=1)
    _KEEP.append((fake, bufs, cams, up))
    p = [b.ctypes.data for b in bufs]
    #       0      1  2  3                  4..6    7  8  9                  10..14    15             16    17
    return [scene, 8, 8, C.byref(cams[0])] + p[:3] + [2, 2, C.byref(cams[1])] + p[3:8] + [C.byref(up), p[8], p[9]], cams


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_each_refused_parameter_is_refused_by_the_wrapper_and_by_the_entry(product_lib, field, value):
    bad = capi.UpsampleParams()
    setattr(bad, field, value)
    with pytest.raises(ValueError):
        bad.check()
    a, _ = _good_call()
    a[15] = C.byref(bad)
    assert product_lib.rgk_upsample_device(*a) == INVALID and product_lib.rgk_last_error()


def test_argument_errors_need_no_gpu(product_lib):
    lib, fn = product_lib, product_lib.rgk_upsample_device
    good, cams = _good_call()
    for k in (0, 3, 5, 6, 9, 10, 11, 13, 14, 15, 16):  # every pointer but the two albedo planes and the support plane is needed
        a = list(good)
        a[k] = None
        assert fn(*a) == INVALID and b"null" in lib.rgk_last_error(), k
    for k in (4, 12):  # an albedo plane is needed with demodulate ...
        a = list(good)
        a[k] = None
        assert fn(*a) == INVALID and b"albedo" in lib.rgk_last_error(), k
    for k, v in ((1, 0), (2, 0), (1, 65536), (2, 70000), (7, 0), (8, 0), (7, 65536), (8, 70000)):
        a = list(good)
        a[k] = v
        assert fn(*a) == INVALID and b"resolution" in lib.rgk_last_error(), (k, v)
    for k, v in ((1, 9), (2, 7), (7, 3), (8, 1)):  # a camera made for another grid
        a = list(good)
        a[k] = v
        assert fn(*a) == INVALID and b"xsize" in lib.rgk_last_error(), (k, v)
    for i in (4, 5, 6, 10, 11, 12, 13, 14):  # no output on top of an input, nor on the other output
        for o in (16, 17):
            a = list(good)
            a[o] = a[i]
            assert fn(*a) == INVALID and b"output" in lib.rgk_last_error(), (i, o)
    a = list(good)
    a[17] = a[16]
    assert fn(*a) == INVALID
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(good[0], 8, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(good[0], 7, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


def test_driver_and_cli_refusals(tmp_path, capsys):
    from rgk_amd import render_driver as rd
    from rgk_amd.__main__ import main

    class Cfg:
        xres, yres, render_rounds, render_minutes = 8, 8, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: capi.Params())
    drv = rd.RenderDriver(None, Cfg, None, device="cpu")
    p = drv.default_upsample_params()
    assert isinstance(p, capi.UpsampleParams) and bytes(p) == bytes(capi.UpsampleParams())
    with pytest.raises(ValueError, match="upsample_to"):
        drv.render_frame(rounds=0, output_file=str(tmp_path / "o.exr"), upsampled_file=str(tmp_path / "u.exr"))
    with pytest.raises(ValueError, match="aov_hops"):
        rd.RenderDriver(None, Cfg, None, device="cpu", aov_hops=2).upsample(None, 32, 32)
    cfg = str(tmp_path / "absent.json")  # refused before the file is looked at
    assert main([cfg, "--upsample"]) == 1
    assert "ERROR: --upsample needs -p" in capsys.readouterr().out
    for extra, word in ((["--denoise", "--temporal"], "--temporal"), (["--noise"], "--noise"), (["--until-noise", "0.1"], "--until-noise"),
                        (["--until-noise", "0.1", "--adaptive"], "--until-noise"), (["--aov", "--aov-hops", "2"], "--aov-hops"), (["-d", "1", "1"], "-d")):
        assert main([cfg, "-p", "--upsample"] + extra) == 1, extra
        out = capsys.readouterr().out
        assert "ERROR: --upsample cannot be combined with " + word in out, (extra, out)
    assert main([cfg, "-p", "--upsample", "-q"]) == 1 and "Failed to load config file" in capsys.readouterr().out  # accepted: it got as far as the file
