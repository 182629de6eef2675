"""The device output path, the part that needs no GPU: the arithmetic the four pack kernels call and the file images the host entries
build around them (rgk_amd/csrc/rgk_pack.h) under ASan + UBSan in a stand-alone program (tests/cpp/pack_main.cpp), held to the host
writers of rgk_output.cpp byte for byte; the ABI of the two new entries and the argument errors they report before a scene or a
device is touched; the driver's and the command line's switch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rgk_amd import capi

from conftest import ROOT

INVALID = -1
CPP = os.path.join(ROOT, "tests", "cpp")
HARNESS_CASES = ["half", "pixel", "scale", "exr", "checksums", "png"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack") / "pack_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "pack_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("case", HARNESS_CASES)
def test_pack_unit_on_the_cpu(harness, case, tmp_path):
    """half: rgk_pack_half against rgk_float_to_half on every half value as a float, its neighbours, the midpoints between halves and
    theirs, the four boundary patterns, zeros, infinities, quiet and signalling NaNs, 2^20 random patterns.  pixel: both pixel
    expressions against rgk_output_normalize and a single multiply, counts up to 2^24 + 1 and 2^32 - 1.  scale: the auto-scale fold
    under three partitions against the host loop, on random, all-zero, all-negative, NaN-holding, signed-zero and infinite frames.
    exr: header, offset table and line blocks against files rgk_output_write_exr wrote at 1 x 1, 3 x 2, 67 x 45.  checksums: the
    stored-block layout and Adler-32 / CRC-32 from pieces against the whole-buffer sums, raw sizes 1, L - 1, L, L + 1, 65535, 65536,
    2 * 65535 + 7 under seven piece lengths.  png: whole files against rgk_output_write_png, one to three blocks, raw byte 65535 a
    filter byte.  That the program links without the HIP runtime is the check that the unit calls nothing of it."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([harness, case, str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout


def test_harness_refuses_an_unknown_case(harness):
    assert subprocess.run([harness, "nothing"], capture_output=True).returncode == 2


# ----------------------------------------------------------------------- ABI
def test_abi_of_the_two_entries(product_lib):
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    for name, n_args in (("rgk_output_write_exr_device", 8), ("rgk_output_write_png_device", 5)):
        assert name in capi.EXPORTS and getattr(product_lib, name) is not None
        proto = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]
        assert len(args) == len(getattr(product_lib, name).argtypes) == n_args, name
    assert "which = 12" in hdr and "which = 13" in hdr


_KEEP = []


def _good_calls(tmp_path):
    """Argument lists both entries would accept, on a `scene` that is 64 bytes of nothing: every refusal below is reported before
    the scene, a device or the file is touched."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    buf = np.zeros(8 * 8 * 3, np.float32)
    _KEEP.append((fake, buf))
    exr = [scene, str(tmp_path / "o.exr").encode(), 8, 8, buf.ctypes.data, buf.ctypes.data, C.c_float(1.0), None]
    png = [scene, str(tmp_path / "o.png").encode(), 8, 8, buf.ctypes.data]
    return exr, png


def test_argument_errors_need_no_gpu_and_create_no_file(product_lib, tmp_path):
    lib = product_lib
    exr, png = _good_calls(tmp_path)
    for fn, good in ((lib.rgk_output_write_exr_device, exr), (lib.rgk_output_write_png_device, png)):
        for k in (0, 1, 4):  # scene, path, pixels
            a = list(good)
            a[k] = None
            assert fn(*a) == INVALID and b"null" in lib.rgk_last_error(), k
        for k, v in ((2, 0), (3, 0), (2, 65536), (3, 70000)):
            a = list(good)
            a[k] = v
            assert fn(*a) == INVALID and b"resolution" in lib.rgk_last_error(), (k, v)
    for scale in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):  # image mode: the scale is always applied
        a = list(exr)
        a[5], a[6] = None, C.c_float(scale)
        assert lib.rgk_output_write_exr_device(*a) == INVALID and b"output_scale" in lib.rgk_last_error(), scale
    assert os.listdir(str(tmp_path)) == []
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(exr[0], 14, None, C.byref(n)) == INVALID
    for which in (12, 13):
        assert lib.rgk_scene_get_post_timing(exr[0], which, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


# ----------------------------------------------------------------------- driver and command line
def test_driver_switch_and_cpu_tensors_take_the_host_path(product_lib, tmp_path, capsys):
    import torch
    from rgk_amd import render_driver as rd
    from rgk_amd.__main__ import main

    class Cfg:
        xres, yres, render_rounds, render_minutes = 5, 3, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: capi.Params())
    assert rd.RenderDriver(None, Cfg, None, device="cpu").device_output is True
    assert rd.RenderDriver(None, Cfg, None, device="cpu", device_output=False).device_output is False

    class FakeScene:  # a scene object is not enough: the tensors must live on its GPU
        device = 0
    img = torch.arange(45, dtype=torch.float32).reshape(3, 5, 3) / 7
    assert not rd.on_scene_gpu(FakeScene(), img) and not rd.on_scene_gpu(None, img)
    a, b = tmp_path / "a.exr", tmp_path / "b.exr"
    rd.write_exr_image(a, img, 0.5, FakeScene())
    rd.write_exr(b, (img * 0.5).numpy())
    assert a.read_bytes() == b.read_bytes()
    ob = rd.EXRTexture(5, 3, "cpu")
    ob.data.copy_(img)
    ob.count.fill_(2)
    val = ob.write(tmp_path / "c.exr", -1.0, FakeScene())
    assert val == ob.write(tmp_path / "d.exr", -1.0) and (tmp_path / "c.exr").read_bytes() == (tmp_path / "d.exr").read_bytes()
    rgba = torch.arange(60, dtype=torch.uint8).reshape(3, 5, 4)
    rd.write_png_image(tmp_path / "a.png", rgba, FakeScene())
    rd.write_png(tmp_path / "b.png", rgba)
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    cfg = str(tmp_path / "absent.json")
    assert main([cfg, "-q", "--host-output", "--png"]) == 1 and "Failed to load config file" in capsys.readouterr().out  # accepted: it got as far as the file
    from rgk_amd import __main__ as M
    assert "--host-output" in M.__doc__
