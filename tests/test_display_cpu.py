"""The display stage, the part that needs no GPU: the functions the two kernels call, the solve and the PNG writer under ASan + UBSan
in a stand-alone program (tests/cpp/display_main.cpp); the table, the solve and the writer through the library's C ABI against the
numpy restatement (tests/display_ref.py) and the standard library's zlib; the ABI, the argument errors and the command line's
refusals."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from rgk_amd import capi

import display_ref as D
from conftest import ROOT

F = np.float32
INVALID = -1
CPP = os.path.join(ROOT, "tests", "cpp")
HARNESS_CASES = ["colour", "solve", "byte", "checksums", "png"]


# ----------------------------------------------------------------------- the sanitized harness
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("display") / "display_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "display_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("case", HARNESS_CASES)
def test_display_unit_on_the_cpu(harness, case, tmp_path):
    """Known answers, written out by hand: colour, luminance and bins at their edges; the solve on one pixel, one bin, bin 0, bin 255,
    two equal halves, nothing lit, fixed exposure and white; the byte at every T[k] and the float below it; CRC-32 of "IEND" and
    Adler-32 of "Wikipedia"; a PNG of 1 x 1 byte for byte, one of 21845 x 1 whose row crosses a stored block, an unwritable path.
    That the program links without the HIP runtime is the check that the unit calls nothing of it."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([harness, case, str(tmp_path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout


# ----------------------------------------------------------------------- the table and the solve through the library
def test_table_is_increasing_and_the_double_formula_to_one_ulp(product_lib):
    from rgk_amd import render_driver as rd
    T = rd.display_table()
    assert T.dtype == F and T.shape == (256,) and T[0] == 0
    assert (np.diff(T.astype(np.float64)) > 0).all()
    want = D.table()
    ulp = np.spacing(want.astype(F)).astype(np.float64)
    assert (np.abs(T.astype(np.float64) - want)[1:] <= ulp[1:]).all()
    assert np.array_equal(T, rd.display_table())  # the same storage every time
    # the thresholds are where the rounded sRGB byte of the textbook encoding changes
    v = np.linspace(0, 1, 4097).astype(F)
    srgb = np.where(v <= 0.0031308, v.astype(np.float64) * 12.92, 1.055 * v.astype(np.float64) ** (1 / 2.4) - 0.055)
    textbook = np.floor(srgb * 255 + 0.5).astype(np.int64)
    assert np.abs(D.byte_of(T, v).astype(np.int64) - textbook).max() <= 1  # (<= 1: only at a threshold's own rounding)
    assert (D.byte_of(T, v).astype(np.int64) != textbook).mean() < 0.01


def random_histograms(rng):
    yield np.zeros(256, np.uint32)
    for _ in range(200):
        h = np.zeros(256, np.uint32)
        k = int(rng.integers(1, 40))
        h[rng.integers(0, 256, k)] = rng.integers(1, 10 ** int(rng.integers(1, 8)), k).astype(np.uint32)
        yield h
    for _ in range(50):
        yield rng.integers(0, 3, 256).astype(np.uint32)
    h = np.zeros(256, np.uint32)
    h[7], h[250] = 0xFFFFFFF0, 0xF  # the largest total that fits
    yield h


def test_solve_equals_the_restatement_on_the_bits(product_lib):
    from rgk_amd import render_driver as rd
    rng = np.random.default_rng(11)
    n = 0
    for h in random_histograms(rng):
        for kw in (dict(), dict(white_permille=500), dict(white_permille=1), dict(white_permille=1000, key=0.5), dict(exposure=0.37), dict(white=2.5),
                   dict(exposure=3.0, white=0.7)):
            p = capi.DisplayParams(op=capi.DISPLAY_REINHARD, **kw)
            st = rd.display_solve(h, 3, p)
            want = D.solve(h, 3, **kw)
            assert np.array_equal(np.frombuffer(st.hist, np.uint32), h) and st.n_lit == want["n_lit"] and st.n_dark == 3
            got = np.array([st.y_median, st.y_white, st.exposure, st.white], F)
            ref = np.array([want[k] for k in ("y_median", "y_white", "exposure", "white")], F)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (h.nonzero(), kw, got, ref)
            n += 1
    assert n > 1500


def test_solve_refuses_bad_arguments(product_lib):
    lib = product_lib
    h = np.ones(256, np.uint32)
    st, p = capi.DisplayStats(), capi.DisplayParams()
    assert lib.rgk_display_solve(h.ctypes.data, 0, C.byref(p), C.byref(st)) == 0
    assert lib.rgk_display_solve(None, 0, C.byref(p), C.byref(st)) == INVALID and b"null" in lib.rgk_last_error()
    assert lib.rgk_display_solve(h.ctypes.data, 0, None, C.byref(st)) == INVALID
    assert lib.rgk_display_solve(h.ctypes.data, 0, C.byref(p), None) == INVALID
    big = np.full(256, 0x80000000, np.uint32)
    assert lib.rgk_display_solve(big.ctypes.data, 0, C.byref(p), C.byref(st)) == INVALID and b"32 bits" in lib.rgk_last_error()
    for field, value in BAD_PARAMS:
        bad = capi.DisplayParams()
        setattr(bad, field, value)
        assert lib.rgk_display_solve(h.ctypes.data, 0, C.byref(bad), C.byref(st)) == INVALID and b"display parameters" in lib.rgk_last_error(), (field, value)


BAD_PARAMS = [("op", 3), ("op", 0xFFFFFFFF), ("exposure", float("nan")), ("exposure", float("inf")), ("white", float("-inf")), ("white", float("nan")),
              ("key", 0.0), ("key", -0.18), ("key", float("nan")), ("key", float("inf")), ("white_permille", 0), ("white_permille", 1001)]


# ----------------------------------------------------------------------- ABI
def test_abi_struct_sizes_symbols_and_shipped_defaults(product_lib, tmp_path):
    src = tmp_path / "sz.c"
    pf = [f for f, _ in capi.DisplayParams._fields_]
    sf = [f for f, _ in capi.DisplayStats._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgk.h"\nint main(void){printf("%zu %zu", sizeof(rgk_display_params), sizeof(rgk_display_stats));'
                   + "".join(f'printf(" %zu", offsetof(rgk_display_params, {f}));' for f in pf)
                   + "".join(f'printf(" %zu", offsetof(rgk_display_stats, {f}));' for f in sf)
                   + 'printf(" %d %d %d", RGK_DISPLAY_LINEAR, RGK_DISPLAY_REINHARD, RGK_DISPLAY_FILMIC); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, S = capi.DisplayParams, capi.DisplayStats
    assert got == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in pf] + [getattr(S, f).offset for f in sf] + [
        capi.DISPLAY_LINEAR, capi.DISPLAY_REINHARD, capi.DISPLAY_FILMIC]
    assert C.sizeof(P) == 20 and C.sizeof(S) == 4 * 256 + 8 + 16
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    assert set(re.findall(r"\b(rgk_[a-z_]+)\s*\(", hdr)) == set(capi.EXPORTS)
    for name, n_args in (("rgk_display_table", 0), ("rgk_display_solve", 4), ("rgk_display_measure_device", 7), ("rgk_display_encode_device", 8),
                         ("rgk_output_write_png", 4)):
        assert name in capi.EXPORTS and getattr(product_lib, name) is not None
        proto = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",") if a.strip() != "void"]
        assert len(args) == len(getattr(product_lib, name).argtypes) == n_args, name
    d = capi.DisplayParams().check()
    assert (d.op, d.exposure, round(d.key, 6), d.white_permille, d.white) == (capi.DISPLAY_FILMIC, 0.0, 0.18, 995, 0.0)  # the shipped values
    assert capi.DISPLAY_OPS == D.OPS


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_each_refused_parameter_is_refused_by_the_wrapper_and_by_both_entries(product_lib, field, value):
    bad = capi.DisplayParams()
    setattr(bad, field, value)
    with pytest.raises(ValueError):
        bad.check()
    m, e = _good_calls()
    m[5] = e[5] = C.byref(bad)
    assert product_lib.rgk_display_measure_device(*m) == INVALID and b"display parameters" in product_lib.rgk_last_error()
    assert product_lib.rgk_display_encode_device(*e) == INVALID and b"display parameters" in product_lib.rgk_last_error()


_KEEP = []


def _good_calls():
    """Argument lists both entries would accept, on a `scene` that is 64 bytes of nothing: every refusal below is reported before
    the scene or a device is touched."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    bufs = [np.zeros(8 * 8 * 3, np.float32) for _ in range(3)]
    p, st = capi.DisplayParams(), capi.DisplayStats()
    st.exposure, st.white = 1.0, 1.0
    _KEEP.append((fake, bufs, p, st))
    a = [b.ctypes.data for b in bufs]
    #          0      1  2  3     4     5           6
    measure = [scene, 8, 8, a[0], a[1], C.byref(p), C.byref(st)]
    #         0      1  2  3     4     5           6            7
    encode = [scene, 8, 8, a[0], a[1], C.byref(p), C.byref(st), a[2]]
    return measure, encode


def test_argument_errors_need_no_gpu(product_lib):
    lib = product_lib
    for fn, good, pointers in ((lib.rgk_display_measure_device, _good_calls()[0], (0, 3, 5, 6)), (lib.rgk_display_encode_device, _good_calls()[1], (0, 3, 5, 6, 7))):
        for k in pointers:  # every pointer but the count plane is needed
            a = list(good)
            a[k] = None
            assert fn(*a) == INVALID and b"null" in lib.rgk_last_error(), k
        for k, v in ((1, 0), (2, 0), (1, 65536), (2, 70000)):
            a = list(good)
            a[k] = v
            assert fn(*a) == INVALID and b"resolution" in lib.rgk_last_error(), (k, v)
    _, good = _good_calls()
    for i in (3, 4):  # the output on top of an input
        a = list(good)
        a[7] = a[i]
        assert lib.rgk_display_encode_device(*a) == INVALID and b"output" in lib.rgk_last_error(), i
    for field, value in (("exposure", 0.0), ("exposure", -1.0), ("exposure", float("inf")), ("exposure", float("nan")), ("white", 0.0), ("white", float("nan"))):
        st = capi.DisplayStats()
        st.exposure, st.white = 1.0, 1.0
        setattr(st, field, value)
        a = list(good)
        a[6] = C.byref(st)
        assert lib.rgk_display_encode_device(*a) == INVALID and b"display stats" in lib.rgk_last_error(), (field, value)
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(good[0], 12, None, C.byref(n)) == INVALID
    for which in (10, 11):
        assert lib.rgk_scene_get_post_timing(good[0], which, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


# ----------------------------------------------------------------------- the PNG container, decoded with the standard library alone
def decode_png(data):
    """-> (height, width, 3) uint8.  Nothing is skipped: the signature, every chunk's CRC (zlib.crc32), the header's fields, the
    zlib stream (zlib.decompress, which checks the Adler-32), every row's filter byte."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack_from(">I", data, pos)
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack_from(">I", data, pos + 8 + n)
        assert zlib.crc32(kind + body) == crc, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == h * (1 + 3 * w)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize("size", [(1, 1), (67, 45), (300, 317)])
def test_png_decodes_to_the_array_with_the_standard_library_and_with_pil(product_lib, tmp_path, size):
    """300 x 317 is 285,617 raw bytes: five stored blocks, the last one short."""
    from PIL import Image
    from rgk_amd import render_driver as rd
    w, h = size
    rgba = np.random.default_rng(w).integers(0, 256, (h, w, 4), dtype=np.uint8)
    path = tmp_path / "p.png"
    rd.write_png(path, rgba)
    data = path.read_bytes()
    raw_bytes = h * (1 + 3 * w)
    assert len(data) == 8 + 25 + 12 + (2 + 5 * -(-raw_bytes // 65535) + raw_bytes + 4) + 12
    assert np.array_equal(decode_png(data), rgba[..., :3])
    with Image.open(str(path)) as im:
        assert im.mode == "RGB" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), rgba[..., :3])


def test_png_writer_refusals(product_lib, tmp_path):
    from rgk_amd import render_driver as rd
    one = np.zeros((1, 1, 4), np.uint8)
    with pytest.raises(capi.RgkError, match="cannot open"):
        rd.write_png(tmp_path / "absent" / "p.png", one)
    with pytest.raises(ValueError):
        rd.write_png(tmp_path / "p.png", np.zeros((2, 2, 3), np.uint8))
    assert product_lib.rgk_output_write_png(None, 1, 1, one.ctypes.data) == INVALID
    assert product_lib.rgk_output_write_png(str(tmp_path / "p.png").encode(), 0, 1, one.ctypes.data) == INVALID
    assert rd.png_beside("a/b/t.preview.denoised.exr") == "a/b/t.preview.denoised.png"


# ----------------------------------------------------------------------- what the restatement means
def test_restatement_known_answers():
    """A grey card at the median comes out as the sRGB byte of the key; the searched threshold inputs sit on the byte's edge."""
    T = D.table().astype(F)
    rgb = np.full((4, 4, 3), 0.5, F)
    hist, dark = D.measure(rgb)
    assert dark == 0 and hist.sum() == 16 and hist[D.bin_of(D.lum(rgb))[0, 0]] == 16
    st = D.solve(hist, dark)
    words = D.encode(rgb, None, D.LINEAR, st["exposure"], st["white"], T)
    grey = D.rgba_bytes(words)[0, 0]
    assert grey[3] == 255 and abs(int(grey[0]) - 118) <= 8 and grey[0] == grey[1] == grey[2]  # 0.18 -> 118; the median is read to 1/8 octave
    black = np.zeros((2, 2, 3), F)
    hist, dark = D.measure(black)
    assert hist.sum() == 0 and dark == 4 and D.solve(hist, dark)["exposure"] == 1 and D.solve(hist, dark)["white"] == 1
    assert (D.encode(black, None, D.FILMIC, 1, 1, T) == 0xFF000000).all()
    for op in (D.LINEAR, D.REINHARD, D.FILMIC):
        for others in (None, (0.25, 0.125)):
            c = D.threshold_inputs(op, 0.7391, 3.3, T, others)
            reach = c[:, 1] < np.finfo(F).max
            assert reach.sum() >= 250, (op, reach.sum())
            px = np.zeros((255, 2, 3), F)
            px[..., 0] = c
            px[..., 1] = c if others is None else others[0]
            px[..., 2] = c if others is None else others[1]
            red = D.encode(px, None, op, 0.7391, 3.3, T) & 0xFF
            k = np.arange(1, 256)
            assert np.array_equal(red[reach, 1], k[reach]) and np.array_equal(red[reach, 0], k[reach] - 1), op


# ----------------------------------------------------------------------- driver and command line
def test_driver_and_cli_refusals(tmp_path, capsys):
    from rgk_amd import render_driver as rd
    from rgk_amd.__main__ import main

    class Cfg:
        xres, yres, render_rounds, render_minutes = 8, 8, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: capi.Params())
    drv = rd.RenderDriver(None, Cfg, None, device="cpu")
    assert drv.display_stats is None
    with pytest.raises(ValueError, match="output_file"):
        drv.render_frame(rounds=0, display=capi.DisplayParams())
    with pytest.raises(ValueError, match="white_permille"):
        drv.render_frame(rounds=0, output_file=str(tmp_path / "o.exr"), display=capi.DisplayParams(white_permille=0))
    with pytest.raises(ValueError, match="key"):
        drv.display(params=capi.DisplayParams(key=0.0))
    drv.render_frame(rounds=0, output_file=str(tmp_path / "o.exr"), display=capi.DisplayParams())  # no round: nothing written, nothing asked of a GPU
    assert os.listdir(str(tmp_path)) == []
    cfg = str(tmp_path / "absent.json")  # refused before the file is looked at
    assert main([cfg, "--png", "-d", "1", "1"]) == 1
    assert "ERROR: --png cannot be combined with -d." in capsys.readouterr().out
    assert main([cfg, "--exposure", "1"]) == 1
    assert "ERROR: --exposure needs --png." in capsys.readouterr().out
    for ev in ("101", "-200", "nan", "inf"):
        assert main([cfg, "--png", "--exposure", ev]) == 1
        assert "ERROR: Invalid argument for --exposure" in capsys.readouterr().out
    for extra in (["--png"], ["--png", "linear"], ["--png=reinhard", "--exposure", "-2.5"], ["-p", "--denoise", "--upsample", "--png", "filmic"]):
        assert main([cfg, "-q"] + extra) == 1 and "Failed to load config file" in capsys.readouterr().out  # accepted: it got as far as the file
    with pytest.raises(SystemExit):
        main([cfg, "--png", "aces"])
    capsys.readouterr()
