"""The display stage on the GPU: rgk_display_measure_device and rgk_display_encode_device against the numpy restatement
(tests/display_ref.py), every histogram count, every solved float and every RGBA word on the bits, no pixel left out; then the
driver entry on a real accumulator, the reuse of an exposure, a call between two rounds, the timing slots and the command line.

Planes are made in numpy and uploaded (tests/display_cases.py says which, and why 1183 x 889 and a shifted 640 x 480 are among
them); the scene is the small Cornell fixture and only lends its handle."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi

import display_cases as DC
import display_ref as D
import memstate_ref as M
from conftest import ROOT, record_parity
from test_display_cpu import decode_png

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1
FATAL_STATUS = (134, 139, 124, 137)  # abort, segmentation fault, a time limit's two ways out
CHILD_TIMEOUT = 300


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


@pytest.fixture(scope="module")
def bit_runs(rd):
    """The bit cases, run once in this process on fresh memory.  Never changed afterwards."""
    assert "RGK_POISON" not in os.environ
    images, results, thresholds, g, poisoned = DC.run_bit_cases(rd)
    for res in list(results.values()) + [thresholds]:
        for a in res.values():
            a.setflags(write=False)
    assert poisoned == [0, 0]
    return images, results, thresholds, g, rd.display_table()


def differing(a, b):
    return int((M.bits(a) != M.bits(b)).sum())


CASES = [(name, counted, mode) for name, variants in DC.VARIANTS.items() for counted, mode in variants]


# ----------------------------------------------------------------------- bits
@pytest.mark.parametrize("name,counted,mode", CASES)
def test_histogram_solve_and_every_word_equal_the_restatement(bit_runs, name, counted, mode):
    """hist, n_lit, n_dark, the four solved floats, and the words of all three operators encoded with those stats."""
    images, results, _, _, T = bit_runs
    img, got = images[name], results[name]
    key = f"{int(counted)}|{mode}::"
    cnt = img.cnt if counted else None
    hist, dark = D.measure(img.rgb, cnt)
    assert np.array_equal(got[key + "hist"], hist)
    assert got[key + "counts"].tolist() == [int(hist.sum()), dark] and int(hist.sum()) + dark == img.W * img.H
    bad_words = 0
    for op in DC.OPS:
        p = DC.params_of(op, mode)
        st = D.solve(hist, dark, exposure=p.exposure, key=p.key, white_permille=p.white_permille, white=p.white)
        want = np.array([st[k] for k in ("y_median", "y_white", "exposure", "white")], F)
        assert differing(got[key + "floats"], want) == 0, (got[key + "floats"], want)
        words = D.encode(img.rgb, cnt, D.OPS[op], st["exposure"], st["white"], T)
        assert not (got[key + op] == DC.PREFILL).any(), "a pixel was never written"
        d = differing(got[key + op], words)
        print(f"display bits [{name}, counted {counted}, {mode}, {op}]: {d} of {words.size} words differ; exposure {st['exposure']:.6g} white {st['white']:.6g}")
        bad_words += d
    record_parity(f"gpu_display.bits[{name}, counted {int(counted)}, {mode}]", pixels=img.W * img.H, lit=int(hist.sum()), dark=dark, words_differing=bad_words)
    assert bad_words == 0


def test_the_cases_reach_every_branch(bit_runs):
    images, results, _, _, T = bit_runs
    z = images["zoo 67x45"]
    assert np.isnan(z.rgb).any() and np.isinf(z.rgb).any() and (z.rgb < 0).any() and (z.cnt == 0).any() and (D.colour(z.rgb, z.cnt) == F(1e-30)).any()
    hist = results["zoo 67x45"]["1|auto::hist"]
    assert hist[0] > 0 and hist[255] > 0 and (hist[1:255] > 0).all()  # below 2^-20, above 2^12, and every bin between: the edge pixels
    Y = D.lum(D.colour(z.rgb, z.cnt)).reshape(-1)
    e = np.array([D.edge(b) for b in range(257)], F)
    at_edge = np.isin(Y, e).sum()
    assert at_edge >= 257 and np.isin(Y, D._next(e, -1)).sum() >= 257 and np.isin(Y, D._next(e, 1)).sum() >= 257  # the searched edge pixels, both sides
    c = results["constant 67x45"]["1|auto::hist"]
    assert (c > 0).sum() == 1 and c.max() == 67 * 45
    b = results["black 67x45"]
    assert b["1|auto::hist"].sum() == 0 and b["1|auto::counts"].tolist() == [0, 67 * 45] and b["1|auto::floats"].tolist() == [0, 0, 1, 1]
    assert (b["1|auto::filmic"] == 0xFF000000).all() and b["1|fixed::floats"].tolist() == [0, 0, 0.5, 2.0]
    for name in ("zoo 96x96", "zoo 640x480"):
        for op in DC.OPS:
            red = results[name]["1|auto::" + op] & 0xFF
            assert red.min() == 0 and red.max() == 255, (name, op)
    assert images["zoo 1183x889"].W * images["zoo 1183x889"].H > 1024 * 256 * 4 and images["zoo 640x480"].W * images["zoo 640x480"].H > 1024 * 256
    assert differing(results["zoo 640x480 unaligned"]["1|auto::filmic"], results["zoo 640x480"]["1|auto::filmic"]) == 0


@pytest.mark.parametrize("op", DC.OPS)
def test_values_on_the_byte_thresholds_and_the_float_below(bit_runs, op):
    """Per byte k, inputs the restatement searched for: the smallest channel value whose curve output reaches T[k] and the float
    just below it, as grey pixels and as the red of coloured ones, encoded with hand-filled stats; with and without counts."""
    _, _, thresholds, _, T = bit_runs
    px = DC.threshold_image(op, T)
    v = D.curve(D.OPS[op], D.colour(px), DC.HAND["exposure"], DC.HAND["white"])[..., 0].reshape(4, 255)
    on, below = int((v[[1, 3]] == T[1:]).sum()), int((v[[0, 2]] == D._next(T[1:], -1)).sum())
    print(f"display thresholds [{op}]: {on} of 510 outputs exactly on T[k], {below} exactly one float below")
    assert on >= 64  # (the curve's own rounding decides how many land exactly; the pairs below straddle every threshold regardless)
    want = D.encode(px, None, D.OPS[op], DC.HAND["exposure"], DC.HAND["white"], T)
    red = (want & 0xFF).reshape(4, 255)
    reach = px.reshape(4, 255, 3)[1, :, 0] < np.finfo(F).max
    k = np.arange(1, 256)
    assert reach.sum() >= 250 and np.array_equal(red[1][reach], k[reach]) and np.array_equal(red[0][reach], k[reach] - 1)
    for plane in ("mean", "counted"):
        got = thresholds[f"{op}|{plane}"]
        assert not (got == DC.PREFILL).any()
        assert differing(got, want) == 0, (op, plane)
    record_parity(f"gpu_display.thresholds[{op}]", on_threshold=on, one_below=below, words_differing=0)


def test_refusals_leave_the_output_alone_and_the_timing_slots(bit_runs):
    import torch
    images, results, _, g, _ = bit_runs
    img = images["zoo 67x45"]
    rgb, cnt = M.up(img.rgb), M.up(img.cnt)
    out = torch.full((img.H, img.W), 0x7B7B7B7B, dtype=torch.int32, device="cuda:0")
    p, st = capi.DisplayParams(), capi.DisplayStats()
    st.exposure, st.white = 1.0, 1.0
    bad_p, bad_st = capi.DisplayParams(op=7), capi.DisplayStats()
    torch.cuda.synchronize()

    def encode(params=p, stats=st, o=None, xres=img.W):
        return g.lib.rgk_display_encode_device(g.h, xres, img.H, rgb.data_ptr(), cnt.data_ptr(), C.byref(params), C.byref(stats), o or out.data_ptr())
    for rc in (encode(params=bad_p), encode(stats=bad_st), encode(o=rgb.data_ptr()), encode(xres=0)):
        assert rc == INVALID and g.lib.rgk_last_error()
        torch.cuda.synchronize()
        assert bool((out == 0x7B7B7B7B).all())
    assert g.lib.rgk_display_measure_device(g.h, img.W, img.H, rgb.data_ptr(), cnt.data_ptr(), C.byref(bad_p), C.byref(st)) == INVALID
    g.set_tuning(time_post=1)
    try:
        s1 = g.display_measure_device(img.W, img.H, rgb.data_ptr(), cnt.data_ptr(), p)
        assert encode(stats=s1) == 0
        t10, t11 = g.post_timing(10), g.post_timing(11)
        assert len(t10) == 2 and t10[1] > 0 and len(t11) == 1 and t11[0] > 0  # {clear, k_display_hist}, {k_display_encode}
        record_parity("gpu_display.timing[zoo 67x45]", clear_ms=t10[0], hist_ms=t10[1], encode_ms=t11[0])
    finally:
        g.set_tuning(time_post=0)
    g.display_measure_device(img.W, img.H, rgb.data_ptr(), cnt.data_ptr(), p)
    assert encode(stats=s1) == 0 and g.post_timing(10) == [] and g.post_timing(11) == []
    torch.cuda.synchronize()
    assert differing(out.cpu().numpy(), results["zoo 67x45"]["1|auto::filmic"]) == 0


# ----------------------------------------------------------------------- the driver
class CornellFrame:
    """Cornell at 96 x 96, 4 spp: the scene, a driver configuration and the camera."""

    def __init__(self, rd):
        from rgk_amd.workloads import Workload
        wl = Workload("cornell-256", scale=0.375, spp=4)
        assert (wl.xres, wl.yres) == (96, 96)
        prm = wl.params()

        class Cfg:
            xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, 1, None
            get_params = staticmethod(lambda sampler=0, flags=0: prm)
        self.wl, self.cfg, self.camera = wl, Cfg, wl.camera
        self.scene = rd.Scene(wl.builder)

    def driver(self, rd):
        return rd.RenderDriver(self.scene, self.cfg, self.camera)


@pytest.fixture(scope="module")
def cornell_frame(rd):
    return CornellFrame(rd)


def stats_floats(st):
    return np.array([st.y_median, st.y_white, st.exposure, st.white], F)


def ref_of_stats(hist, dark, p):
    st = D.solve(hist, dark, exposure=p.exposure, key=p.key, white_permille=p.white_permille, white=p.white)
    return st, np.array([st[k] for k in ("y_median", "y_white", "exposure", "white")], F)


def test_real_accumulator_through_the_driver_and_stats_reuse(rd, cornell_frame, bit_runs):
    """RenderDriver.display() of a rendered accumulator equals the restatement on the accumulator's host copy; the stats it returns,
    handed to display(image=denoise()), give the restatement's words for the denoised image with the ACCUMULATOR's exposure."""
    T = bit_runs[4]
    drv = cornell_frame.driver(rd)
    drv.render_round()
    acc, cnt = drv.total_ob.data.cpu().numpy(), drv.total_ob.count.cpu().numpy().view(np.uint32)
    hist, dark = D.measure(acc, cnt)
    for op in DC.OPS:
        p = capi.DisplayParams(op=capi.DISPLAY_OPS[op])
        rgba, st = drv.display(params=p)
        assert rgba.shape == (96, 96, 4) and str(rgba.dtype) == "torch.uint8"
        want_st, want_f = ref_of_stats(hist, dark, p)
        assert np.array_equal(np.frombuffer(st.hist, np.uint32), hist) and (st.n_lit, st.n_dark) == (int(hist.sum()), dark)
        assert differing(stats_floats(st), want_f) == 0
        want = D.rgba_bytes(D.encode(acc, cnt, D.OPS[op], want_st["exposure"], want_st["white"], T))
        got = rgba.cpu().numpy()
        assert np.array_equal(got, want), op
        share = float(((got[..., :3] == 0) | (got[..., :3] == 255)).all(-1).mean())
        print(f"display cornell 96x96 [{op}]: exposure {st.exposure:.5g} white {st.white:.5g}; pixels 0 or 255 in every channel {share:.4f}")
        record_parity(f"gpu_display.cornell[{op}]", exposure=float(st.exposure), white=float(st.white), clipped_share=share)
        assert share < 0.25  # a picture, not a black or a white frame
        den = drv.denoise()
        again, st2 = drv.display(image=den, params=p, stats=st)
        assert st2 is st
        want = D.rgba_bytes(D.encode(den.cpu().numpy(), None, D.OPS[op], want_st["exposure"], want_st["white"], T))
        assert np.array_equal(again.cpu().numpy(), want), op
        own, st3 = drv.display(image=den, params=p)  # measured on the image itself: other stats, not the accumulator's
        h2, d2 = D.measure(den.cpu().numpy())
        assert np.array_equal(np.frombuffer(st3.hist, np.uint32), h2) and differing(stats_floats(st3), ref_of_stats(h2, d2, p)[1]) == 0
    with pytest.raises(ValueError):
        drv.display(image=den.cpu())


def test_a_call_between_two_rounds_changes_neither(rd, cornell_frame):
    def two_rounds(between):
        drv = cornell_frame.driver(rd)
        drv.render_round()
        first = drv.total_ob.data.cpu().numpy().copy()
        if between:
            drv.display()
            drv.display(image=drv.total_ob.get_pixels(), params=capi.DisplayParams(op=capi.DISPLAY_REINHARD))
        drv.render_round()
        return first, drv.total_ob.data.cpu().numpy(), drv.total_ob.count.cpu().numpy(), [c.path_rays for c in drv.counters]
    a, b = two_rounds(False), two_rounds(True)
    assert differing(a[0], b[0]) == 0 and differing(a[1], b[1]) == 0 and np.array_equal(a[2], b[2]) and (a[2] == 8).all() and a[3] == b[3]


# ----------------------------------------------------------------------- the command line
SCENE = '''{
    "output-file": "t.exr", "output-width": 50, "output-height": 42, "multisample": 8, "rounds": 2, "recursion-max": 3, "clamp": 20,
    "camera": {"position": [0,1.2,5], "lookat": [0,0.8,0], "fov": 35},
    "materials": [{"name": "m", "brdf": "diffuse", "diffuse255": [255, 128, 0]},
                  {"name": "g", "brdf": "diffuse", "diffuse": [0.4,0.4,0.5]},
                  {"name": "l", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5], "emission": [9,9,8]}],
    "scene": [{"primitive": "cube", "material": "m", "translate": [0,0.5,0]},
              {"primitive": "plane", "material": "g", "scale": [4,1,4]},
              {"primitive": "plane", "material": "l", "scale": [0.5,1,0.5], "translate": [0,3,0], "rotate": [180, 0, 0]}],
    "sky": {"color": [0.3, 0.4, 0.6], "intensity": 0.5}
}'''


def run_cli(args, cwd, env):
    try:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, "-m", "rgk_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT + 30)
    except subprocess.TimeoutExpired:
        pytest.exit(f"the command-line child did not finish in {CHILD_TIMEOUT} s: nothing else may start on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode in FATAL_STATUS:
        pytest.exit(f"the command-line child ended with status {r.returncode}: nothing else may start on the GPU\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", returncode=3)
    return r


def test_cli_writes_three_pictures_with_one_exposure_and_changes_no_exr(rd, tmp_path, bit_runs):
    """-p --denoise --upsample --png on a 50 x 42 configuration (12 x 10 after -p): three PNGs beside the three EXRs, each what
    display() gives for that image with the exposure measured on the accumulator -- which the command line reports -- and every
    .exr byte-identical to the run without --png."""
    from rgk_amd.config import load_config
    T = bit_runs[4]
    cfg_path = tmp_path / "s.json"
    cfg_path.write_text(SCENE)
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir(); b.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    common = ["-p", "--denoise", "--upsample"]
    with_png = run_cli([str(cfg_path), "-D", str(a)] + common + ["--png"], str(tmp_path), env)
    assert with_png.returncode == 0, with_png.stderr + with_png.stdout
    without = run_cli([str(cfg_path), "-D", str(b)] + common, str(tmp_path), env)
    assert without.returncode == 0, without.stderr + without.stdout
    exrs = ["t.preview.denoised.exr", "t.preview.exr", "t.preview.upsampled.exr"]
    pngs = ["t.preview.denoised.png", "t.preview.png", "t.preview.upsampled.png"]
    assert sorted(os.listdir(str(b))) == exrs and sorted(os.listdir(str(a))) == sorted(exrs + pngs)
    for n in exrs:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert "Display:" not in without.stdout
    m = re.search(r"Display: exposure (\S+) white (\S+) \(median luminance (\S+), (\d+) lit and (\d+) black pixels\)", with_png.stdout)
    assert m, with_png.stdout
    # the same through the Python entry: the configuration's camera at both sizes, two rounds of the halved samples
    cfg = load_config(str(cfg_path))
    full_cam = cfg.get_camera(0.0)
    cfg.xres, cfg.yres, cfg.multisample = cfg.xres // 4, cfg.yres // 4, max(1, cfg.multisample // 2)
    g = rd.Scene(cfg.build_scene().to_desc())
    drv = rd.RenderDriver(g, cfg, cfg.get_camera(0.0))
    drv.render_round()
    drv.render_round()
    p = capi.DisplayParams()
    rgba, st = drv.display(params=p)
    assert (F(m.group(1)), F(m.group(2)), F(m.group(3))) == (F(st.exposure), F(st.white), F(st.y_median)) and (int(m.group(4)), int(m.group(5))) == (st.n_lit, st.n_dark)
    images = {"t.preview.png": (None, (10, 12)), "t.preview.denoised.png": (drv.denoise(), (10, 12)),
              "t.preview.upsampled.png": (drv.upsample(full_cam, 50, 42, denoise=True)[0], (42, 50))}
    for n, (image, shape) in images.items():
        got = decode_png((a / n).read_bytes())
        assert got.shape == shape + (3,), n
        want, used = drv.display(image=image, params=p, stats=st)
        assert used is st and np.array_equal(got, want.cpu().numpy()[..., :3]), n
        if image is not None:  # and that is the restatement with the ACCUMULATOR's exposure and white
            ref = D.rgba_bytes(D.encode(image.cpu().numpy(), None, D.FILMIC, F(st.exposure), F(st.white), T))
            assert np.array_equal(got, ref[..., :3]), n
    # a fixed exposure is taken as given: 2^-1
    c = tmp_path / "fixed"
    c.mkdir()
    r = run_cli([str(cfg_path), "-D", str(c), "-p", "--png=linear", "--exposure", "-1"], str(tmp_path), env)
    assert r.returncode == 0 and "Display: exposure 0.5 white" in r.stdout, r.stderr + r.stdout
    assert (c / "t.preview.exr").read_bytes() == (a / "t.preview.exr").read_bytes()
    p = capi.DisplayParams(op=capi.DISPLAY_LINEAR, exposure=0.5)
    assert np.array_equal(decode_png((c / "t.preview.png").read_bytes()), drv.display(params=p)[0].cpu().numpy()[..., :3])
