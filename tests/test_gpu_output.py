"""GPU suite (-m gpu): EXR and PNG files assembled on the device (rgk_output_write_exr_device, rgk_output_write_png_device) are byte
for byte the files the host writers produce from host copies -- rgk_output_normalize + rgk_output_write_exr, rgk_output_write_png --
which stay the reference on every comparison; the PNGs also decode, with the standard library alone, back to their input.  Every
bar is equality of bytes: no tolerance anywhere.  The cases are tests/output_cases.py's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from rgk_amd import capi

import memstate_ref as M
import output_cases as OC
from conftest import ROOT, record_parity
from test_display_cpu import decode_png
from test_gpu_display import SCENE, rd, run_cli  # noqa: F401  (rd: the fixture)

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1


@pytest.fixture(scope="module")
def runs(rd, tmp_path_factory):  # noqa: F811
    """Every device case, run once in this process on fresh memory, and the same files through the host writers.  Never changed."""
    assert "RGK_POISON" not in os.environ
    tmp = tmp_path_factory.mktemp("output")
    got, scene, (exrs, pngs), poisoned = OC.run_device_cases(rd, tmp)
    want = {}
    for c in exrs:
        want[f"exr##{c.name}"], want[f"exr##{c.name}##scale"] = OC.host_exr(c, tmp / "h.exr")
    for name, words in pngs:
        want[f"png##{name}"] = OC.host_png(words, tmp / "h.png")
    for a in list(got.values()) + list(want.values()):
        a.setflags(write=False)
    assert poisoned == [0, 0]
    return got, want, scene, exrs, pngs


EXR_NAMES = [c.name for c in OC.exr_cases()] + ["cornell accum auto", "cornell accum fixed", "cornell image scale 1", "cornell image fixed"]
PNG_NAMES = [name for name, _ in OC.png_cases()]


@pytest.mark.parametrize("name", EXR_NAMES)
def test_exr_bytes_and_scale_equal_the_host_path(runs, name):
    got, want, _, exrs, _ = runs
    case = {c.name: c for c in exrs}[name]
    g, w = got[f"exr##{name}"], want[f"exr##{name}"]
    assert g.size == w.size == 331 + 8 * case.H + case.H * (8 + 8 * case.W)
    differing = int((g != w).sum())
    gs, ws = got[f"exr##{name}##scale"], want[f"exr##{name}##scale"]
    record_parity(f"gpu_output.exr[{name}]", bytes=int(g.size), differing=differing, scale=float(gs[0]))
    assert differing == 0, np.flatnonzero(g != w)[:10]
    assert gs.view(np.uint32)[0] == ws.view(np.uint32)[0], (gs, ws)


def test_the_exr_cases_reach_what_they_are_for(runs):
    _, want, _, exrs, _ = runs
    by = {c.name: c for c in exrs}
    assert sorted(by) == sorted(EXR_NAMES)
    assert np.isposinf(want["exr##67x45 no sample anywhere##scale"][0])   # val = inf, every pixel 0
    body = want["exr##67x45 no sample anywhere"][331 + 8 * OC.H:].reshape(OC.H, 8 + 8 * OC.W)[:, 8 + 2 * OC.W:]
    assert not body.any()
    assert any(want[f"exr##{c.name}##scale"][0] == 0.0 for c in exrs if c.name.endswith("auto wild"))   # +inf wins the maximum
    for name in ("cornell accum auto", "boundary set accum auto", "130x5 accum auto", "3x2 accum auto"):
        s = want[f"exr##{name}##scale"][0]
        assert np.isfinite(s) and s > 0, name
    assert {int(n) for c in exrs if c.cnt is not None for n in np.unique(c.cnt)} >= {0, 1, 3, 256, (1 << 24) + 1}
    assert any(np.isnan(c.rgb).any() for c in exrs) and any(np.isneginf(c.rgb).any() for c in exrs) and any((c.rgb.view(np.uint32) == 0x80000000).any() for c in exrs)
    whole = by["boundary set image scale 1"].rgb.view(np.uint32)
    assert np.isin(OC.half_boundary_values().view(np.uint32), whole).all()
    acc, cnt = by["cornell accum auto"].rgb, by["cornell accum auto"].cnt
    assert (cnt == 16).all() and (acc > 0).mean() > 0.5                    # two rounds of 8 samples


@pytest.mark.parametrize("name", PNG_NAMES)
def test_png_bytes_equal_the_host_writer_and_decode_to_the_input(runs, name):
    got, want, _, _, pngs = runs
    words = dict(pngs)[name]
    g, w = got[f"png##{name}"], want[f"png##{name}"]
    differing = int((g != w).sum()) if g.size == w.size else -1
    record_parity(f"gpu_output.png[{name}]", bytes=int(g.size), differing=differing)
    assert differing == 0
    image = decode_png(g.tobytes())
    assert np.array_equal(image, np.ascontiguousarray(words).view(np.uint8).reshape(words.shape + (4,))[..., :3])


def test_the_png_cases_cross_the_blocks_they_name():
    raw = {name: (3 * w.shape[1] + 1) * w.shape[0] for name, w in OC.png_cases()}
    assert raw["150x150 two blocks"] == 67650 and -(-raw["211x211 three blocks"] // 65535) == 3
    kinds = OC.boundary_sizes()
    for kind, (w, h) in kinds.items():
        c = 65535 % (3 * w + 1)
        assert (3 * w + 1) * h > 65536 and (kind == "filter") == (c == 0) and (c == 0 or "RGB"[(c - 1) % 3] == kind)
    assert {(2 + r + 5 * -(-r // 65535)) % 4 for r in raw.values()} == {0, 1, 2, 3}  # every cut of the payload's last dword


# ----------------------------------------------------------------------- the driver and the command line
class Cfg:
    xres, yres, render_rounds, render_minutes = OC.W, OC.H, 2, None


def frame_files(rd, scene, directory, device_output):  # noqa: F811
    g, cam, prm = scene
    Cfg.get_params = staticmethod(lambda sampler=0, flags=0: prm)
    drv = rd.RenderDriver(g, Cfg, cam, device_output=device_output)
    aov = {n: str(directory / f"{n}.exr") for n in ("albedo", "normal", "depth")}
    drv.render_frame(rounds=2, output_file=str(directory / "o.exr"), aov_files=aov, denoised_file=str(directory / "o.denoised.exr"), display=capi.DisplayParams())
    return {n: (directory / n).read_bytes() for n in sorted(os.listdir(str(directory)))}


def test_render_frame_writes_the_same_files_either_way(rd, runs, tmp_path):  # noqa: F811
    scene = runs[2]
    (tmp_path / "dev").mkdir(); (tmp_path / "host").mkdir()
    g = scene[0]
    g.set_tuning(time_post=1)
    try:
        dev = frame_files(rd, scene, tmp_path / "dev", True)
        assert len(g.post_timing(12)) == 2 and len(g.post_timing(13)) == 2   # the device entries ran
        host = frame_files(rd, scene, tmp_path / "host", False)
    finally:
        g.set_tuning(time_post=0)
    assert sorted(dev) == sorted(host) == ["albedo.exr", "depth.exr", "normal.exr", "o.denoised.exr", "o.denoised.png", "o.exr", "o.png"]
    for n in dev:
        assert dev[n] == host[n], n
    record_parity("gpu_output.render_frame", files=len(dev), bytes=sum(len(b) for b in dev.values()))


def test_command_line_writes_the_same_files_with_and_without_host_output(tmp_path):
    cfg_path = tmp_path / "s.json"
    cfg_path.write_text(SCENE)
    a, b = tmp_path / "device", tmp_path / "host"
    a.mkdir(); b.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    common = ["--denoise", "--aov", "--png"]
    dev = run_cli([str(cfg_path), "-D", str(a)] + common, str(tmp_path), env)
    assert dev.returncode == 0, dev.stderr + dev.stdout
    host = run_cli([str(cfg_path), "-D", str(b)] + common + ["--host-output"], str(tmp_path), env)
    assert host.returncode == 0, host.stderr + host.stdout
    names = sorted(os.listdir(str(a)))
    assert names == sorted(os.listdir(str(b))) and sum(n.endswith(".exr") for n in names) >= 5 and sum(n.endswith(".png") for n in names) == 2, names
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n


def test_calls_between_rounds_change_no_bit_of_the_accumulator(rd, runs, tmp_path):  # noqa: F811
    g, cam, prm = runs[2]

    def between(acc, cnt):
        import torch
        torch.cuda.synchronize()
        g.write_exr_device(tmp_path / "b.exr", OC.W, OC.H, acc.data_ptr(), cnt.data_ptr(), -1.0)
        g.write_exr_device(tmp_path / "b.exr", OC.W, OC.H, acc.data_ptr(), None, OC.SCALE)
        words = torch.full((OC.H, OC.W), 0x01020304, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        g.write_png_device(tmp_path / "b.png", OC.W, OC.H, words.data_ptr())
    plain = OC.render_rounds(rd, g, cam, prm)
    called = OC.render_rounds(rd, g, cam, prm, between=between)
    for a, b in zip(plain, called):
        assert int((M.bits(a.cpu().numpy()) != M.bits(b.cpu().numpy())).sum()) == 0
    assert (plain[1] == 16).all() and (tmp_path / "b.png").exists()


# ----------------------------------------------------------------------- refusals and the timing slots
def test_argument_errors_create_no_file_and_the_timing_slots(runs, tmp_path):
    import torch
    g = runs[2][0]
    lib = g.lib
    case = OC.ExrCase("x", *OC.synthetic(65, 3, 1, False), -1.0)
    rgb, cnt = M.up(case.rgb), M.up(case.cnt)
    words = M.up(np.zeros((3, 65), np.uint32))
    torch.cuda.synchronize()
    path = str(tmp_path / "o.bin").encode()
    absent = str(tmp_path / "absent" / "o.bin").encode()

    def exr(scene=g.h, p=path, w=65, h=3, d=rgb.data_ptr(), c=cnt.data_ptr(), s=-1.0):
        return lib.rgk_output_write_exr_device(scene, p, w, h, d, c, s, None)

    def png(scene=g.h, p=path, w=65, h=3, d=words.data_ptr()):
        return lib.rgk_output_write_png_device(scene, p, w, h, d)
    for fn in (exr, png):
        for kw in (dict(scene=None), dict(p=None), dict(d=None), dict(w=0), dict(h=0), dict(w=65536), dict(p=absent)):
            assert fn(**kw) == INVALID and lib.rgk_last_error(), (fn.__name__, kw)
    assert b"cannot open" in lib.rgk_last_error()
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert exr(c=None, s=s) == INVALID and b"output_scale" in lib.rgk_last_error(), s
    assert os.listdir(str(tmp_path)) == []
    g.set_tuning(time_post=1)
    try:
        assert exr() == 0 and png() == 0
        auto, t13 = g.post_timing(12), g.post_timing(13)
        assert exr(s=2.0) == 0
        fixed = g.post_timing(12)
        assert len(auto) == 2 and min(auto) > 0 and len(fixed) == 2 and fixed[0] == 0 and fixed[1] > 0 and len(t13) == 2 and min(t13) > 0
        record_parity("gpu_output.timing[65x3]", max_ms=auto[0], pack_exr_ms=auto[1], pack_png_ms=t13[0], sums_ms=t13[1])
    finally:
        g.set_tuning(time_post=0)
    assert exr() == 0 and png() == 0 and g.post_timing(12) == [] and g.post_timing(13) == []
    assert np.array_equal(np.fromfile(path.decode(), np.uint8), OC.host_png(np.zeros((3, 65), np.uint32), tmp_path / "h.png"))
