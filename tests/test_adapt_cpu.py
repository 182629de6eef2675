"""Adaptive tile sampling without a GPU: the selection rule (rgk_amd/csrc/rgk_adapt.h, rgk_adapt_select) and the round fold's grid
and tile-list check (rgk_plan.h, rgk_adapt.h).

  tests/cpp/adapt_main.cpp includes the two headers and nothing else of the library, is built with ASan + UBSan and run as a child
  process: known-answer masks (all retired, one hot tile, exactly on the threshold, a black frame, a tile without an estimable
  pixel, visits below min_visits, ragged 67 x 45 with tiles of 32 and of 5, 1 x 1), the refused parameters, and the fold's grid
  walked workgroup by workgroup and thread by thread: every element of every listed tile exactly once, nothing else.
  tests/adapt_ref.py restates the rule in numpy; rgk_adapt_select (ctypes, host only) agrees with it mask for mask on random
  statistics, inputs on the threshold included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rgk_amd import capi

import adapt_ref as A
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
INVALID = -1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapt") / "adapt_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "adapt_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("case", ["known", "refuse", "fold"])
def test_adapt_unit_on_the_cpu(harness, case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([harness, case], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout


def test_params_layout_and_exports(product_lib, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rgk.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(rgk_adapt_params), '
                   'offsetof(rgk_adapt_params, target), offsetof(rgk_adapt_params, min_visits));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.AdaptParams), capi.AdaptParams.target.offset, capi.AdaptParams.min_visits.offset]
    p = capi.AdaptParams()
    assert (p.target, p.min_visits) == (0.0, 4)
    for name in ("rgk_adapt_select", "rgk_round_fold_device"):
        assert name in capi.EXPORTS and getattr(product_lib, name) is not None


def call(lib, tiles, visits, xres, yres, ts, target, min_visits):
    live = np.full(tiles.size + 1, 0xAB, np.uint8)
    n_live, done = C.c_uint32(77), C.c_uint32(77)
    prm = capi.AdaptParams(target, min_visits)
    rc = lib.rgk_adapt_select(tiles.ctypes.data, visits.ctypes.data, xres, yres, ts, C.byref(prm), live.ctypes.data, C.byref(n_live), C.byref(done))
    assert live[-1] == 0xAB
    return rc, live[:-1], n_live.value, done.value


def test_select_refuses_bad_arguments_without_a_gpu(product_lib):
    lib = product_lib
    tiles = np.zeros(4, A.TILE_DT)
    visits = np.zeros(4, np.uint32)
    assert call(lib, tiles, visits, 64, 64, 32, 0.5, 4)[0] == 0
    for target, mv in ((0.5, 0), (0.5, 1), (float("nan"), 4), (float("inf"), 4), (-0.1, 4)):
        rc, live, n_live, done = call(lib, tiles, visits, 64, 64, 32, target, mv)
        assert rc == INVALID and (live == 0xAB).all() and (n_live, done) == (77, 77), (target, mv)
    assert b"rgk_adapt_select" in lib.rgk_last_error()
    for xres, yres, ts in ((0, 64, 32), (64, 0, 32), (65536, 64, 32), (64, 64, 0)):
        assert call(lib, tiles, visits, xres, yres, ts, 0.5, 4)[0] == INVALID
    prm, live = capi.AdaptParams(0.5, 4), np.zeros(4, np.uint8)
    good = [tiles.ctypes.data, visits.ctypes.data, 64, 64, 32, C.byref(prm), live.ctypes.data, None, None]
    assert lib.rgk_adapt_select(*good) == 0  # n_live and done may be NULL
    for k in (0, 1, 5, 6):
        a = list(good)
        a[k] = None
        assert lib.rgk_adapt_select(*a) == INVALID, k


def test_fold_refuses_bad_arguments_without_a_gpu(product_lib):
    """Reported before the scene or a device is touched: the `scene` below is 64 bytes of nothing."""
    lib = product_lib
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    bufs = [np.zeros(8 * 8 * 3, np.float32) for _ in range(6)]
    planes = [b.ctypes.data for b in bufs]
    tiles = (capi.Tile * 2)()
    tiles[0].x0, tiles[0].x1, tiles[0].y0, tiles[0].y1 = 0, 4, 0, 8
    tiles[1].x0, tiles[1].x1, tiles[1].y0, tiles[1].y1 = 4, 8, 0, 8
    flags = np.zeros(2, np.uint8)
    fold = lib.rgk_round_fold_device
    good = [scene, 8, 8, tiles, 2, flags.ctypes.data] + planes
    for k in (0, 3, 5, 6, 7, 8, 9, 10, 11):
        a = list(good)
        a[k] = None
        assert fold(*a) == INVALID, k
    for k, v in ((1, 0), (2, 0), (1, 65536), (1, 7), (2, 7)):  # resolution; a frame the tiles do not fit in
        a = list(good)
        a[k] = v
        assert fold(*a) == INVALID, (k, v)
    a = list(good)
    a[8] = a[6]  # total on top of round
    assert fold(*a) == INVALID and b"different" in lib.rgk_last_error()
    tiles[1].x0 = 3
    assert fold(*good) == INVALID and b"overlaps" in lib.rgk_last_error()
    tiles[1].x0 = tiles[1].x1 = 6
    assert fold(*good) == INVALID and b"empty" in lib.rgk_last_error()


def random_case(rng, k):
    xres, yres, ts = [(96, 96, 32), (67, 45, 32), (67, 45, 5), (1, 1, 32), (1920, 1080, 32)][k % 5]
    ty, tx = -(-yres // ts), -(-xres // ts)
    n = ty * tx
    tiles = np.zeros(n, A.TILE_DT)
    tiles["n_estimable"] = rng.integers(0, ts * ts + 1, n)
    if k % 7 == 0:
        tiles["n_estimable"][rng.integers(0, n)] = 0
    energy = rng.uniform(0.0, 4.0, n) * tiles["n_estimable"]
    tiles["sum_sq"] = np.where(tiles["n_estimable"] > 0, energy, 0.0)
    # variance: around the allowance, a few decades each way; some tiles exactly zero
    tiles["sum_var"] = np.where(tiles["n_estimable"] > 0, energy * 10.0 ** rng.uniform(-4, 0, n) * (rng.random(n) > 0.1), 0.0)
    if k % 11 == 0:
        tiles["sum_sq"] = 0.0  # a black frame ...
        tiles["sum_var"] = 0.0 if k % 2 else tiles["sum_var"]  # ... and one whose variance has no energy under it
    visits = rng.integers(0, 9, n).astype(np.uint32)
    target = float(np.float32(10.0 ** rng.uniform(-2.5, 0)))
    return xres, yres, ts, tiles, visits, target, int(rng.integers(2, 7))


def test_select_equals_the_numpy_restatement(product_lib):
    rng = np.random.default_rng(20260113)
    seen_live = seen_retired = seen_done = on_threshold = 0
    for k in range(300):
        xres, yres, ts, tiles, visits, target, mv = random_case(rng, k)
        if k % 3 == 0 and tiles["n_estimable"].sum() > 0:
            # put some tiles exactly on their threshold, formed as the rule forms it (it depends on the frame's energy and estimable
            # pixels, not on the variances being set here)
            SQ, NE = 0.0, 0
            for t in tiles:
                SQ += float(t["sum_sq"])
                NE += int(t["n_estimable"])
            t32 = float(np.float32(target))
            allowance = (t32 * t32) * SQ
            pick = np.flatnonzero(tiles["n_estimable"] > 0)[:3]
            for j in pick:
                tiles["sum_var"][j] = allowance * (float(tiles["n_estimable"][j]) / float(NE))
            visits[pick] = mv
            on_threshold += 1
        rc, live, n_live, done = call(product_lib, tiles, visits, xres, yres, ts, target, mv)
        assert rc == 0
        wlive, wn, wdone = A.select(tiles, visits, target, mv)
        assert np.array_equal(live, wlive.astype(np.uint8)), k
        assert (n_live, bool(done)) == (wn, wdone), k
        if k % 3 == 0 and tiles["n_estimable"].sum() > 0:
            assert not live[pick].any(), k  # on the threshold is not above it
        seen_live += int(live.sum())
        seen_retired += int((live == 0).sum())
        seen_done += int(done)
    assert seen_live > 1000 and seen_retired > 1000 and 5 < seen_done < 295 and on_threshold >= 90


def test_driver_refuses_what_adaptive_cannot_do(product_lib):
    """Before a scene or a device is asked for anything."""
    from rgk_amd import render_driver as rd

    class Cfg:
        xres, yres, render_rounds, render_minutes = 67, 45, 1, None

        def __init__(self, reverse=0):
            self.reverse = reverse

        def get_params(self, sampler=0, flags=0):
            return capi.Params(xres=67, yres=45, multisample=2, depth=3, reverse=self.reverse)

    with pytest.raises(ValueError, match="track_noise"):
        rd.RenderDriver(None, Cfg(), None, device="cpu", adaptive=capi.AdaptParams(0.1))
    with pytest.raises(ValueError, match="reverse"):
        rd.RenderDriver(None, Cfg(reverse=2), None, device="cpu", track_noise=True, adaptive=capi.AdaptParams(0.1))
    with pytest.raises(ValueError, match="world_size"):
        rd.RenderDriver(None, Cfg(), None, device="cpu", rank=0, world_size=2, track_noise=True, adaptive=capi.AdaptParams(0.1))
    with pytest.raises(ValueError, match="min_visits"):
        rd.RenderDriver(None, Cfg(), None, device="cpu", track_noise=True, adaptive=capi.AdaptParams(0.1, 1))
    drv = rd.RenderDriver(None, Cfg(), None, device="cpu", track_noise=True, adaptive=capi.AdaptParams(0.1))
    assert drv.visits.shape == (6,) and sorted(drv.task_tile) == list(range(6))
    for i, t in enumerate(drv.tasks):
        assert (t.y0 // 32) * 3 + t.x0 // 32 == drv.task_tile[i]
    plain = rd.RenderDriver(None, Cfg(), None, device="cpu", track_noise=True)
    with pytest.raises(ValueError, match="adaptive"):
        plain.render_round(live=np.ones(6, bool))


def test_cli_refuses_adaptive_without_a_target(tmp_path):
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for extra, text in ((["--adaptive"], "--until-noise"), (["--adaptive", "1", "--until-noise", "0.1"], "--adaptive")):
        r = subprocess.run([sys.executable, "-m", "rgk_amd", "nothing.json"] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "ERROR" in r.stdout and text in r.stdout, r.stdout + r.stderr
