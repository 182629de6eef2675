"""Adaptive tile sampling on the GPU: the round fold (rgk_round_fold_device) against numpy bit for bit, and RenderDriver's adaptive
rounds end to end -- nothing retires means nothing changes, a sparse round holds the samples the whole round would have put there,
tiles that see nothing stop at min_visits, the estimate stays calibrated, a frame resumes from its checkpoint, and the command line.

Cornell at 96 x 96 (3 x 3 tiles), 2 samples per pixel and round.  "Far": the same box from 1.6 times the distance, the camera moved
right and down without turning, over the scene's black sky: the box's front is 58 pixels wide around pixel (32, 32) -- inside the
four tiles of the upper left -- and the five tiles of the right column and the bottom row see nothing.  (The box is then some
3000 pixels of the frame: the frame's estimate is a sum over enough of them to fall as 1 / sqrt(N) from round to round.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera
from rgk_amd.workloads import Workload

import adapt_ref as A
import post_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

W = H = 96
MS = 2


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def down(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.fixture(scope="module")
def world(rd):
    """The 2-spp Cornell workload, its scene on the GPU, and the far camera."""
    wl = Workload("cornell-256", scale=0.375, spp=MS)
    assert (wl.xres, wl.yres, wl.reverse) == (W, H, 0)
    c = wl.builder.extra["camera"]
    assert c["pos"][:2] == c["lookat"][:2] == [0.0, 1.0]
    far = make_camera([0.55, 0.45, 10.67], [0.55, 0.45, c["lookat"][2]], c["up"], fov=c["fov"], xres=W, yres=H)
    return wl, rd.Scene(wl.builder.to_desc()), far


def driver(rd, world, camera=None, rounds=1, **kw):
    wl, scene, _ = world

    class Cfg:
        xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, rounds, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    return rd.RenderDriver(scene, Cfg, camera or wl.camera, **kw)


def obs(drv):
    return [down(t) for t in (drv.total_ob.data, drv.total_ob.count, drv.half_ob.data, drv.half_ob.count)]


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def tile_slices():
    """The frame's tiles in the row-major order of noise()["tiles"]."""
    return [(slice(y, min(H, y + 32)), slice(x, min(W, x + 32))) for y in range(0, H, 32) for x in range(0, W, 32)]


# ----------------------------------------------------------------------- 1. the fold
def random_planes(rng, w, h):
    """round / total / half, rgb and count: floats of every size and sign -- denormals and values near 1e30 among them -- and
    counts over the whole 32-bit range (the addition wraps).  No plane holds a zero: a cleared pixel shows."""
    def rgb():
        a = (rng.standard_normal((h, w, 3)) * 10.0 ** rng.uniform(-44, 30, (h, w, 3))).astype(np.float32)
        a[a == 0] = np.float32(1e-45)
        sel = rng.random((h, w, 3)) < 0.1
        a[sel] = (rng.integers(1, 1 << 22, (h, w, 3)).astype(np.uint32).view(np.float32))[sel]  # denormals for sure
        return a

    def cnt():
        return rng.integers(1, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    return [rgb(), cnt(), rgb(), cnt(), rgb(), cnt()]


def tile_array(rects):
    t = (capi.Tile * len(rects))()
    for i, (x0, x1, y0, y1) in enumerate(rects):
        t[i].x0, t[i].x1, t[i].y0, t[i].y1, t[i].seed = x0, x1, y0, y1, 1000 + i
    return t


def gpu_fold(scene, w, h, rects, flags, planes):
    import torch
    t = [up(p) for p in planes]
    torch.cuda.synchronize()
    try:
        scene.round_fold_device(w, h, tile_array(rects), flags, *[x.data_ptr() for x in t])
    finally:
        torch.cuda.synchronize()
        out = [down(x) for x in t]
    return out


FOLD_CASES = {
    # 67 x 45: the 3 x 2 grid of 32-pixel tiles without two of them (ragged ones stay), flags mixed
    "67x45/grid": (67, 45, [(64, 67, 32, 45), (0, 32, 0, 32), (32, 64, 32, 45), (64, 67, 0, 32)], [1, 0, 1, 0]),
    # tiles of no grid: higher than one band of rows, a single pixel, a column one pixel wide, 5 x 5
    "67x45/odd": (67, 45, [(3, 66, 1, 44), (0, 1, 0, 45), (66, 67, 44, 45), (1, 6, 0, 1)], [0, 1, 1, 1]),
    "67x45/all": (67, 45, [(x, min(67, x + 32), y, min(45, y + 32)) for y in (0, 32) for x in (0, 32, 64)], [1, 1, 0, 0, 1, 0]),
    "1x1": (1, 1, [(0, 1, 0, 1)], [1]),
    "1x1/total-only": (1, 1, [(0, 1, 0, 1)], [0]),
    "67x45/nothing": (67, 45, [], []),
}


@pytest.mark.parametrize("case", list(FOLD_CASES))
def test_fold_equals_numpy(world, case):
    """All six planes np.array_equal (as bit patterns) to the restatement: total += round, half += round where flagged, round = 0
    inside the listed tiles; every pixel outside them keeps its random value in all six."""
    w, h, rects, flags = FOLD_CASES[case]
    planes = random_planes(np.random.default_rng(len(case) * 7919 + w), w, h)
    got = gpu_fold(world[1], w, h, rects, np.array(flags, np.uint8), planes)
    want = A.fold(rects, flags, *planes)
    inside = np.zeros((h, w), bool)
    for x0, x1, y0, y1 in rects:
        inside[y0:y1, x0:x1] = True
    for k, name in enumerate(("round_rgb", "round_count", "total_rgb", "total_count", "half_rgb", "half_count")):
        assert np.array_equal(bits(got[k]), bits(want[k])), name
        assert np.array_equal(bits(got[k][~inside]), bits(planes[k][~inside])), name  # outside: what was there
    assert (got[0][inside] == 0).all() and (got[1][inside] == 0).all()
    assert (bits(got[0][inside]) == 0).all()  # +0, not -0
    if rects:
        assert not (got[0][~inside] == 0).any() and (bits(got[2][inside]) != bits(planes[2][inside])).any()


@pytest.mark.parametrize("rects", [[(0, 32, 0, 32), (31, 40, 31, 40)], [(0, 32, 0, 32), (0, 32, 0, 32)], [(40, 68, 0, 10)], [(0, 10, 40, 46)],
                                   [(0, 32, 0, 32), (5, 5, 0, 3)]], ids=["overlap", "twice", "right of the frame", "below the frame", "empty"])
def test_fold_refuses_a_bad_tile_list_and_touches_nothing(world, rects):
    planes = random_planes(np.random.default_rng(5), 67, 45)
    with pytest.raises(RuntimeError, match="rgk error -1"):
        gpu_fold(world[1], 67, 45, rects, np.ones(len(rects), np.uint8), planes)
    import torch
    t = [up(p) for p in planes]
    torch.cuda.synchronize()
    rc = world[1].lib.rgk_round_fold_device(world[1].h, 67, 45, tile_array(rects), len(rects), np.ones(len(rects), np.uint8).ctypes.data, *[x.data_ptr() for x in t])
    torch.cuda.synchronize()
    assert rc == -1
    assert same_bits([down(x) for x in t], planes)


# ----------------------------------------------------------------------- 2. nothing retires: nothing changes
def test_nothing_retires_means_nothing_changes(rd, world):
    """Four rounds with min_visits 4 -- every tile is live in all of them -- through render_frame and its selection: the bits of the
    tracked driver's accumulator and half-buffer, and its task counter."""
    plain = driver(rd, world, track_noise=True)
    plain.render_frame(rounds=4, until_noise=1e-6)
    seen = []
    drv = driver(rd, world, track_noise=True, adaptive=capi.AdaptParams(min_visits=4))
    drv.render_frame(rounds=4, until_noise=1e-6, on_noise=lambda r, rel, n_live: seen.append((r, rel, n_live)))
    assert same_bits(obs(drv), obs(plain))
    assert (drv.seedcount, drv.rounds_done) == (plain.seedcount, plain.rounds_done) == (36, 4)
    assert (drv.visits == 4).all() and [(r, n) for r, _, n in seen[:2]] == [(2, 9), (3, 9)] and seen[2][1] == plain.noise()["rel"]
    assert float(drv.round_ob.data.abs().max()) == 0 and int(drv.round_ob.count.max()) == 0  # all zero between rounds
    # ... and by hand, without a selection
    byhand = driver(rd, world, track_noise=True, adaptive=capi.AdaptParams())
    for _ in range(4):
        byhand.render_round()
    assert same_bits(obs(byhand), obs(plain)) and byhand.seedcount == 36


def round_ob_is_zero(drv):
    return bool((drv.round_ob.data == 0).all()) and bool((drv.round_ob.count == 0).all())


def test_the_two_tracked_drivers_are_one(rd, world):
    """A tracked driver and an adaptive one driven without a mask take the same path through the round -- the per-round accumulator,
    then the fold over the tiles that were rendered: the same four planes bit for bit after every one of four rounds, the per-round
    accumulator all zero after each, and the accumulator of the driver that tracks nothing and renders in place."""
    tracked, adaptive, plain = driver(rd, world, track_noise=True), driver(rd, world, track_noise=True, adaptive=capi.AdaptParams()), driver(rd, world)
    assert plain.round_ob is None and plain.half_ob is None
    for r in range(1, 5):
        for d in (tracked, adaptive, plain):
            d.render_round()
        assert same_bits(obs(tracked), obs(adaptive)), r
        assert round_ob_is_zero(tracked) and round_ob_is_zero(adaptive), r
        assert same_bits(obs(tracked)[:2], [down(plain.total_ob.data), down(plain.total_ob.count)]), r
        assert (obs(tracked)[1] == r * MS).all() and (obs(tracked)[3] == (r // 2) * MS).all(), r
    assert plain.round_ob is None  # the untracked driver never made one
    assert (adaptive.visits == 4).all() and tracked.seedcount == adaptive.seedcount == plain.seedcount == 36


def test_the_fold_covers_what_a_round_writes(rd):
    """Bidirectional rounds: light-tracing splats land outside a path's own tile, anywhere in the frame.  The whole-frame fold of a
    tracked driver takes all of them: the per-round accumulator is all zero after each round, and the counts are the uniform
    multisample x rounds, and x (rounds // 2) in the half-buffer.  (No claim on the radiance bits: splat order is not fixed.)"""
    from rgk_amd.workloads import SceneFixture
    wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_box6.npz"), scale=0.04, spp=2, depth=3)
    assert wl.reverse > 0

    class Cfg:
        xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, 2, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    drv = rd.RenderDriver(rd.Scene(wl.builder.to_desc()), Cfg, wl.camera, track_noise=True)
    for r in (1, 2):
        drv.render_round()
        S, n, SB, nB = obs(drv)
        assert round_ob_is_zero(drv), r
        assert (n == wl.multisample * r).all() and (nB == wl.multisample * (r // 2)).all(), r
        assert np.isfinite(S).all() and S.max() > 0 and (SB.max() > 0) == (r == 2), r


# ----------------------------------------------------------------------- 3. sparse rounds are the same samples
def test_sparse_rounds_hold_the_samples_of_the_whole_rounds(rd, world):
    """all, all, then two different subsets: every tile holds the float32 sum, in the order of its visits, of its pixels in four
    separately rendered whole rounds with the same task-counter bases; the half-buffer the sum of its second and fourth visit."""
    wl, scene, _ = world
    schedule = [np.ones(9, bool), np.ones(9, bool), np.array([1, 0, 1, 0, 1, 1, 0, 0, 1], bool), np.array([0, 0, 1, 1, 1, 0, 1, 0, 1], bool)]
    rounds = []
    for r in range(4):
        acc, cnt, _ = scene.render_round(wl.camera, wl.params(), rd.generate_task_list(W, H, rd.SEEDSTART, 9 * r))
        assert (cnt == MS).all()
        rounds.append(acc)
    drv = driver(rd, world, track_noise=True, adaptive=capi.AdaptParams())
    for live in schedule:
        drv.render_round(live=live.reshape(3, 3))
    S, n, SB, nB = obs(drv)
    want_S, want_SB = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    visits = np.zeros(9, np.uint32)
    for t, s in enumerate(tile_slices()):
        for r in range(4):
            if schedule[r][t]:
                want_S[s] = want_S[s] + rounds[r][s]
                if visits[t] % 2 == 1:
                    want_SB[s] = want_SB[s] + rounds[r][s]
                visits[t] += 1
        assert (n[s] == visits[t] * MS).all() and (nB[s] == (visits[t] // 2) * MS).all(), t
        assert np.array_equal(bits(S[s]), bits(want_S[s])) and np.array_equal(bits(SB[s]), bits(want_SB[s])), t
    assert np.array_equal(drv.visits, visits) and sorted(set(visits)) == [2, 3, 4] and drv.seedcount == 36
    assert [int(c.paths) for c in drv.counters] == [W * H * MS, W * H * MS, 5 * 1024 * MS, 5 * 1024 * MS]


# ----------------------------------------------------------------------- 4. the structural saving
@pytest.fixture(scope="module")
def far_frames(rd, world):
    """The far camera: the uniform frame and the adaptive frame rendered to the same noise level X = 0.7 x the estimate after four
    uniform rounds (as test_gpu_noise.py chooses its target), at most 12 rounds."""
    far = world[2]
    probe = driver(rd, world, far, track_noise=True)
    for _ in range(4):
        probe.render_round()
    X = 0.7 * probe.noise()["rel"]
    uni = driver(rd, world, far, track_noise=True)
    uni.render_frame(rounds=12, until_noise=X)
    log = []
    ada = driver(rd, world, far, track_noise=True, adaptive=capi.AdaptParams(min_visits=4))
    ada.render_frame(rounds=12, until_noise=X, on_noise=lambda r, rel, n_live: log.append((r, rel, n_live)))
    return X, uni, ada, log


def test_tiles_that_see_nothing_stop_at_min_visits(rd, world, far_frames):
    X, uni, ada, log = far_frames
    tri = ada.render_aov()["tri"].cpu().numpy()
    missed = [t for t, s in enumerate(tile_slices()) if (tri[s] == -1).all()]
    assert len(missed) >= 4, missed
    n = down(ada.total_ob.count)
    for t in missed:
        assert (n[tile_slices()[t]] == 4 * MS).all() and ada.visits[t] == 4, t
    rel = ada.noise()["rel"]
    paths_a, paths_u = sum(int(c.paths) for c in ada.counters), sum(int(c.paths) for c in uni.counters)
    record_parity("gpu_adaptive.saving[cornell far 96x96]", target=X, rounds_adaptive=ada.rounds_done, rounds_uniform=uni.rounds_done, rel_adaptive=rel,
                  rel_uniform=uni.noise()["rel"], paths_adaptive=paths_a, paths_uniform=paths_u, all_miss_tiles=len(missed),
                  live_per_round="/".join(str(n_live) for _, _, n_live in log))
    assert rel <= X and uni.noise()["rel"] <= X and 4 < ada.rounds_done <= 12
    assert paths_a < paths_u
    assert paths_a == int(ada.visits.sum()) * 1024 * MS
    # the tiles that were live in every round hold what the uniform frame holds after as many rounds
    same = driver(rd, world, world[2], track_noise=True)
    for _ in range(ada.rounds_done):
        same.render_round()
    always = [t for t in range(9) if ada.visits[t] == ada.rounds_done]
    assert always and len(always) < 9
    for t in always:
        s = tile_slices()[t]
        assert same_bits([a[s] for a in obs(ada)], [a[s] for a in obs(same)]), t
    assert same.seedcount == ada.seedcount


# ----------------------------------------------------------------------- 5. the estimate under selection
def test_the_estimate_stays_honest_under_selection(rd, world):
    """estimated relative noise / measured rel-L2 against 256 spp, for the adaptive frame and for the uniform frame stopped at the
    same X: the adaptive ratio within the factor 1.25 the project accepts for this estimator (test_gpu_noise.py) of the uniform one.
    Tiles retire on an estimate made from the samples it then judges, which could bias it low (DESIGN.md 13 has the figures)."""
    wl, scene, _ = world
    hi = Workload("cornell-256", scale=0.375, spp=256)

    class Cfg:
        xres, yres, render_rounds, render_minutes = W, H, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: hi.params(sampler, flags))
    ref_drv = rd.RenderDriver(scene, Cfg, hi.camera)
    ref_drv.render_round()
    ref = ref_drv.total_ob.get_pixels().cpu().numpy()
    probe = driver(rd, world, track_noise=True)
    for _ in range(4):
        probe.render_round()
    X = 0.7 * probe.noise()["rel"]
    uni = driver(rd, world, track_noise=True)
    uni.render_frame(rounds=32, until_noise=X)
    log = []
    ada = driver(rd, world, track_noise=True, adaptive=capi.AdaptParams(min_visits=4))
    ada.render_frame(rounds=32, until_noise=X, on_noise=lambda r, rel, n_live: log.append(n_live))
    ratio = {}
    for name, d in (("uniform", uni), ("adaptive", ada)):
        est, measured = d.noise()["rel"], R.rel_l2(d.total_ob.get_pixels().cpu().numpy(), ref)
        ratio[name] = est / measured
        record_parity(f"gpu_adaptive.calibration[cornell 96x96, {name}]", target=X, rounds=d.rounds_done, estimated=est, measured=measured,
                      ratio=est / measured, paths=sum(int(c.paths) for c in d.counters))
    record_parity("gpu_adaptive.calibration[cornell 96x96, live tiles per round]", live="/".join(str(n) for n in log))
    print("calibration ratios", ratio, "live", log)
    assert uni.rounds_done < 32 and ada.rounds_done < 32 and ada.noise()["rel"] <= X
    assert ratio["uniform"] / 1.25 <= ratio["adaptive"] <= ratio["uniform"] * 1.25


# ----------------------------------------------------------------------- 6. checkpoint
def test_an_adaptive_frame_resumes_from_its_checkpoint(rd, world, far_frames, tmp_path):
    """Five rounds (the fifth is sparse), saved; a new driver resumes and finishes: the uninterrupted frame's bits, visits, rounds and
    task counter.  The per-tile state comes out of the count planes; a tile that is not uniform in its counts is refused."""
    X, _, whole, _ = far_frames
    assert whole.rounds_done > 5
    ck = str(tmp_path / "a.ck")
    first = driver(rd, world, world[2], track_noise=True, adaptive=capi.AdaptParams(min_visits=4))
    first.render_frame(rounds=5, until_noise=X, checkpoint=ck)
    assert first.rounds_done == 5 and first.visits.min() == 4 and first.visits.max() == 5
    assert sorted(os.listdir(str(tmp_path))) == ["a.ck", "a.ck.half"]
    back = driver(rd, world, world[2], track_noise=True, adaptive=capi.AdaptParams(min_visits=4))
    back.load_checkpoint(ck)
    assert np.array_equal(back.visits, first.visits) and (back.rounds_done, back.seedcount) == (5, 45)
    back.render_frame(rounds=12 - 5, until_noise=X)
    assert same_bits(obs(back), obs(whole))
    assert np.array_equal(back.visits, whole.visits) and (back.rounds_done, back.seedcount) == (whole.rounds_done, whole.seedcount)
    # a finished frame resumed: nothing more is rendered
    back.save_checkpoint(ck)
    again = driver(rd, world, world[2], track_noise=True, adaptive=capi.AdaptParams(min_visits=4))
    again.load_checkpoint(ck)
    again.render_frame(rounds=3, until_noise=X)
    assert again.rounds_done == whole.rounds_done and same_bits(obs(again), obs(whole))
    # one pixel with another count: refused
    back.total_ob.count[40, 40] += 1
    bad = str(tmp_path / "bad.ck")
    back.save_checkpoint(bad)
    with pytest.raises(RuntimeError, match="not uniform"):
        driver(rd, world, world[2], track_noise=True, adaptive=capi.AdaptParams()).load_checkpoint(bad)
    driver(rd, world, world[2], track_noise=True).load_checkpoint(bad)  # a uniform driver does not mind


# ----------------------------------------------------------------------- 7. the command line
SCENE = '''{
    "output-file": "post.exr", "output-width": 96, "output-height": 64, "multisample": 2, "rounds": %d, "recursion-max": 3, "clamp": 20,
    "camera": {"position": [0,1.2,14], "lookat": [0,0.8,0], "fov": 35},
    "materials": [{"name": "m", "brdf": "diffuse", "diffuse255": [255, 128, 0]},
                  {"name": "l", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5], "emission": [9,9,8]}],
    "scene": [{"primitive": "cube", "material": "m", "translate": [0,0.5,0]},
              {"primitive": "plane", "material": "l", "scale": [0.5,1,0.5], "translate": [0,3,0], "rotate": [180, 0, 0]}],
    "sky": {"color": [0.3, 0.4, 0.6], "intensity": 0.5}
}'''


def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([sys.executable, "-m", "rgk_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def test_cli_adaptive(rd, tmp_path):
    """--adaptive --until-noise X writes the output and its noise image and reports the live tiles; with a min_visits no round
    reaches, the output has the bytes of the frame rendered without any of the switches."""
    many, few = tmp_path / "many.json", tmp_path / "few.json"
    many.write_text(SCENE % 6)
    few.write_text(SCENE % 3)
    a, b, c = tmp_path / "adaptive", tmp_path / "guarded", tmp_path / "plain"
    for d in (a, b, c):
        d.mkdir()
    r = run_cli([str(many), "-D", str(a), "--adaptive", "--until-noise", "1e-4", "-q"], str(tmp_path))  # (out of reach: all 6 rounds)
    assert r.returncode == 0, r.stderr + r.stdout
    assert sorted(os.listdir(str(a))) == ["post.exr", "post.noise.exr"]
    lines = [ln.split() for ln in r.stdout.splitlines() if "live tiles" in ln]  # "Round R: N live tiles, relative noise V"
    live, rel = [int(ln[2]) for ln in lines], [float(ln[-1]) for ln in lines]
    assert [int(ln[1].rstrip(":")) for ln in lines] == [2, 3, 4, 5, 6], r.stdout
    # 3 x 2 tiles, most of them sky alone: those retire with their fourth visit, the ones with the cube in them never do
    assert live[:2] == [6, 6] and all(1 <= n < 6 for n in live[2:]) and all(0 < v < 1 for v in rel), r.stdout
    img = rd.read_exr(str(a / "post.exr"))
    assert img.shape == (64, 96, 4) and np.isfinite(img).all() and img[..., :3].max() > 0
    r = run_cli([str(few), "-D", str(b), "--adaptive", "8", "--until-noise", "1e-6", "-q"], str(tmp_path))
    assert r.returncode == 0, r.stderr + r.stdout
    r = run_cli([str(few), "-D", str(c), "-q"], str(tmp_path))
    assert r.returncode == 0 and "relative noise" not in r.stdout, r.stderr + r.stdout
    assert sorted(os.listdir(str(c))) == ["post.exr"]
    assert (b / "post.exr").read_bytes() == (c / "post.exr").read_bytes()
