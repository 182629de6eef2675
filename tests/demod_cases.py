"""The GPU cases of test_gpu_demod.py that test_gpu_demod_memstate.py repeats in a child with RGK_POISON=1: the inputs, the calls of
rgk_render_round_demod_device / rgk_render_round_device on fresh scenes, and, run as a program, those cases in a process of their own
(python tests/demod_cases.py --out FILE.npz).

    ROUND_CASES   name -> RoundCase: one round through both entries on fresh scenes (test 1: the main accumulator is unchanged)
    SUM_CASES     name -> (scene, size, lens): A of one 8 spp round (test 2) and D of four 1 spp rounds (test 3), with the plain
                  entry's per-round images that D is rebuilt from
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from rgk_amd import capi  # noqa: E402
from rgk_amd.config import make_camera  # noqa: E402
from rgk_amd.workloads import SceneFixture  # noqa: E402

F = np.float32
FLOOR = 0.02
FIXTURES = {"spheres": "scene_cornell-box-spheres.npz", "rubiks": "scene_rubiks-bump.npz", "box6": "scene_box6.npz"}
SIZES = [(24, 24), (37, 19)]
# 41 x 29 = 1189 pixels: the smallest batch a scene takes is 1024 paths, so only a frame above that has two pixel ranges
SPLIT_SIZE = (41, 29)
SPPS = [1, 4, 8, 16]
COUNTER_FIELDS = ("paths", "path_rays", "shadow_rays", "node_visits", "tri_tests", "shadow_node_visits", "shadow_tri_tests", "n_trace_launches",
                  "n_shadow_launches", "n_shade_launches")

_FIX = {}


def fixture(name):
    if name not in _FIX:
        _FIX[name] = SceneFixture(os.path.join(ROOT, "tests", "golden", FIXTURES[name]))
    return _FIX[name]


def camera_of(name, w, h, lens=False):
    """The fixture's camera on a w x h grid; lens: with a lens of 0.05 focused on the look-at point."""
    c = fixture(name).builder.extra["camera"]
    focus = float(np.linalg.norm(np.asarray(c["pos"], np.float64) - np.asarray(c["lookat"], np.float64)))
    return make_camera(c["pos"], c["lookat"], c["up"], fov=c.get("fov"), focal=c.get("focal"), xres=w, yres=h,
                       focus_plane=focus if lens else 1.0, lens_size=0.05 if lens else 0.0)


def params_of(name, w, h, spp):
    wl = fixture(name)
    wl.xres, wl.yres, wl.multisample = w, h, spp
    prm = wl.params()
    prm.reverse = 0  # (box6 ships with reverse 3: demodulated rounds are unidirectional)
    return prm


class RoundCase:
    def __init__(self, scene, size, spp, tuning=None, lens=False, passes=1, builder=None):
        self.scene, self.size, self.spp, self.tuning, self.lens, self.passes, self.builder = scene, size, spp, dict(tuning or {}), lens, passes, builder


def variants(size, spp):
    """(tag, tuning, lens, expected passes) for one frame size and sample count."""
    P = size[0] * size[1]
    out = [("default", {}, False, 1), ("group0", dict(sample_group=0), False, 1), ("group3-beam0", dict(sample_group=3, beam=0), False, 1),
           ("group3-beam1", dict(sample_group=3, beam=1), False, 1), ("lens", {}, True, 1)]
    if spp >= 4:  # two samples per pass: spp / 2 sample passes, the default group lowered to 2 samples side by side
        out.append(("sample-passes", dict(batch_paths=2 * P), False, spp // 2))
        out.append(("sample-passes-group0", dict(batch_paths=2 * P, sample_group=0), False, spp // 2))
    return out


ROUND_CASES = {}
for _scene in ("spheres", "rubiks"):
    for _size in SIZES:
        for _spp in SPPS:
            for _tag, _tune, _lens, _passes in variants(_size, _spp):
                ROUND_CASES[f"{_scene} {_size[0]}x{_size[1]}x{_spp} {_tag}"] = RoundCase(_scene, _size, _spp, _tune, _lens, _passes)
    for _spp in (4, 8):  # batch_paths 1024 < 1189 pixels: two pixel ranges x one sample pass per sample
        ROUND_CASES[f"{_scene} {SPLIT_SIZE[0]}x{SPLIT_SIZE[1]}x{_spp} pixel-ranges"] = RoundCase(_scene, SPLIT_SIZE, _spp, dict(batch_paths=1024), False, 2 * _spp)

SUM_CASES = {f"{_scene} {_w}x{_h}{' lens' if _lens else ''}": (_scene, (_w, _h), _lens)
             for _scene in ("spheres", "rubiks") for (_w, _h) in SIZES for _lens in (False, True)}
SUM_SPP, SUM_ROUNDS = 8, 4


def counters_of(k):
    return np.array([int(getattr(k, f)) for f in COUNTER_FIELDS] + [int(ks.launches) for ks in k.kernel] + [int(ks.units) for ks in k.kernel], np.uint64)


def passes_of(g, depth):
    """The passes of the scene's last round, from the stage count rgk_scene_get_progress reports."""
    p = capi.Progress()
    capi.check(g.lib, g.lib.rgk_scene_get_progress(g.h, C.byref(p)))
    assert p.stages % max(1, depth) == 0
    return p.stages // max(1, depth)


class Planes:
    """Zeroed device planes of one frame: accum, count, demod (D), div (A)."""

    def __init__(self, w, h):
        import torch
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda:0")
        self.accum, self.count, self.demod, self.div = z(h, w, 3), z(h, w, dt=torch.int32), z(h, w, 3), z(h, w, 3)

    def host(self):
        import torch
        torch.cuda.synchronize()
        return dict(accum=self.accum.cpu().numpy(), count=self.count.cpu().numpy().view(np.uint32), demod=self.demod.cpu().numpy(), div=self.div.cpu().numpy())


def fresh_scene(rd, builder, tuning=None):
    g = rd.Scene(builder.to_desc())
    if tuning:
        g.set_tuning(**tuning)
    return g


def run_round_case(rd, case):
    """One round of the case through both entries, each on a scene of its own: the arrays of both."""
    import torch
    (w, h), builder = case.size, case.builder or fixture(case.scene).builder
    cam, prm = camera_of(case.scene, w, h, case.lens), params_of(case.scene, w, h, case.spp)
    tiles = rd.generate_task_list(w, h)
    out = {}
    for entry in ("plain", "demod"):
        g, pl = fresh_scene(rd, builder, case.tuning), Planes(w, h)
        torch.cuda.synchronize()
        before = int(g.lib.rgk_debug_poisoned_bytes())
        if entry == "plain":
            k = g.render_round_device(cam, prm, tiles, pl.accum.data_ptr(), pl.count.data_ptr())
        else:
            k = g.render_round_demod_device(cam, prm, tiles, pl.accum.data_ptr(), pl.count.data_ptr(), pl.demod.data_ptr(), pl.div.data_ptr(), FLOOR)
        res = pl.host()
        out.update({f"{entry}.accum": res["accum"], f"{entry}.count": res["count"], f"{entry}.counters": counters_of(k),
                    f"{entry}.passes": np.array([passes_of(g, prm.depth)], np.uint32)})
        out[f"_{entry}.poisoned_by_round"] = np.array([int(g.lib.rgk_debug_poisoned_bytes()) - before], np.uint64)  # (0 without RGK_POISON)
        if entry == "demod":
            out.update({"demod.D": res["demod"], "demod.A": res["div"]})
        g.close()
    return out


def run_sum_case(rd, name):
    """A of one SUM_SPP round; then a frame of SUM_ROUNDS rounds at 1 spp: D and A of the demodulated entry on one scene, and each
    round's image from the plain entry into a zeroed accumulator on another (the pinned code, not the code under test)."""
    import torch
    scene, (w, h), lens = SUM_CASES[name]
    builder, cam = fixture(scene).builder, camera_of(scene, w, h, lens)
    out = {}
    g, pl = fresh_scene(rd, builder), Planes(w, h)
    prm = params_of(scene, w, h, SUM_SPP)
    torch.cuda.synchronize()
    g.render_round_demod_device(cam, prm, rd.generate_task_list(w, h), pl.accum.data_ptr(), pl.count.data_ptr(), pl.demod.data_ptr(), pl.div.data_ptr(), FLOOR)
    res = pl.host()
    out.update({"spp8.A": res["div"], "spp8.D": res["demod"], "spp8.accum": res["accum"], "spp8.count": res["count"]})
    g.close()
    g, gp, pl = fresh_scene(rd, builder), fresh_scene(rd, builder), Planes(w, h)
    prm = params_of(scene, w, h, 1)
    n_tiles = len(rd.generate_task_list(w, h))
    for r in range(SUM_ROUNDS):
        tiles = rd.generate_task_list(w, h, rd.SEEDSTART, r * n_tiles)
        one = Planes(w, h)
        torch.cuda.synchronize()
        g.render_round_demod_device(cam, prm, tiles, pl.accum.data_ptr(), pl.count.data_ptr(), pl.demod.data_ptr(), pl.div.data_ptr(), FLOOR)
        gp.render_round_device(cam, prm, tiles, one.accum.data_ptr(), one.count.data_ptr())
        out[f"round{r}.L"] = one.host()["accum"]
    res = pl.host()
    out.update({"rounds.D": res["demod"], "rounds.A": res["div"], "rounds.accum": res["accum"], "rounds.count": res["count"]})
    g.close()
    gp.close()
    return out


def run_all(rd, names=None):
    """{case: {key: array}} of every round case and sum case (or the named ones), each with the poisoned byte total behind it."""
    lib = capi.load_product()
    res = {}
    for name in names or list(ROUND_CASES) + list(SUM_CASES):
        arrays = run_round_case(rd, ROUND_CASES[name]) if name in ROUND_CASES else run_sum_case(rd, name)
        arrays["_poisoned_total"] = np.array([int(lib.rgk_debug_poisoned_bytes())], np.uint64)
        res[name] = arrays
    return res


def flatten(res):
    return {f"{case}::{key}": a for case, arrays in res.items() for key, a in arrays.items()}


def unflatten(z):
    res = {}
    for k in z.files:
        case, key = k.split("::", 1)
        res.setdefault(case, {})[key] = z[k]
    return res


# The memstate run repeats every round case and every sum case.
MEMSTATE_ROUND_CASES = list(ROUND_CASES)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from rgk_amd import render_driver
    lib = capi.load_product()
    assert lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    before = int(lib.rgk_debug_poisoned_bytes())
    res = run_all(render_driver, MEMSTATE_ROUND_CASES + list(SUM_CASES))
    np.savez(args.out, **flatten(res))
    print(f"demod cases ok: {len(res)} cases, poisoned bytes {before} -> {int(lib.rgk_debug_poisoned_bytes())}")
