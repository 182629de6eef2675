"""GPU suite (-m gpu): what a shading launch computes depends on the arguments of THAT launch alone.

k_shade and k_last_vertex take the scene, the camera and the pass by value, 872 bytes of arguments, and how the kernels come by
them is open to change: held in registers from the entry, or fetched from the argument segment or a device-resident copy where
they are used ("Shading kernels: packed fp32 and SGPR spills").  Whatever the route, a launch must see what
it was given, not what an earlier launch, another scene or another pass left behind.  So in one process, on the bump-mapped
fixture scene (tests/golden/scene_rubiks-bump.npz: one point light, on the constant-light route) and the Cornell box (area
lights, off it), at 8 spp and depth 3, every comparison exact (bits of the RGB sums, sample counts, path and shadow ray counts):
  - camera A, camera B (moved, with a lens: another sampler layout), camera A again: the third equals the first, and each equals
    the same camera rendered by a fresh scene;
  - two scenes alive at once, rounds interleaved: each equals the same scene rendered alone;
  - a round split into passes by a small batch_paths (the tuning key behind RGK_BATCH_PATHS; pixel ranges and sample passes, so
    j0 and s0 differ from launch to launch) equals the unsplit round;
  - the constant-light route on and off agree, as test_gpu_const_light requires.
Frames: 64 x 64, and 62 x 50 -- 24 800 paths, 48 first-vertex workgroups of 512 and one of 224, and a pixel count that is no
multiple of the 256-thread workgroups of the later vertices either.  The fresh-scene renders are made once per scene and frame
and shared by the tests."""
import os

import numpy as np
import pytest

from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPP, DEPTH = 8, 3
FRAMES = [(64, 64), (62, 50)]
SCENES = {"rubiks-bump": os.path.join(ROOT, "tests", "golden", "scene_rubiks-bump.npz"),
          "cornell": os.path.join(ROOT, "rgk_amd", "data", "cornell_scene.npz")}
CONST_LIGHT = {"rubiks-bump": 1, "cornell": 0}   # rgk_scene_info::const_light of the two


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


class Case:
    """A scene at a frame size: its builder, two cameras, the round's parameters and tiles."""

    def __init__(self, rd, name, frame):
        self.name, (self.w, self.h) = name, frame
        self.builder = SceneBuilder.load_npz(SCENES[name])
        ex = self.builder.extra
        c = ex["camera"]
        pos, look = np.asarray(c["pos"], np.float64), np.asarray(c["lookat"], np.float64)
        kw = dict(fov=c.get("fov"), focal=c.get("focal"), xres=self.w, yres=self.h)
        self.cam = {"A": make_camera(c["pos"], c["lookat"], c["up"], focus_plane=c.get("focus_plane", 1.0), lens_size=0.0, **kw),
                    # B: a quarter closer and off to the side, with a lens focused on the look-at point
                    "B": make_camera(list(look + 0.75 * (pos - look) + np.array([0.3, 0.2, 0.0])), c["lookat"], c["up"],
                                     focus_plane=float(0.75 * np.linalg.norm(pos - look)), lens_size=0.05, **kw)}
        self.prm = make_params(self.w, self.h, SPP, DEPTH, clamp=float(ex["clamp"]), russian=float(ex["russian"]),
                               bumpscale=float(ex["bumpscale"]), reverse=0)
        self.tiles = rd.generate_task_list(self.w, self.h)

    def scene(self, rd, **tuning):
        g = rd.Scene(self.builder.to_desc())
        assert g.info().const_light == CONST_LIGHT[self.name]
        if tuning:
            g.set_tuning(**tuning)
        return g

    def render(self, g, which):
        return g.render_round(self.cam[which], self.prm, self.tiles)


_cases, _alone = {}, {}


def case_of(rd, name, frame):
    if (name, frame) not in _cases:
        _cases[name, frame] = Case(rd, name, frame)
    return _cases[name, frame]


def alone(rd, cs, which):
    """Camera `which` of the case rendered by a fresh scene at default switches: made once, read by every test."""
    key = (cs.name, cs.w, cs.h, which)
    if key not in _alone:
        g = cs.scene(rd)
        acc, cnt, k = cs.render(g, which)
        g.close()
        assert (cnt == SPP).all() and float(acc.max()) > 0.0 and k.path_rays > 0 and k.shadow_rays > 0
        acc.setflags(write=False); cnt.setflags(write=False)
        _alone[key] = (acc, cnt, k)
    return _alone[key]


def assert_same_bits(base, got, what):
    (a0, c0, k0), (a1, c1, k1) = base, got
    assert np.array_equal(c0, c1), (what, "sample counts")
    differ = int((a0.view(np.uint32) != a1.view(np.uint32)).any(axis=2).sum())
    assert differ == 0, (what, f"{differ} pixels differ", float(np.linalg.norm(a1 - a0) / np.linalg.norm(a0)))
    assert (k0.path_rays, k0.shadow_rays) == (k1.path_rays, k1.shadow_rays), (what, "ray counts")


by_scene_and_frame = pytest.mark.parametrize("name,frame", [(n, f) for n in SCENES for f in FRAMES], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)


@by_scene_and_frame
def test_camera_a_then_b_then_a(rd, name, frame):
    cs = case_of(rd, name, frame)
    g = cs.scene(rd)
    a1, b, a2 = cs.render(g, "A"), cs.render(g, "B"), cs.render(g, "A")
    g.close()
    assert_same_bits(a1, a2, (name, frame, "camera A before and after camera B"))
    assert_same_bits(alone(rd, cs, "A"), a1, (name, frame, "camera A, first"))
    assert_same_bits(alone(rd, cs, "B"), b, (name, frame, "camera B behind camera A"))
    assert not np.array_equal(a1[0], b[0]), "the two cameras see the same image: the test shows nothing"


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_two_scenes_alive_with_rounds_interleaved(rd, frame):
    """The two scenes at two frame sizes (the second one's is the other entry of FRAMES), camera A and camera B each, in turn."""
    other = FRAMES[1 - FRAMES.index(frame)]
    c1, c2 = case_of(rd, "rubiks-bump", frame), case_of(rd, "cornell", other)
    g1, g2 = c1.scene(rd), c2.scene(rd)
    got = []
    for which in ("A", "B", "A"):
        got.append((c1, which, c1.render(g1, which)))
        got.append((c2, which, c2.render(g2, which)))
    g1.close(); g2.close()
    for cs, which, r in got:
        assert_same_bits(alone(rd, cs, which), r, (cs.name, (cs.w, cs.h), which, "interleaved with another scene"))


@by_scene_and_frame
@pytest.mark.parametrize("batch", [3000, 10000])
def test_round_split_into_passes(rd, name, frame, batch):
    """batch_paths 3000: fewer paths than the frame has pixels -- pixel ranges (j0 > 0) of single-sample passes (s0 = 0 .. 7);
    10 000: the whole pixel list, sample passes of 2 or 3 (64 x 64: 2)."""
    cs = case_of(rd, name, frame)
    assert batch < cs.w * cs.h * SPP and (batch > cs.w * cs.h or batch == 3000)
    g = cs.scene(rd, batch_paths=batch)
    got = [cs.render(g, which) for which in ("A", "B")]
    g.close()
    for which, r in zip(("A", "B"), got):
        assert_same_bits(alone(rd, cs, which), r, (name, frame, which, "batch_paths", batch))


@by_scene_and_frame
def test_constant_light_route_on_and_off(rd, name, frame):
    cs = case_of(rd, name, frame)
    for switch in (0, 1):
        g = cs.scene(rd, const_light=switch)
        got = [cs.render(g, which) for which in ("A", "B")]
        g.close()
        for which, r in zip(("A", "B"), got):
            assert_same_bits(alone(rd, cs, which), r, (name, frame, which, "const_light", switch))
