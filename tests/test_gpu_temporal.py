"""Temporal reuse on the GPU: rgk_temporal_reproject_device and rgk_temporal_blend_device against their numpy restatement
(tests/temporal_ref.py), bit for bit, on the GPU's own feature planes of two cameras of an animation; the refusals, the timing
slot, and three frames end to end through RenderDriver with one TemporalHistory."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera
from rgk_amd.scene import glm_rotate
from rgk_amd.workloads import SceneFixture

import post_ref as R
import temporal_ref as T
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1
SIZES = [(1, 1), (67, 45), (96, 96)]
SCENES = {"spheres": "scene_cornell-box-spheres.npz", "box6": "scene_box6.npz"}


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fixture_scene(name):
    return SceneFixture(os.path.join(ROOT, "tests", "golden", SCENES[name]), spp=4)


def animation_camera(wl, W, H, t):
    """The config's get_camera(t): the position turned by t of a full circle about the up vector through the look-at point."""
    c = wl.builder.extra["camera"]
    pos, lookat, up = (np.array(c[k], F) for k in ("pos", "lookat", "up"))
    if t != 0.0:
        rot = glm_rotate(F(t) * F(2.0) * F(math.pi), up)[:3, :3]
        pos = lookat - (rot @ (lookat - pos)).astype(F)
    return make_camera(pos, lookat, up, fov=c.get("fov"), focal=c.get("focal"), xres=W, yres=H)


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def gpu_reproject(g, cam, prev, cur_planes, prev_planes, hist, tp=None, fill=None):
    """cur_planes / prev_planes: (depth, normal, tri); hist: (rgb, length) -> (hist_rgb, hist_len) as numpy."""
    import torch
    H, W = cur_planes[0].shape
    t = [up(a) for a in tuple(cur_planes) + tuple(prev_planes) + tuple(hist)]
    out = torch.full((H, W, 3), -1.0 if fill is None else fill, dtype=torch.float32, device="cuda:0")
    ln = torch.full((H, W), -1.0 if fill is None else fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g.temporal_reproject_device(W, H, cam, prev, *[x.data_ptr() for x in t], tp or capi.TemporalParams(), out.data_ptr(), ln.data_ptr())
    return out.cpu().numpy(), ln.cpu().numpy()


def gpu_blend(g, acc, cnt, alb, hist_rgb, hist_len, tp=None, fill=None):
    import torch
    H, W = hist_len.shape
    tp = tp or capi.TemporalParams()
    t = [up(acc), up(cnt), None if alb is None else up(alb), up(hist_rgb), up(hist_len)]
    outs = [torch.full(s, -1.0 if fill is None else fill, dtype=torch.float32, device="cuda:0") for s in ((H, W, 3), (H, W), (H, W, 3))]
    torch.cuda.synchronize()
    g.temporal_blend_device(W, H, *[None if x is None else x.data_ptr() for x in t], tp, *[o.data_ptr() for o in outs])
    return [o.cpu().numpy() for o in outs]


def random_history(W, H, seed):
    """Colours in [0, 2), lengths in [0, 10] with a quarter of them 0."""
    rng = np.random.default_rng(seed)
    rgb = (rng.random((H, W, 3)) * 2).astype(F)
    length = (rng.random((H, W)) * 10).astype(F)
    length[rng.random((H, W)) < 0.25] = 0
    return rgb, length


class Case:
    pass


def planes3(aov):
    """(depth, normal, tri) of render_aov's (albedo, normal, depth, tri)."""
    return aov[2], aov[1], aov[3]


def build_cases(rd, names, sizes):
    """Per scene: the GPU scene, and per size the two cameras (t = 0 and 2/500), their feature planes, a 4-spp accumulator of
    the later one and a random previous history."""
    out = {}
    for name in names:
        wl = fixture_scene(name)
        desc = wl.builder.to_desc()
        g = rd.Scene(desc)
        kinds = T.tri_kinds(desc)
        for k, (W, H) in enumerate(sizes):
            c = Case()
            c.g, c.kinds, c.W, c.H = g, kinds, W, H
            c.prev_cam, c.cam = animation_camera(wl, W, H, 0.0), animation_camera(wl, W, H, 2.0 / 500.0)
            c.away_cam = animation_camera(wl, W, H, 0.5)
            prm = wl.params()
            prm.xres, prm.yres = W, H
            tiles = rd.generate_task_list(W, H)
            c.prev_aov = g.render_aov(c.prev_cam, prm, tiles)
            c.aov = g.render_aov(c.cam, prm, tiles)
            c.away_aov = g.render_aov(c.away_cam, prm, tiles)
            c.acc, c.cnt, _ = g.render_round(c.cam, prm, tiles)
            c.hist = random_history(W, H, 7 + k)
            out[(name, (W, H))] = c
    return out


@pytest.fixture(scope="module")
def cases(rd):
    """Made once, never changed."""
    return build_cases(rd, list(SCENES), SIZES)


def ref_reproject(c, cam, prev, aov, prev_aov, hist, tp=None, **kw):
    tp = tp or capi.TemporalParams()
    return T.reproject_ref(cam, prev, aov[2], aov[1], aov[3], prev_aov[2], prev_aov[1], prev_aov[3], hist[0], hist[1], c.kinds,
                           plane_tol=tp.plane_tol, normal_cos=tp.normal_cos, **kw)


def differing(got, want):
    d = bits(got) != bits(want)
    return int((d.any(axis=-1) if d.ndim == 3 else d).sum())


# ----------------------------------------------------------------------- both entries against the restatement
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(SCENES))
def test_both_entries_equal_the_numpy_restatement(cases, name, size):
    """np.array_equal on every output.  67 x 45 = 3015 pixels: the twelfth workgroup has 57 idle lanes, and a camera that turns
    moves the taps of the border pixels out of the frame on every side."""
    c = cases[(name, size)]
    g_rgb, g_len = gpu_reproject(c.g, c.cam, c.prev_cam, planes3(c.aov), planes3(c.prev_aov), c.hist)
    r_rgb, r_len, ntaps = ref_reproject(c, c.cam, c.prev_cam, c.aov, c.prev_aov, c.hist, want_taps=True)
    d_rgb, d_len = differing(g_rgb, r_rgb), differing(g_len, r_len)
    share = float((r_len > 0).mean())
    tri = c.aov[3]
    specular = (tri >= 0) & np.isin(c.kinds[np.where(tri >= 0, tri, 0)], T.SPECULAR_KINDS)
    record_parity(f"gpu_temporal.reproject[{name} {size[0]}x{size[1]}]", rgb_differ=d_rgb, len_differ=d_len, with_history=share,
                  specular=float(specular.mean()), sky=float((tri < 0).mean()), partial_taps=float(((ntaps > 0) & (ntaps < 4)).mean()))
    assert d_rgb == 0 and d_len == 0
    assert (r_len[specular] == 0).all()
    if size == (96, 96):
        assert share > 0.4 and ((ntaps > 0) & (ntaps < 4)).any()  # most pixels find history, some at an edge of it
        if name == "spheres":
            assert specular.any()
    # the blend of this frame's accumulator into what the reprojection found, with and without demodulation, and a pixel without samples
    cnt = c.cnt.copy()
    if size != (1, 1):
        cnt[5, 7] = 0
    for tp in (capi.TemporalParams(), capi.TemporalParams(demodulate=0, alpha_min=0.3, max_len=4.0), capi.TemporalParams(albedo_floor=0.5)):
        got = gpu_blend(c.g, c.acc, cnt, c.aov[0], g_rgb, g_len, tp)
        want = T.blend_ref(c.acc, cnt, c.aov[0], r_rgb, r_len, tp.alpha_min, tp.max_len, tp.demodulate, tp.albedo_floor)
        assert [differing(a, b) for a, b in zip(got, want)] == [0, 0, 0]
    tp = capi.TemporalParams(demodulate=0)
    got = gpu_blend(c.g, c.acc, cnt, None, g_rgb, g_len, tp)  # no albedo plane needed then
    assert differing(got[2], T.blend_ref(c.acc, cnt, None, r_rgb, r_len, tp.alpha_min, tp.max_len, 0, tp.albedo_floor)[2]) == 0
    # other tolerances: the restatement follows
    tp = capi.TemporalParams(plane_tol=0.0005, normal_cos=0.999)
    g2 = gpu_reproject(c.g, c.cam, c.prev_cam, planes3(c.aov), planes3(c.prev_aov), c.hist, tp)
    r2 = ref_reproject(c, c.cam, c.prev_cam, c.aov, c.prev_aov, c.hist, tp)
    assert differing(g2[0], r2[0]) == 0 and differing(g2[1], r2[1]) == 0


@pytest.mark.parametrize("name", list(SCENES))
def test_looking_away_all_miss_and_first_frame(cases, name):
    c = cases[(name, (67, 45))]
    H, W = c.H, c.W
    # the camera half a circle on looks the other way across the look-at point: what it sees was behind the previous view screen or is
    # rejected by the surface tests; the restatement says which, and almost nothing is reused
    got = gpu_reproject(c.g, c.away_cam, c.prev_cam, planes3(c.away_aov), planes3(c.prev_aov), c.hist)
    want = ref_reproject(c, c.away_cam, c.prev_cam, c.away_aov, c.prev_aov, c.hist)
    assert differing(got[0], want[0]) == 0 and differing(got[1], want[1]) == 0
    # a previous camera that looks straight away from everything the current one sees: q <= 0 everywhere
    back = capi.Camera.from_buffer_copy(c.cam)
    for k in range(3):
        back.direction[k] = -c.cam.direction[k]
    got = gpu_reproject(c.g, c.cam, back, planes3(c.aov), planes3(c.aov), c.hist)
    assert (got[0] == 0).all() and (got[1] == 0).all()
    # an all-miss frame: sky found again by direction alone
    miss = (np.zeros((H, W), F), np.zeros((H, W, 3), F), np.full((H, W), -1, np.int32))
    got = gpu_reproject(c.g, c.cam, c.prev_cam, miss, miss, c.hist)
    want = T.reproject_ref(c.cam, c.prev_cam, miss[0], miss[1], miss[2], miss[0], miss[1], miss[2], c.hist[0], c.hist[1], c.kinds)
    assert differing(got[0], want[0]) == 0 and differing(got[1], want[1]) == 0 and (want[1] > 0).mean() > 0.5
    # a first frame: every length 0 -> nothing found, and the blend is the frame itself with length 1
    none = (c.hist[0], np.zeros((H, W), F))
    got = gpu_reproject(c.g, c.cam, c.prev_cam, planes3(c.aov), planes3(c.prev_aov), none)
    assert (got[0] == 0).all() and (got[1] == 0).all()
    h, L, out = gpu_blend(c.g, c.acc, c.cnt, c.aov[0], got[0], got[1])
    assert (L == 1).all() and differing(h, T.blend_ref(c.acc, c.cnt, c.aov[0], got[0], got[1])[0]) == 0
    mean = R.mean_color(c.acc, c.cnt)
    assert np.allclose(out, mean, rtol=3e-7, atol=0)  # (c / div) * div: two roundings


POISON_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_temporal as t
from rgk_amd import render_driver as rd
c = t.build_cases(rd, ["box6"], [(67, 45)])[("box6", (67, 45))]
poison = float(np.frombuffer(b"\\xff" * 4, np.float32)[0])
g_rgb, g_len = t.gpu_reproject(c.g, c.cam, c.prev_cam, t.planes3(c.aov), t.planes3(c.prev_aov), c.hist, fill=poison)
outs = t.gpu_blend(c.g, c.acc, c.cnt, c.aov[0], g_rgb, g_len, fill=poison)
for a in [g_rgb, g_len] + outs:
    assert not (t.bits(a) == 0xFFFFFFFF).any() and np.isfinite(a).all()
r = t.ref_reproject(c, c.cam, c.prev_cam, c.aov, c.prev_aov, c.hist)
assert t.differing(g_rgb, r[0]) == 0 and t.differing(g_len, r[1]) == 0
print("poison ok")
"""


def test_with_poisoned_allocations_every_output_element_is_written(rd, tmp_path):
    """RGK_POISON is read once per process, so this runs in a child: every fresh device buffer of the library starts as 0xFF
    bytes, the output planes start as the same pattern, and afterwards no element of any output holds it (67 x 45: the last
    workgroup is ragged) and the results are the restatement's."""
    script = tmp_path / "poison_child.py"
    script.write_text(POISON_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, RGK_POISON="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stderr + r.stdout


def test_refusals_leave_the_outputs_alone(cases):
    import torch
    c = cases[("box6", (67, 45))]
    g, lib, H, W = c.g, c.g.lib, c.H, c.W
    ins = [up(a) for a in planes3(c.aov) + planes3(c.prev_aov) + c.hist]
    acc, cnt, alb = up(c.acc), up(c.cnt), up(c.aov[0])
    o_rgb, o_len, o_img = (torch.full(s, 7.5, dtype=torch.float32, device="cuda:0") for s in ((H, W, 3), (H, W), (H, W, 3)))
    torch.cuda.synchronize()
    good_tp = capi.TemporalParams()

    def rp(tp=good_tp, xres=W, yres=H, out=(o_rgb, o_len), inputs=ins):
        return lib.rgk_temporal_reproject_device(g.h, xres, yres, C.byref(c.cam), C.byref(c.prev_cam), *[x.data_ptr() for x in inputs], C.byref(tp),
                                                 out[0].data_ptr(), out[1].data_ptr())

    def bl(tp=good_tp, xres=W, yres=H, out=(o_rgb, o_len, o_img), albedo=alb, hist=(ins[6], ins[7])):
        return lib.rgk_temporal_blend_device(g.h, xres, yres, acc.data_ptr(), cnt.data_ptr(), None if albedo is None else albedo.data_ptr(),
                                             hist[0].data_ptr(), hist[1].data_ptr(), C.byref(tp), *[o.data_ptr() for o in out])

    def refused(rc):
        assert rc == INVALID and lib.rgk_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == 7.5).all()) for o in (o_rgb, o_len, o_img))

    before = [x.clone() for x in ins]
    for field, v in (("alpha_min", 0.0), ("max_len", 0.5), ("plane_tol", float("nan")), ("normal_cos", float("nan")), ("alpha_min", float("nan")),
                     ("max_len", float("nan")), ("albedo_floor", float("nan"))):
        bad = capi.TemporalParams()
        setattr(bad, field, v)
        refused(rp(tp=bad))
        refused(bl(tp=bad))
    refused(rp(out=(ins[6], o_len)))          # an output on top of an input
    refused(rp(out=(o_rgb, ins[7])))
    refused(rp(out=(o_rgb, ins[0])))
    refused(bl(out=(ins[6], o_len, o_img)))
    refused(bl(out=(o_rgb, ins[7], o_img)))
    refused(bl(out=(o_rgb, o_len, acc)))
    refused(bl(out=(o_rgb, o_len, o_rgb)))    # ... or on another output
    refused(bl(albedo=None))                  # demodulate without an albedo plane
    assert b"albedo" in lib.rgk_last_error()
    for xres, yres in ((0, H), (W, 0), (0, 0)):
        refused(rp(xres=xres, yres=yres))
        refused(bl(xres=xres, yres=yres))
    assert all(torch.equal(a, b) for a, b in zip(before, ins))
    assert rp() == 0 and bl() == 0  # and the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert not bool((o_img == 7.5).any())


def test_timing_slot_5_holds_the_pair(cases):
    c = cases[("box6", (96, 96))]
    g = c.g
    g.set_tuning(time_post=1)
    try:
        rgb, ln = gpu_reproject(g, c.cam, c.prev_cam, planes3(c.aov), planes3(c.prev_aov), c.hist)
        t = g.post_timing(5)
        assert len(t) == 2 and t[0] > 0 and t[1] == 0
        gpu_blend(g, c.acc, c.cnt, c.aov[0], rgb, ln)
        t2 = g.post_timing(5)
        assert len(t2) == 2 and t2[0] == t[0] and t2[1] > 0
        record_parity("gpu_temporal.timing[box6 96x96]", reproject_ms=t2[0], blend_ms=t2[1])
    finally:
        g.set_tuning(time_post=0)
    gpu_blend(g, c.acc, c.cnt, c.aov[0], rgb, ln)
    assert g.post_timing(5) == []


# ----------------------------------------------------------------------- end to end
def _cfg(wl, W, H, spp):
    prm = wl.params()
    prm.xres, prm.yres, prm.multisample = W, H, spp

    class Cfg:
        xres, yres, render_rounds, render_minutes = W, H, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: prm)
    return Cfg


def test_three_frames_with_history_beat_the_third_frame_alone(rd):
    """Cornell with spheres, 96 x 96, 4 spp per frame at t = 0, 1/500, 2/500 through RenderDriver with one TemporalHistory: on the
    pixels whose first hit is not specular the third frame's temporal image is strictly closer (relative L2) to a 1024-spp render
    of the third camera than its single-frame denoise() -- it carries three times the samples.  The history changes nothing else:
    accumulators and denoise() outputs of all three frames are the bits a chain without one gives."""
    W = H = 96
    wl = fixture_scene("spheres")
    desc = wl.builder.to_desc()
    scene = rd.Scene(desc)
    cams = [animation_camera(wl, W, H, k / 500.0) for k in range(3)]
    hist = rd.TemporalHistory()
    with_h, without = [], []
    for cam in cams:
        for keep, h in ((with_h, hist), (without, None)):
            drv = rd.RenderDriver(scene, _cfg(wl, W, H, 4), cam, history=h)
            drv.render_round()
            plain = drv.denoise().cpu().numpy()
            temporal = None
            if h is not None:
                temporal = drv.denoise_temporal().cpu().numpy()
                state = (hist.rgb.cpu().numpy(), hist.length.cpu().numpy())
                again = drv.denoise_temporal().cpu().numpy()  # the same frame twice: not blended into itself
                assert differing(again, temporal) == 0 and differing(hist.rgb.cpu().numpy(), state[0]) == 0 and differing(hist.length.cpu().numpy(), state[1]) == 0
            keep.append((drv.total_ob.data.cpu().numpy(), drv.total_ob.count.cpu().numpy(), plain, temporal))
    for a, b in zip(with_h, without):
        assert differing(a[0], b[0]) == 0 and np.array_equal(a[1], b[1]) and differing(a[2], b[2]) == 0
    ref_drv = rd.RenderDriver(scene, _cfg(wl, W, H, 1024), cams[2])
    ref_drv.render_round()
    ref = ref_drv.total_ob.get_pixels().cpu().numpy()
    tri = ref_drv.render_aov()["tri"].cpu().numpy()
    kinds = T.tri_kinds(desc)
    keep = ~((tri >= 0) & np.isin(kinds[np.where(tri >= 0, tri, 0)], T.SPECULAR_KINDS))
    e_single, e_temporal = R.rel_l2(with_h[2][2][keep], ref[keep]), R.rel_l2(with_h[2][3][keep], ref[keep])
    e_noisy = R.rel_l2((with_h[2][0] / with_h[2][1][..., None].astype(F))[keep], ref[keep])
    L = hist.length.cpu().numpy()
    print(f"temporal end to end: noisy {e_noisy:.4f}  single-frame denoise {e_single:.4f}  temporal {e_temporal:.4f}  pixels with history {hist.share:.4f}  "
          f"mean length {float(L.mean()):.3f}  non-specular pixels {float(keep.mean()):.4f}")
    record_parity("gpu_temporal.end_to_end[spheres 96x96, 3 x 4 spp vs 1024]", noisy_rel_l2=e_noisy, single_rel_l2=e_single, temporal_rel_l2=e_temporal,
                  with_history=float(hist.share), mean_length=float(L.mean()))
    assert hist.share > 0.5 and L.max() == 3
    assert e_temporal < e_single


SCENE = '''{
    "output-file": "t.exr", "output-width": 48, "output-height": 40, "multisample": 4, "rounds": 2, "recursion-max": 3, "clamp": 20,
    "camera": {"position": [0,1.2,5], "lookat": [0,0.8,0], "fov": 35},
    "materials": [{"name": "m", "brdf": "diffuse", "diffuse255": [255, 128, 0]},
                  {"name": "g", "brdf": "diffuse", "diffuse": [0.4,0.4,0.5]},
                  {"name": "l", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5], "emission": [9,9,8]}],
    "scene": [{"primitive": "cube", "material": "m", "translate": [0,0.5,0]},
              {"primitive": "plane", "material": "g", "scale": [4,1,4]},
              {"primitive": "plane", "material": "l", "scale": [0.5,1,0.5], "translate": [0,3,0], "rotate": [180, 0, 0]}],
    "sky": {"color": [0.3, 0.4, 0.6], "intensity": 0.5}
}'''


def test_cli_temporal_changes_only_the_denoised_images_after_the_first_frame(rd, tmp_path):
    cfg = tmp_path / "s.json"
    cfg.write_text(SCENE)
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir(); b.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for d, extra in ((a, ["--temporal"]), (b, [])):
        r = subprocess.run([sys.executable, "-m", "rgk_amd", str(cfg), "-D", str(d), "-r", "--frames", "2", "--denoise", "-q"] + extra, cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
    names = sorted(os.listdir(str(b)))
    assert names == sorted(os.listdir(str(a))) == ["t.00000.denoised.exr", "t.00000.exr", "t.00001.denoised.exr", "t.00001.exr"]
    for n in ("t.00000.exr", "t.00001.exr"):
        assert (a / n).read_bytes() == (b / n).read_bytes()
    d1a, d1b = rd.read_exr(str(a / "t.00001.denoised.exr")), rd.read_exr(str(b / "t.00001.denoised.exr"))
    assert np.isfinite(d1a).all() and not np.array_equal(d1a, d1b)
    assert abs(float(d1a[..., :3].mean()) - float(d1b[..., :3].mean())) < 0.2 * float(d1b[..., :3].mean())
