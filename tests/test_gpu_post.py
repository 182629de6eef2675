"""Feature buffers (rgk_render_aov[_device]) against their composition from the oracle library, the a-trous denoiser
(rgk_denoise_device) against its numpy restatement, bit for bit, and both end to end through RenderDriver and the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder, glm_mat4_mul, glm_rotate, glm_scale, glm_translate
from rgk_amd.workloads import Workload

import post_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------- features against the oracle composition
def zoo():
    """Mirror, dielectric, transparent, a two-level mix, LTC with and without a diffuse part, and an emitter."""
    sb = SceneBuilder()

    def mat(name, kind, **kw):
        m = sb.new_material(name, kind)
        for k, v in kw.items():
            m[k] = sb.create_solid_texture(v) if k.startswith("tex_") else v
        return sb.register_material(m)
    mat("white", capi.BXDF_DIFFUSE, tex_diffuse=(0.7, 0.7, 0.7))
    mat("red", capi.BXDF_DIFFUSE, tex_diffuse=(0.6, 0.1, 0.1))
    mat("light", capi.BXDF_DIFFUSE, tex_diffuse=(0.5, 0.5, 0.5), emission=(12.0, 12.0, 10.0))
    mat("mirror", capi.BXDF_MIRROR, tex_color=(0.9, 0.9, 0.9))
    mat("glass", capi.BXDF_DIELECTRIC, tex_color=(1.0, 1.0, 1.0), ior=1.5)
    mat("ghost", capi.BXDF_TRANSPARENT)
    mat("bek", capi.BXDF_LTC_BECKMANN, tex_color=(0.8, 0.6, 0.2), roughness=0.3)
    mat("ggxd", capi.BXDF_LTC_GGX_DIFFUSE, tex_color=(0.3, 0.3, 0.3), tex_diffuse=(0.2, 0.4, 0.6), roughness=0.15)
    mat("inner", capi.BXDF_MIX, mix_m1=sb.material_index("red"), mix_m2=sb.material_index("bek"), amount=0.4)
    mat("mix2", capi.BXDF_MIX, mix_m1=sb.material_index("inner"), mix_m2=sb.material_index("mirror"), amount=0.7)

    def T(scale, translate, rot=None):
        m = glm_scale(scale)
        if rot:
            m = glm_mat4_mul(glm_rotate(rot[0], rot[1]), m)
        return glm_mat4_mul(glm_translate(translate), m)
    sb.add_primitive("plane", T((2, 1, 2), (0, 0, 0)), "white")
    sb.add_primitive("plane", T((2, 1, 2), (0, 1.5, -2), (np.pi / 2, (1, 0, 0))), "ggxd")
    sb.add_primitive("plane", T((2, 1, 2), (-2, 1.5, 0), (-np.pi / 2, (0, 0, 1))), "red")
    sb.add_primitive("plane", T((2, 1, 2), (2, 1.5, 0), (np.pi / 2, (0, 0, 1))), "mirror")
    sb.add_primitive("plane", T((0.5, 1, 0.5), (0, 2.98, 0), (np.pi, (1, 0, 0))), "light")
    sb.add_primitive("cube", T((0.8, 0.8, 0.8), (-0.9, 0.4, -0.5), (0.4, (0, 1, 0))), "glass")
    sb.add_primitive("cube", T((0.7, 1.4, 0.7), (0.8, 0.7, -0.8), (-0.3, (0, 1, 0))), "mix2")
    sb.add_primitive("cube", T((0.5, 0.5, 0.5), (0.2, 0.25, 0.9)), "bek")
    sb.add_primitive("plane", T((0.4, 1, 0.4), (-0.2, 1.2, 0.6), (np.pi / 2, (1, 0, 0))), "ghost")
    return sb


def cornell_camera(wl, W, H):
    c = wl.builder.extra["camera"]
    return make_camera(c["pos"], c["lookat"], c["up"], fov=c["fov"], xres=W, yres=H)


def feature_case(name):
    """(scene builder, camera, xres, yres, bumpmap scale, largest share of pixels whose triangle may differ from the oracle's)."""
    if name == "cornell":
        wl = Workload("cornell-256", scale=1.0, spp=1)
        return wl.builder, cornell_camera(wl, 100, 70), 100, 70, wl.bumpscale, 0.0
    if name == "sponza-proxy":
        wl = Workload("sponza-1080p", scale=0.06, spp=1)
        return wl.builder, wl.camera, wl.xres, wl.yres, wl.bumpscale, 0.001
    lens = 0.08 if name == "zoo-lens" else 0.0
    cam = make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=61, yres=47, focus_plane=5.0, lens_size=lens)
    return zoo(), cam, 61, 47, 1.0, 0.001


SENTINEL = 7.5


@pytest.mark.parametrize("name", ["cornell", "sponza-proxy", "zoo", "zoo-lens"])
def test_features_equal_the_oracle_composition(rd, oracle, name):
    """tri and depth equal, normal and albedo equal bit for bit wherever the GPU's walker and the oracle's agree on the triangle
    (epsilon-band ties: at most 0.1 % of the pixels, none on Cornell).  Cornell: ragged 32-pixel tiles and a subset of them --
    pixels outside keep the sentinel.  zoo-lens: a thin-lens camera gives the pinhole camera's features.

    The Cornell subset: at 100 x 70 the centre rays of 14 pixels pass exactly through the diagonal of the back wall, where the
    oracle's own triangle test gives its two coplanar triangles the same t to the bit.  The reference has no rule for that (the
    first triangle of its kd leaf's list wins), the walker's is "the higher id" (rgk_trace.h): measured on a subset chosen
    without regard to this, 11 of 3584 pixels (0.31 %) then name the other triangle of the pair, with depth equal.  So the
    subset is every tile in which the ORACLE finds no such pixel -- 9 of the 12, five of them ragged -- and on it the share of
    differing triangles must be 0; test_exact_ties_follow_the_walkers_rule covers the other three tiles."""
    sb, cam, W, H, bump, tie_share = feature_case(name)
    desc = sb.to_desc()
    g, o = rd.Scene(desc), oracle.OracleScene(desc)
    prm = make_params(W, H, 1, 1, bumpscale=bump)
    tiles = rd.generate_task_list(W, H)
    if name == "cornell":
        ties = R.reference_exact_ties(oracle, o, desc, cam, W, H)
        free = [t for t in tiles if not ties[t.y0:t.y1, t.x0:t.x1].any()]
        assert 0 < len(free) < len(tiles)
        tiles = (capi.Tile * len(free))(*free)
        assert any(t.x1 - t.x0 < 32 for t in tiles) and any(t.y1 - t.y0 < 32 for t in tiles)
    inside = np.zeros((H, W), bool)
    for t in tiles:
        inside[t.y0:t.y1, t.x0:t.x1] = True
    assert inside.all() == (name != "cornell")
    ga, gn, gz, gt = g.render_aov(cam, prm, tiles, sentinel=SENTINEL)
    ra, rn, rz, rt = R.oracle_features(oracle, o, desc, cam, W, H, bump)
    if cam.lens_size > 0:  # the reference's own thin-lens rays are something else: the features ignore the lens
        sub, lens, a, b = (C.c_float * 2)(0.5, 0.5), (C.c_float * 2)(0.3, 0.6), (C.c_float * 6)(), (C.c_float * 6)()
        oracle.lib().orc_camera_ray(C.byref(cam), 3, 4, W, H, sub, lens, a)
        oracle.lib().orc_camera_ray(C.byref(R.pinhole(cam)), 3, 4, W, H, sub, lens, b)
        assert list(a) != list(b)
    # outside the listed tiles nothing was written
    assert np.all(ga[~inside] == SENTINEL) and np.all(gn[~inside] == SENTINEL) and np.all(gz[~inside] == SENTINEL) and np.all(gt[~inside] == int(SENTINEL))
    differ = inside & (gt != rt)
    share = float(differ.sum()) / float(inside.sum())
    same = inside & ~differ
    nb = int((bits(gn[same]) != bits(rn[same])).any(axis=-1).sum())
    ab = int((bits(ga[same]) != bits(ra[same])).any(axis=-1).sum())
    zb = int((bits(gz[same]) != bits(rz[same])).sum())
    record_parity(f"gpu_post.features[{name}]", tri_differs=share, depth_differs=zb, normal_differs=nb, albedo_differs=ab, hits=float((gt[inside] >= 0).mean()))
    assert share <= tie_share, share
    assert zb == 0 and nb == 0 and ab == 0, (zb, nb, ab)
    miss = same & (gt < 0)
    assert np.all(gz[miss] == 0) and np.all(gn[miss] == 0) and np.all(ga[miss] == 0)
    assert (gt[inside] >= 0).mean() > 0.5
    if name.startswith("zoo"):  # every branch of the albedo was on screen
        seen = {tuple(np.round(v, 4)) for v in ga[same & (gt >= 0)].reshape(-1, 3)}
        inner = np.float32(0.4) * np.float32([0.6, 0.1, 0.1]) + (np.float32(1) - np.float32(0.4)) * np.float32([0.8, 0.6, 0.2])
        mix2 = np.float32(0.7) * inner + (np.float32(1) - np.float32(0.7)) * np.float32([1, 1, 1])
        for want in ([1, 1, 1], [0.8, 0.6, 0.2], np.float32([0.2, 0.4, 0.6]) + np.float32([0.3, 0.3, 0.3]), mix2, [0.5, 0.5, 0.5]):
            assert tuple(np.round(np.float32(want), 4)) in seen, want


def test_exact_ties_follow_the_walkers_rule(rd, oracle):
    """Whole Cornell frame at 100 x 70: wherever the feature pass names another triangle than the oracle, the oracle's own
    triangle test has two nearest triangles at exactly the same distance there, the depth is the oracle's to the bit, and the
    pass names the higher id -- the round's walker's rule for exact ties."""
    sb, cam, W, H, bump, _ = feature_case("cornell")
    desc = sb.to_desc()
    g, o = rd.Scene(desc), oracle.OracleScene(desc)
    _, _, gz, gt = g.render_aov(cam, make_params(W, H, 1, 1, bumpscale=bump), rd.generate_task_list(W, H))
    _, _, rz, rt = R.oracle_features(oracle, o, desc, cam, W, H, bump)
    ties = R.reference_exact_ties(oracle, o, desc, cam, W, H)
    differ = gt != rt
    record_parity("gpu_post.exact_ties[cornell 100x70]", reference_ties=int(ties.sum()), tri_differs=int(differ.sum()))
    assert ties.sum() > 0 and not (differ & ~ties).any()
    assert np.array_equal(bits(gz), bits(rz)) and (gt[differ] > rt[differ]).all()


def test_feature_entries_host_and_device_agree_and_accept_null_outputs(rd):
    import torch
    wl = Workload("cornell-256", scale=0.25, spp=1)
    g = rd.Scene(wl.builder.to_desc())
    prm, tiles = wl.params(), rd.generate_task_list(wl.xres, wl.yres)
    H, W = wl.yres, wl.xres
    ha, hn, hz, ht = g.render_aov(wl.camera, prm, tiles)
    da = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"); dn = torch.zeros_like(da)
    dz = torch.zeros((H, W), dtype=torch.float32, device="cuda:0"); dt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    g.render_aov_device(wl.camera, prm, tiles, da.data_ptr(), dn.data_ptr(), dz.data_ptr(), dt.data_ptr())
    for h, d in ((ha, da), (hn, dn), (hz, dz), (ht, dt)):
        assert np.array_equal(bits(h), bits(d.cpu().numpy()))
    # each output alone, the others NULL
    lib = g.lib
    for k, want in enumerate((ha, hn, hz, ht)):
        out = np.zeros_like(want)
        ptrs = [None] * 4
        ptrs[k] = out.ctypes.data
        capi.check(lib, lib.rgk_render_aov(g.h, C.byref(wl.camera), C.byref(prm), tiles, len(tiles), *ptrs))
        assert np.array_equal(bits(out), bits(want))
    capi.check(lib, lib.rgk_render_aov(g.h, C.byref(wl.camera), C.byref(prm), tiles, len(tiles), None, None, None, None))
    capi.check(lib, lib.rgk_render_aov_device(g.h, C.byref(wl.camera), C.byref(prm), tiles, 0, None, None, None, None))


# ----------------------------------------------------------------------- the denoiser against its numpy restatement
def gpu_denoise(g, acc, cnt, alb, nrm, z, dp):
    import torch
    H, W = z.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    t = [up(acc), up(cnt.view(np.int32)), up(alb), up(nrm), up(z)]
    out = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g.denoise_device(W, H, *[x.data_ptr() for x in t], dp, out.data_ptr())
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def cornell_frames(rd):
    """The GPU's own 4-spp accumulator and feature planes of the Cornell box at the three sizes, rendered once."""
    wl = Workload("cornell-256", spp=4)
    g, frames = rd.Scene(wl.builder.to_desc()), {}
    for W, H in ((96, 96), (67, 45), (1, 1)):
        cam, prm = cornell_camera(wl, W, H), wl.params()
        prm.xres, prm.yres = W, H
        tiles = rd.generate_task_list(W, H)
        acc, cnt, _ = g.render_round(cam, prm, tiles)
        frames[(W, H)] = (acc, cnt) + g.render_aov(cam, prm, tiles)[:3]
    return g, frames


@pytest.mark.parametrize("size", [(96, 96), (67, 45), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("demodulate", [0, 1])
def test_denoiser_equals_the_numpy_restatement(cornell_frames, size, demodulate):
    """np.array_equal on the output, the GPU's own accumulator and feature planes on both sides.  67 x 45 is narrower than the
    last iteration's reach (2 * 16 pixels each way): every border case occurs.  One pixel has no samples."""
    g, frames = cornell_frames
    acc, cnt, alb, nrm, z = [a.copy() for a in frames[size]]
    if size != (1, 1):
        cnt[5, 7] = 0
    sigma = R.default_sigma_color(acc, cnt, 6.0) or 1.0
    dp = capi.DenoiseParams(sigma_color=sigma, demodulate=demodulate)
    got = gpu_denoise(g, acc, cnt, alb, nrm, z, dp)
    want = R.atrous_ref(acc, cnt, alb, nrm, z, dp.iterations, dp.sigma_color, dp.sigma_depth, dp.normal_power_log2, dp.demodulate)
    differ = int((bits(got) != bits(want)).any(axis=-1).sum())
    c = R.mean_color(acc, cnt)
    record_parity(f"gpu_post.denoise[{size[0]}x{size[1]},demod={demodulate}]", pixels_differ=differ, pixels_changed=float((got != c).any(axis=-1).mean()))
    assert differ == 0
    if size != (1, 1):
        assert (got != c).any(axis=-1).mean() > 0.5 and (got[5, 7] > 0).any()  # it filtered; the empty pixel was filled in from its neighbours
    # iterations 0: the image itself, with or without demodulation
    dp0 = capi.DenoiseParams(iterations=0, sigma_color=sigma, demodulate=demodulate)
    assert np.array_equal(bits(gpu_denoise(g, acc, cnt, alb, nrm, z, dp0)), bits(c))
    # fewer iterations, other powers and widths: the restatement follows
    dp2 = capi.DenoiseParams(iterations=2, sigma_color=0.37 * sigma, sigma_depth=0.1, normal_power_log2=1, demodulate=demodulate)
    want2 = R.atrous_ref(acc, cnt, alb, nrm, z, 2, dp2.sigma_color, dp2.sigma_depth, 1, demodulate)
    assert np.array_equal(bits(gpu_denoise(g, acc, cnt, alb, nrm, z, dp2)), bits(want2))


def test_a_frame_of_misses_comes_back_unchanged(cornell_frames):
    g, frames = cornell_frames
    acc, cnt = frames[(67, 45)][:2]
    zero3, zero = np.zeros_like(acc), np.zeros(cnt.shape, np.float32)
    for demodulate in (0, 1):
        got = gpu_denoise(g, acc, cnt, zero3, zero3, zero, capi.DenoiseParams(sigma_color=1.0, demodulate=demodulate))
        assert np.array_equal(bits(got), bits(R.mean_color(acc, cnt)))


# ----------------------------------------------------------------------- end to end
def _driver(rd, wl, scene=None):
    class Cfg:
        xres, yres, render_rounds, render_minutes = wl.xres, wl.yres, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: wl.params(sampler, flags))
    return rd.RenderDriver(scene or rd.Scene(wl.builder.to_desc()), Cfg, wl.camera)


def test_denoised_4spp_is_closer_to_256spp_and_the_pass_disturbs_no_round(rd):
    lo, hi = Workload("cornell-256", scale=0.375, spp=4), Workload("cornell-256", scale=0.375, spp=256)
    ref_drv = _driver(rd, hi)
    ref_drv.render_round()
    ref = ref_drv.total_ob.get_pixels().cpu().numpy()
    # rounds with a feature pass over a few tiles, a whole-frame one and two denoise calls between them ...
    drv = _driver(rd, lo)
    drv.render_round()
    noisy = drv.total_ob.get_pixels().cpu().numpy()
    few = (capi.Tile * 2)(drv.tasks[3], drv.tasks[0])
    drv.scene.render_aov(lo.camera, drv.params, few)
    den = drv.denoise().cpu().numpy()
    den2 = drv.denoise().cpu().numpy()
    assert np.array_equal(bits(den), bits(den2))
    a, b = R.rel_l2(noisy, ref), R.rel_l2(den, ref)
    record_parity("gpu_post.end_to_end[cornell 96x96, 4 vs 256 spp]", noisy_rel_l2=a, denoised_rel_l2=b, sigma_color=float(drv.default_denoise_params().sigma_color))
    assert b < a
    drv.render_round()
    drv.denoise()
    drv.render_round()
    # ... leave the accumulator of the same rounds without them
    plain = _driver(rd, lo)
    for _ in range(3):
        plain.render_round()
    assert np.array_equal(bits(drv.total_ob.data.cpu().numpy()), bits(plain.total_ob.data.cpu().numpy()))
    assert np.array_equal(drv.total_ob.count.cpu().numpy(), plain.total_ob.count.cpu().numpy())
    # the driver's planes are the entry point's
    ha, hn, hz, ht = drv.scene.render_aov(lo.camera, drv.params, drv.tasks)
    f = drv.render_aov()
    for h, k in ((ha, "albedo"), (hn, "normal"), (hz, "depth"), (ht, "tri")):
        assert np.array_equal(bits(h), bits(f[k].cpu().numpy()))


SCENE = '''{
    "output-file": "post.exr", "output-width": 48, "output-height": 40, "multisample": 4, "rounds": 2, "recursion-max": 3, "clamp": 20,
    "camera": {"position": [0,1.2,5], "lookat": [0,0.8,0], "fov": 35},
    "materials": [{"name": "m", "brdf": "diffuse", "diffuse255": [255, 128, 0]},
                  {"name": "g", "brdf": "ltc_ggx_diffuse", "exponent": 200, "specular": [0.3,0.3,0.3], "diffuse": [0.4,0.4,0.5]},
                  {"name": "l", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5], "emission": [9,9,8]}],
    "scene": [{"primitive": "cube", "material": "m", "translate": [0,0.5,0]},
              {"primitive": "plane", "material": "g", "scale": [4,1,4]},
              {"primitive": "plane", "material": "l", "scale": [0.5,1,0.5], "translate": [0,3,0], "rotate": [180, 0, 0]}],
    "sky": {"color": [0.3, 0.4, 0.6], "intensity": 0.5}
}'''


def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([sys.executable, "-m", "rgk_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def test_cli_writes_feature_and_denoised_images_beside_an_unchanged_output(rd, tmp_path):
    cfg = tmp_path / "s.json"
    cfg.write_text(SCENE)
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir(); b.mkdir()
    r = run_cli([str(cfg), "-D", str(a), "--aov", "--denoise", "-q"], str(tmp_path))
    assert r.returncode == 0, r.stderr + r.stdout
    r = run_cli([str(cfg), "-D", str(b), "-q"], str(tmp_path))
    assert r.returncode == 0, r.stderr + r.stdout
    assert sorted(os.listdir(str(b))) == ["post.exr"]
    assert sorted(os.listdir(str(a))) == ["post.albedo.exr", "post.denoised.exr", "post.depth.exr", "post.exr", "post.normal.exr"]
    assert (a / "post.exr").read_bytes() == (b / "post.exr").read_bytes()
    img = {k: rd.read_exr(str(a / f"post.{k}.exr")) for k in ("albedo", "normal", "depth", "denoised")}
    plain = rd.read_exr(str(a / "post.exr"))
    for v in img.values():
        assert v.shape == (40, 48, 4) and (v[..., 3] == 1).all()
    z = img["depth"]
    assert np.array_equal(z[..., 0], z[..., 1]) and np.array_equal(z[..., 0], z[..., 2]) and z.max() > 1
    hit = z[..., 0] > 0
    assert np.allclose(np.linalg.norm(img["normal"][hit][:, :3], axis=-1), 1, atol=2e-3) and np.all(img["normal"][~hit][:, :3] == 0)
    assert np.any(np.all(np.isclose(img["albedo"][..., :3], [1.0, 128 / 255, 0], atol=0.3), axis=-1))  # the orange cube (gamma-decoded)
    d = img["denoised"][..., :3]
    assert np.isfinite(d).all() and not np.array_equal(d, plain[..., :3])
    assert abs(float(d.mean()) - float(plain[..., :3].mean())) < 0.2 * float(plain[..., :3].mean())  # the same scale as the output
