"""GPU suite (-m gpu): feature planes that follow mirrors and glass (rgk_render_aov_chain[_device], k_aov_hop) against the
composition of their definition from oracle primitives (tests/chain_ref.py), bit for bit and with no pixel left out; against
rgk_render_aov_device at max_hops = 0; across tree builders; between rounds; in the denoiser; and through the command line."""
import ctypes as C
import os

import numpy as np
import pytest

from rgk_amd import capi

import chain_ref as CR
import post_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case(name):
    """(builder, camera, params of one sample, xres, yres)"""
    if name == "hall":
        return CR.hall(), CR.hall_camera(), CR.hall_params(), CR.HALL_W, CR.HALL_H
    sb, cam, W, H, _, wl = CR.spheres_case()
    return sb, cam, wl.params(), W, H


@pytest.fixture(scope="module")
def scenes(rd):
    """One device scene per case, built once: {name: (scene, camera, params, tiles, builder)}."""
    out = {}
    for name in ("hall", "spheres"):
        sb, cam, prm, W, H = case(name)
        out[name] = (rd.Scene(sb.to_desc()), cam, prm, rd.generate_task_list(W, H), sb)
    return out


def same_planes(got, want):
    """Pixels that differ, per plane: albedo, normal, depth as float32 bits; tri and hops as integers."""
    return [int((bits(g) != bits(w)).reshape(g.shape[0], g.shape[1], -1).any(axis=-1).sum()) for g, w in zip(got[:3], want[:3])] + \
           [int((g != w).sum()) for g, w in zip(got[3:5], want[3:5])]


# ----------------------------------------------------------------------- 1. parity with the composition
@pytest.mark.parametrize("name,max_hops", [("hall", 0), ("hall", 1), ("hall", 2), ("hall", 4), ("hall", 8), ("spheres", 4)])
def test_planes_equal_the_composition_bit_for_bit(scenes, oracle, name, max_hops):
    """tri and hops array_equal, depth / normal / albedo array_equal as float32 bits, every pixel of the frame."""
    g, cam, prm, tiles, _ = scenes[name]
    ch, _, _ = CR.reference(name)
    want = CR.planes(ch, max_hops)
    got = g.render_aov_chain(cam, prm, tiles, max_hops, sentinel=SENTINEL)
    differ = same_planes(got, want)
    record_parity(f"gpu_aov_chain.parity[{name}, max_hops {max_hops}]", albedo_differs=differ[0], normal_differs=differ[1], depth_differs=differ[2],
                  tri_differs=differ[3], hops_differs=differ[4], followed=float((want[4] > 0).mean()))
    assert got[3].dtype == np.int32 and got[4].dtype == np.uint8
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert differ == [0, 0, 0, 0, 0], differ
    assert (want[4] > 0).any() == (max_hops > 0)


# ----------------------------------------------------------------------- 2. max_hops = 0 is the first-hit pass
def test_max_hops_0_equals_the_first_hit_entry_outside_tiles_null_outputs_host_and_device(scenes):
    import torch
    g, cam, prm, tiles, _ = scenes["hall"]
    W, H = prm.xres, prm.yres
    few = (capi.Tile * 2)(tiles[3], tiles[0])  # a partial list, one of its tiles ragged (48 rows = 32 + 16)
    assert any(t.y1 - t.y0 < 32 for t in tiles)
    inside = np.zeros((H, W), bool)
    for t in few:
        inside[t.y0:t.y1, t.x0:t.x1] = True
    assert inside.any() and not inside.all()
    for tl in (tiles, few):
        first = g.render_aov(cam, prm, tl, sentinel=SENTINEL)
        got = g.render_aov_chain(cam, prm, tl, 0, sentinel=SENTINEL)
        for a, b in zip(got[:4], first):
            assert np.array_equal(bits(a), bits(b))
        where = inside if tl is few else np.ones((H, W), bool)
        assert (got[4][where] == 0).all() and (got[4][~where] == int(SENTINEL)).all()
    # followed planes: nothing is written outside the listed tiles either
    got = g.render_aov_chain(cam, prm, few, 4, sentinel=SENTINEL)
    full = g.render_aov_chain(cam, prm, tiles, 4)
    for a, b in zip(got, full):
        assert (a[~inside] == np.asarray(SENTINEL).astype(a.dtype)).all() and np.array_equal(a[inside], b[inside])
    assert (full[4][inside] > 0).any()
    # device entry against host entry
    dev = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"),
           torch.zeros((H, W), dtype=torch.float32, device="cuda:0"), torch.zeros((H, W), dtype=torch.int32, device="cuda:0"),
           torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")]
    torch.cuda.synchronize()
    g.render_aov_chain_device(cam, prm, tiles, 4, *[d.data_ptr() for d in dev])
    for h, d in zip(full, dev):
        assert np.array_equal(h, d.cpu().numpy()) and (h.dtype.kind != "f" or np.array_equal(bits(h), bits(d.cpu().numpy())))
    # each output alone, the others NULL; all NULL; no tiles
    lib = g.lib
    for k, want in enumerate(full):
        out = np.zeros_like(want)
        ptrs = [None] * 5
        ptrs[k] = out.ctypes.data
        capi.check(lib, lib.rgk_render_aov_chain(g.h, C.byref(cam), C.byref(prm), tiles, len(tiles), 4, *ptrs))
        assert np.array_equal(out, want)
    capi.check(lib, lib.rgk_render_aov_chain(g.h, C.byref(cam), C.byref(prm), tiles, len(tiles), 8, None, None, None, None, None))
    capi.check(lib, lib.rgk_render_aov_chain_device(g.h, C.byref(cam), C.byref(prm), tiles, 0, 8, None, None, None, None, None))


# ----------------------------------------------------------------------- 3. nothing to follow
def test_a_scene_without_delta_materials_gives_the_first_hit_planes(rd):
    from rgk_amd.workloads import SceneFixture
    wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_box6.npz"), scale=0.1, spp=1)
    assert not any(m["kind"] in CR.DELTA for m in wl.builder.materials)
    g = rd.Scene(wl.builder.to_desc())
    prm, tiles = wl.params(), rd.generate_task_list(wl.xres, wl.yres)
    first = g.render_aov(wl.camera, prm, tiles)
    got = g.render_aov_chain(wl.camera, prm, tiles, 8, sentinel=SENTINEL)
    for a, b in zip(got[:4], first):
        assert np.array_equal(bits(a), bits(b))
    assert (got[4] == 0).all() and (first[3] >= 0).mean() > 0.5


# ----------------------------------------------------------------------- 4. tree independence
def test_planes_do_not_depend_on_the_tree_builder(rd, scenes):
    _, cam, prm, tiles, _ = scenes["hall"]
    got = {}
    for flag in (capi.BUILD_HOST_SAH, capi.BUILD_DEVICE):
        sb = CR.hall()
        sb.build_flags = flag
        got[flag] = rd.Scene(sb.to_desc()).render_aov_chain(cam, prm, tiles, 8)
    for a, b in zip(got[capi.BUILD_HOST_SAH], got[capi.BUILD_DEVICE]):
        assert np.array_equal(a, b) and (a.dtype.kind != "f" or np.array_equal(bits(a), bits(b)))


# ----------------------------------------------------------------------- 5. rounds undisturbed
def test_a_chain_call_between_two_rounds_changes_neither(rd):
    sb, cam, _, W, H = case("hall")
    prm = CR.hall_params(spp=4)
    desc = sb.to_desc()
    tiles0, tiles1 = rd.generate_task_list(W, H, rd.SEEDSTART, 0), rd.generate_task_list(W, H, rd.SEEDSTART, 4)
    out = []
    for with_call in (True, False):
        g = rd.Scene(desc)
        acc, cnt, _ = g.render_round(cam, prm, tiles0)
        if with_call:
            g.render_aov_chain(cam, prm, tiles0, 8)
            g.render_aov_chain(cam, prm, (capi.Tile * 1)(tiles0[2]), 2)
        g.render_round(cam, prm, tiles1, acc, cnt)
        out.append((acc, cnt))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])
    assert out[0][1].min() == 8


# ----------------------------------------------------------------------- 6. it helps where it should
def gpu_denoise(g, acc, cnt, alb, nrm, z, dp):
    import torch
    H, W = z.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    t = [up(acc), up(cnt.view(np.int32)), up(alb), up(nrm), up(z)]
    out = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g.denoise_device(W, H, *[x.data_ptr() for x in t], dp, out.data_ptr())
    return out.cpu().numpy()


def test_followed_planes_denoise_the_reflected_floor_better_than_first_hit_planes(scenes):
    """The hall at 4 spp through rgk_denoise_device (shipped defaults), once with the first-hit planes and once with the followed
    planes (max_hops = 4); relative L2 against 256 spp over the pixels with hops > 0 whose chain ends on the textured floor.  The
    yardstick is the first-hit planes' error: the followed planes' must be below it.
    Measured -- CPU (oracle images, composed planes, numpy filter) and GPU -- in profiles/aov_chain_quality.txt."""
    g, cam, _, tiles, sb = scenes["hall"]
    acc, cnt, _ = g.render_round(cam, CR.hall_params(spp=4), tiles)
    racc, rcnt, _ = g.render_round(cam, CR.hall_params(spp=256), tiles)
    ref = R.mean_color(racc, rcnt)
    first, follow = g.render_aov_chain(cam, CR.hall_params(), tiles, 0), g.render_aov_chain(cam, CR.hall_params(), tiles, 4)
    region = (follow[4] > 0) & np.isin(follow[3], list(sb.parts["floor"]))
    assert region.sum() > 300
    dp = capi.DenoiseParams(sigma_color=R.default_sigma_color(acc, cnt, 6.0))
    err = {}
    for tag, f in (("first-hit", first), ("followed", follow)):
        den = gpu_denoise(g, acc, cnt, f[0], f[1], f[2], dp)
        err[tag] = float(np.linalg.norm(den[region].astype(np.float64) - ref[region]) / np.linalg.norm(ref[region].astype(np.float64)))
    noisy = R.mean_color(acc, cnt)
    err["unfiltered"] = float(np.linalg.norm(noisy[region].astype(np.float64) - ref[region]) / np.linalg.norm(ref[region].astype(np.float64)))
    print("relative L2 on the followed floor pixels:", err)
    record_parity("gpu_aov_chain.quality[hall, 4 vs 256 spp]", pixels=int(region.sum()), unfiltered=err["unfiltered"], first_hit=err["first-hit"], followed=err["followed"])
    assert err["followed"] < err["first-hit"], err


# ----------------------------------------------------------------------- 7. command line and driver
SCENE = '''{
    "output-file": "hall.exr", "output-width": 48, "output-height": 40, "multisample": 4, "rounds": 2, "recursion-max": 4, "clamp": 20,
    "camera": {"position": [0,1.6,5], "lookat": [0,0.6,0], "fov": 40},
    "materials": [{"name": "m", "brdf": "diffuse", "diffuse255": [255, 128, 0]},
                  {"name": "f", "brdf": "diffuse", "diffuse": [0.5,0.6,0.4]},
                  {"name": "s", "brdf": "mirror"},
                  {"name": "l", "brdf": "diffuse", "diffuse": [0.5,0.5,0.5], "emission": [9,9,8]}],
    "scene": [{"primitive": "cube", "material": "m", "translate": [0.8,0.5,1]},
              {"primitive": "plane", "material": "f", "scale": [4,1,4]},
              {"primitive": "plane", "material": "s", "scale": [1.5,1,1], "translate": [-0.5,1,-1.5], "rotate": [-90, 0, 0]},
              {"primitive": "plane", "material": "l", "scale": [0.5,1,0.5], "translate": [0,3,0], "rotate": [180, 0, 0]}],
    "sky": {"color": [0.3, 0.4, 0.6], "intensity": 0.5}
}'''


def test_cli_writes_hops_and_followed_planes_beside_an_unchanged_output(rd, tmp_path):
    from test_gpu_post import run_cli
    cfg = tmp_path / "s.json"
    cfg.write_text(SCENE)
    dirs = {k: tmp_path / k for k in ("hops", "plain")}
    for d in dirs.values():
        d.mkdir()
    for k, extra in (("hops", ["--aov", "--denoise", "--aov-hops", "4"]), ("plain", ["--aov", "--denoise"])):
        r = run_cli([str(cfg), "-D", str(dirs[k]), "-q"] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr + r.stdout
    plain_files = ["hall.albedo.exr", "hall.denoised.exr", "hall.depth.exr", "hall.exr", "hall.normal.exr"]
    assert sorted(os.listdir(str(dirs["plain"]))) == plain_files  # without the switch: the files the command has always written
    assert sorted(os.listdir(str(dirs["hops"]))) == sorted(plain_files + ["hall.hops.exr"])
    assert (dirs["hops"] / "hall.exr").read_bytes() == (dirs["plain"] / "hall.exr").read_bytes()
    hops = rd.read_exr(str(dirs["hops"] / "hall.hops.exr"))
    assert hops.shape == (40, 48, 4) and np.array_equal(hops[..., 0], hops[..., 1]) and np.array_equal(hops[..., 0], hops[..., 2])
    assert set(np.unique(hops[..., 0])) == {0.0, 1.0}
    seen = hops[..., 0] == 1
    z1, z0 = rd.read_exr(str(dirs["hops"] / "hall.depth.exr"))[..., 0], rd.read_exr(str(dirs["plain"] / "hall.depth.exr"))[..., 0]
    assert np.array_equal(z1[~seen], z0[~seen]) and (z1[seen & (z1 > 0)] > z0[seen & (z1 > 0)]).all() and (seen & (z1 > 0)).any()
    a1, a0 = rd.read_exr(str(dirs["hops"] / "hall.albedo.exr"))[..., :3], rd.read_exr(str(dirs["plain"] / "hall.albedo.exr"))[..., :3]
    assert (a0[seen] == 1).all() and (a1[seen] != 1).any()
    assert (dirs["hops"] / "hall.denoised.exr").read_bytes() != (dirs["plain"] / "hall.denoised.exr").read_bytes()


def test_driver_feeds_the_followed_planes_to_the_filters(rd, scenes):
    import torch
    g, cam, _, tiles, _ = scenes["hall"]
    prm4 = CR.hall_params(spp=4)

    class Cfg:
        xres, yres, render_rounds, render_minutes = CR.HALL_W, CR.HALL_H, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: capi.Params.from_buffer_copy(prm4))
    drv = rd.RenderDriver(g, Cfg, cam, aov_hops=4, track_noise=True)
    plain = rd.RenderDriver(g, Cfg, cam, track_noise=True)
    for d in (drv, plain):
        d.render_round()
        d.render_round()
    want = g.render_aov_chain(cam, prm4, tiles, 4)
    f = drv.render_aov()
    for h, k in zip(want, ("albedo", "normal", "depth", "tri", "hops")):
        assert np.array_equal(h, f[k].cpu().numpy())
    assert np.array_equal(drv.aov_hops_plane().cpu().numpy(), want[4]) and (plain.aov_hops_plane() == 0).all() and "hops" not in plain.render_aov()
    assert np.array_equal(bits(drv.total_ob.data.cpu().numpy()), bits(plain.total_ob.data.cpu().numpy()))
    dp = drv.default_denoise_params()
    acc, cnt = drv.total_ob.data.cpu().numpy(), drv.total_ob.count.cpu().numpy().view(np.uint32)
    assert np.array_equal(bits(drv.denoise(dp).cpu().numpy()), bits(gpu_denoise(g, acc, cnt, want[0], want[1], want[2], dp)))
    assert not torch.equal(drv.denoise(dp), plain.denoise(dp))
    assert not torch.equal(drv.denoise_variance()[0], plain.denoise_variance()[0])
    assert drv.noise()["rel"] == plain.noise()["rel"]  # the estimate reads no feature plane
