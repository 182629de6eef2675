"""Per-sample demodulated accumulation without a GPU: the restatement's pieces (tests/demod_ref.py) against the feature pass's
restatement and known answers, the two entries' argument refusals, and the command line's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.workloads import SceneFixture

import demod_ref as D
import post_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, UNSUPPORTED = -1, -5


def test_status_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    assert int(re.search(r"RGK_ERR_INVALID\s*=\s*(-?\d+)", hdr).group(1)) == INVALID
    assert int(re.search(r"RGK_ERR_UNSUPPORTED\s*=\s*(-?\d+)", hdr).group(1)) == UNSUPPORTED


def test_centre_ray_divisors_are_the_feature_albedo_through_the_floor_rule(oracle):
    """scene_rubiks-bump at 16 x 16 (textured, bump mapped): with every sample's ray put through the pixel centre, div_s equals
    post_ref.oracle_features' albedo through the floor rule for every s, and A = multisample x that, summed in float32."""
    O = oracle
    wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_rubiks-bump.npz"), scale=16 / 1200, spp=3)
    wl.xres = wl.yres = 16
    from rgk_amd.config import make_camera
    c = wl.builder.extra["camera"]
    cam = make_camera(c["pos"], c["lookat"], c["up"], fov=c.get("fov"), focal=c.get("focal"), xres=16, yres=16)
    desc = wl.builder.to_desc()
    osc = O.OracleScene(desc)
    albedo, _, _, tri = PR.oracle_features(O, osc, desc, cam, 16, 16, wl.bumpscale)
    assert (tri >= 0).mean() > 0.1 and (tri < 0).any() and len(np.unique(albedo.reshape(-1, 3), axis=0)) > 4, "the frame must see several texture colours and sky"
    tiles = O.generate_task_list(16, 16)
    for floor in (0.0, 0.02, 0.25):
        div, covered = D.sample_divisors(O, osc, desc, cam, tiles, 16, 16, 3, floor, centre=True, trace=osc.trace_closest)
        assert covered.all()
        want = D.floor_rule(albedo, floor)
        want[tri < 0] = 1.0
        for s in range(3):
            assert np.array_equal(div[:, :, s], want), (floor, s)
        A = D.divisor_sum(div, covered)
        assert np.array_equal(A, ((want + want).astype(F) + want).astype(F))
    # (the jittered rays are other rays: the divisors move with them)
    div_j, _ = D.sample_divisors(O, osc, desc, cam, tiles, 16, 16, 3, 0.02)
    assert not np.array_equal(div_j[:, :, 0], div_j[:, :, 1])


def test_pixel_seeds_follow_the_tile_order():
    tiles = (capi.Tile * 2)()
    tiles[0].x0, tiles[0].x1, tiles[0].y0, tiles[0].y1, tiles[0].seed = 1, 4, 0, 2, 42
    tiles[1].x0, tiles[1].x1, tiles[1].y0, tiles[1].y1, tiles[1].seed = 0, 1, 1, 2, 0xFFFFFFF0
    seed, covered = D.pixel_seeds(tiles, 4, 2)
    assert covered.tolist() == [[False, True, True, True], [True, True, True, True]]
    assert int(seed[0, 1]) == (42 + 0x42424242) & 0xFFFFFFFF and int(seed[1, 3]) == (42 + 6 * 0x42424242) & 0xFFFFFFFF
    assert int(seed[1, 0]) == (0xFFFFFFF0 + 0x42424242) & 0xFFFFFFFF


def test_remodulate_known_answers():
    img = np.array([[[2.0, 4.0, 8.0], [1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]], F)
    # a count plane: A / n, 1 where the count is 0
    A = np.array([[[1.0, 2.0, 3.0], [9.0, 9.0, 9.0], [0.0, 1.5, 6.0]]], F)
    n = np.array([[4, 0, 3]], np.uint32)
    out = D.remodulate(img, A, n)
    assert out.dtype == F
    assert out.tolist() == [[[0.5, 2.0, 6.0], [1.0, 1.0, 1.0], [0.0, 1.5, 6.0]]]
    # an albedo plane: zero and negative albedo multiply by 1, a small one by the floor
    alb = np.array([[[0.0, -0.5, 0.01], [0.5, 0.02, 2.0], [0.25, 0.0, 1e-30]]], F)
    out = D.remodulate(img, alb, None, albedo_floor=0.25)
    assert out.tolist() == [[[2.0, 4.0, 2.0], [0.5, 0.25, 2.0], [0.75, 3.0, 0.75]]]
    assert D.remodulate(img, alb, None, albedo_floor=0.0).tolist() == [[[2.0, 4.0, float(F(8.0) * F(0.01))], [0.5, float(F(0.02)), 2.0], [0.75, 3.0, float(F(3.0) * F(1e-30))]]]
    assert D.floor_rule([np.nan], 0.02).tolist() == [1.0]  # (not > 0)


def test_uniform_albedo_copy():
    wl = SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_box6.npz"))
    sb = D.uniform_albedo(wl.builder, 0.5)
    assert len(sb.materials) == len(wl.builder.materials) and all(m["kind"] == capi.BXDF_DIFFUSE for m in sb.materials)
    assert all(sb.textures[m["tex_diffuse"]]["color"] == (0.5, 0.5, 0.5) for m in sb.materials)
    assert [m["emission"] for m in sb.materials] == [m["emission"] for m in wl.builder.materials] and any(max(m["emission"]) > 0 for m in sb.materials)
    assert sb.sky["color"] == (0.0, 0.0, 0.0) and sb.areal == wl.builder.areal and sb.pointlights == wl.builder.pointlights
    assert any(m["kind"] != capi.BXDF_DIFFUSE for m in wl.builder.materials), "the source is left as it was"


# ----------------------------------------------------------------------- the entries' own argument checks need no GPU
def test_the_binding_matches_the_header(product_lib):
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    assert set(re.findall(r"\b(rgk_[a-z_]+)\s*\(", hdr)) == set(capi.EXPORTS)
    for name, n_args in (("rgk_render_round_demod_device", 11), ("rgk_remodulate_device", 8)):
        assert name in capi.EXPORTS and getattr(product_lib, name) is not None
        proto = re.search(r"int %s\s*\(([^;]*)\);" % name, hdr).group(1)
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]
        assert len(args) == len(getattr(product_lib, name).argtypes) == n_args, name


def test_argument_errors_need_no_gpu(product_lib):
    lib = product_lib
    fake = C.create_string_buffer(64)  # a `scene` that is 64 bytes of nothing: every refusal below comes before it is touched
    scene = C.cast(fake, C.c_void_p)
    bufs = [np.zeros(8 * 8 * 3, F) for _ in range(5)]
    p = [b.ctypes.data for b in bufs]
    cam, prm, cnt = capi.Camera(), capi.Params(), capi.Counters()
    prm.xres = prm.yres = 8
    prm.multisample, prm.depth = 1, 2
    tiles = (capi.Tile * 1)()
    tiles[0].x1 = tiles[0].y1 = 8

    def round_(**kw):
        a = dict(scene=scene, cam=C.byref(cam), prm=C.byref(prm), tiles=tiles, n=1, acc=p[0], count=p[1], demod=p[2], div=p[3], floor=0.02)
        a.update(kw)
        return lib.rgk_render_round_demod_device(a["scene"], a["cam"], a["prm"], a["tiles"], a["n"], a["acc"], a["count"], a["demod"], a["div"], a["floor"], C.byref(cnt))
    for k in ("demod", "div", "acc", "count", "scene", "cam", "prm"):
        assert round_(**{k: None}) == INVALID and b"null" in lib.rgk_last_error(), k
    for v in (-0.01, float("nan"), float("inf"), -float("inf")):
        assert round_(floor=v) == INVALID and b"albedo_floor" in lib.rgk_last_error(), v
    for a, b in (("demod", "div"), ("demod", "acc"), ("div", "acc"), ("demod", "count"), ("div", "count")):
        assert round_(**{a: p[4], b: p[4]}) == INVALID and b"different" in lib.rgk_last_error(), (a, b)
    prm.reverse = 1
    assert round_() == UNSUPPORTED and b"reverse" in lib.rgk_last_error()
    prm.reverse = 0
    # what the plain entry refuses, with its status
    plain = lambda: lib.rgk_render_round_device(scene, C.byref(cam), C.byref(prm), tiles, 1, p[0], p[1], C.byref(cnt))
    for field, value in (("multisample", 0), ("xres", 0), ("xres", 70000), ("depth", 63), ("sampler", capi.SAMPLER_STRATIFIED)):
        keep = getattr(prm, field)
        setattr(prm, field, value)
        want = plain()
        assert want in (INVALID, UNSUPPORTED) and round_() == want, (field, value)
        setattr(prm, field, keep)

    def remod(**kw):
        a = dict(scene=scene, x=8, y=8, src=p[0], div=p[1], count=p[2], floor=0.02, out=p[3])
        a.update(kw)
        return lib.rgk_remodulate_device(a["scene"], a["x"], a["y"], a["src"], a["div"], a["count"], a["floor"], a["out"])
    for k in ("scene", "src", "div", "out"):
        assert remod(**{k: None}) == INVALID and b"null" in lib.rgk_last_error(), k
    for v in (-1.0, float("nan"), float("inf")):
        assert remod(floor=v) == INVALID and b"albedo_floor" in lib.rgk_last_error(), v
        assert remod(floor=v, count=None) == INVALID
    for k, v in (("x", 0), ("y", 0), ("x", 65536), ("y", 70000)):
        assert remod(**{k: v}) == INVALID and b"resolution" in lib.rgk_last_error(), (k, v)
    for k in ("src", "div", "count"):
        assert remod(**{k: p[3]}) == INVALID and b"output" in lib.rgk_last_error(), k
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(scene, 10, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(scene, 9, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


# ----------------------------------------------------------------------- driver and command line
class Cfg:
    xres, yres, render_rounds, render_minutes = 8, 8, 1, None
    reverse = 0

    @classmethod
    def get_params(cls, sampler=0, flags=0):
        p = capi.Params()
        p.reverse = cls.reverse
        return p


def test_driver_constructor_clashes():
    from rgk_amd import render_driver as rd
    drv = rd.RenderDriver(None, Cfg, None, device="cpu", track_demod=True)
    assert drv.track_demod and drv.albedo_floor == pytest.approx(0.02) and drv.demod_ob is not None and drv.div_ob is not None
    plain = rd.RenderDriver(None, Cfg, None, device="cpu")
    assert not plain.track_demod and plain.demod_ob is None and plain.div_ob is None
    assert bytes(plain.default_denoise_params()) == bytes(capi.DenoiseParams())  # (an empty frame: sigma_color 1)
    for kw, word in ((dict(track_noise=True), "track_noise"), (dict(track_noise=True, adaptive=capi.AdaptParams(0.1, 4)), "track_noise"),
                     (dict(history=rd.TemporalHistory()), "history"), (dict(aov_hops=2), "aov_hops"), (dict(world_size=2), "world_size")):
        with pytest.raises(ValueError, match=word):
            rd.RenderDriver(None, Cfg, None, device="cpu", track_demod=True, **kw)

    class Bidirectional(Cfg):
        reverse = 3
    with pytest.raises(ValueError, match="reverse"):
        rd.RenderDriver(None, Bidirectional, None, device="cpu", track_demod=True)
    for v in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="albedo_floor"):
            rd.RenderDriver(None, Cfg, None, device="cpu", track_demod=True, albedo_floor=v)
    for call in (plain.irradiance, plain.albedo_mean):
        with pytest.raises(ValueError, match="track_demod"):
            call()
    with pytest.raises(ValueError, match="track_demod"):
        plain.render_frame(rounds=0, output_file="o.exr", irradiance_file="i.exr")


def test_a_checkpoint_without_the_demodulated_sums_is_refused(tmp_path):
    from rgk_amd import render_driver as rd
    drv = rd.RenderDriver(None, Cfg, None, device="cpu", track_demod=True)
    path = tmp_path / "frame.ckpt"
    path.write_bytes(b"x")
    with pytest.raises(RuntimeError, match=r"frame\.ckpt\.demod"):
        drv.load_checkpoint(str(path))
    (tmp_path / "frame.ckpt.demod").write_bytes(b"x")
    with pytest.raises(RuntimeError, match=r"frame\.ckpt\.div"):
        drv.load_checkpoint(str(path))


def test_command_line_refusals(tmp_path, capsys):
    """--demod alone and with each switch it cannot be combined with: the stated ERROR line, before the configuration is looked at."""
    from rgk_amd.__main__ import main
    cfg = str(tmp_path / "absent.json")
    assert main([cfg, "--demod"]) == 1
    assert "ERROR: --demod needs --denoise or --upsample." in capsys.readouterr().out
    for extra, word in ((["--noise"], "--noise"), (["--until-noise", "0.1"], "--until-noise"), (["--until-noise", "0.1", "--adaptive"], "--until-noise"),
                        (["--temporal"], "--temporal"), (["--aov-hops", "2"], "--aov-hops"), (["-d", "1", "1"], "-d")):
        assert main([cfg, "--denoise", "--demod"] + extra) == 1, extra
        out = capsys.readouterr().out
        assert "ERROR: --demod cannot be combined with " + word + "." in out, (extra, out)
    for ok in (["--denoise"], ["-p", "--upsample"], ["-p", "--upsample", "--denoise", "--aov"]):
        assert main([cfg, "--demod", "-q"] + ok) == 1 and "Failed to load config file" in capsys.readouterr().out  # accepted: it got as far as the file
    # a bidirectional configuration: refused once the file is read, before the scene is built or a GPU asked for
    bidir = tmp_path / "bidir.json"
    bidir.write_text('{"output-file": "t.exr", "output-width": 8, "output-height": 8, "multisample": 1, "recursion-max": 2, "reverse": 2, '
                     '"camera": {"position": [0, 1, 5], "lookat": [0, 0, 0], "fov": 35}, "model-file": "absent.obj"}')
    assert main([str(bidir), "--denoise", "--demod"]) == 1
    out = capsys.readouterr().out
    assert 'ERROR: --demod cannot be combined with bidirectional rounds ("reverse" > 0' in out and "Failed to load" not in out, out


# ----------------------------------------------------------------------- the new launches' plans (rgk_plan.h)
def test_demod_launch_plans(tmp_path):
    """tests/cpp/demod_plan_main.cpp includes rgk_plan.h alone and checks, under ASan + UBSan, for every gshift 0 .. 6 and pixel counts
    around the tile sizes: k_resolve_demod's tile is at most 64 pixels (a wave: one lane per pixel), its LDS is exactly two planes of
    [PT][2^g + 1] float4 -- twice k_resolve_tiled's -- and fits a workgroup's 64 KB, its grid covers the pixels or is the bounded
    maximum; k_demod_divisor's grid is ceil(slots / 256) up to 8 workgroups per compute unit, never 0."""
    import subprocess
    exe = str(tmp_path / "demod_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "demod_plan_main.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
