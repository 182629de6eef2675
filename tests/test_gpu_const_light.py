"""GPU suite (-m gpu): the constant-light route (include/rgk.h rgk_scene_info::const_light, tuning key "const_light").

A scene whose only light is one point light of size 0 reports const_light == 1, and unidirectional rounds then take the light as
launch constants instead of picking, storing and re-reading it per path, and queue 32-byte shadow records.  The route must give
the bits of the per-path route (switch 0): RGB sums, sample counts, path and shadow ray counts -- on a small scene that mixes
fast-route, generic-route and sky vertices, at depths where the light is used at the last vertex only (1), at a first and a last
vertex (2) and at non-last later vertices (5), with a lens camera, with two sample passes, over two rounds of a frame (capped
entry lists, light-side entry nodes), and on the Sponza workload's material mix.  Scenes that are not eligible report 0 and the
switch does nothing.  The small scene is compared once with the oracle, which keeps the generic pick."""
import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder, glm_mat4_mul, glm_rotate, glm_scale, glm_translate

from conftest import record_parity

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 40, 8   # 72 x 40: no multiple of the 32-pixel tile nor (per tile row) of the 8-pixel entry group


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


class Frame:
    """What render_fresh needs of a workload: a builder and a camera."""

    def __init__(self, builder, camera):
        self.builder, self.camera = builder, camera


def render_fresh(rd, wl, prm, tiles, rounds=1, expect=None, **tuning):
    """[(accum, count, counters)] of `rounds` rounds of one frame in a fresh scene with the given switches."""
    g = rd.Scene(wl.builder.to_desc())
    if expect is not None:
        assert g.info().const_light == expect, (g.info().const_light, expect)
    if tuning:
        g.set_tuning(**tuning)
    out = [g.render_round(wl.camera, prm, tiles) for _ in range(rounds)]
    g.close()
    return out


def assert_same_bits(base, got, what):
    (a0, c0, k0), (a1, c1, k1) = base, got
    assert np.array_equal(c0, c1), (what, "sample counts")
    differ = int((a0.view(np.uint32) != a1.view(np.uint32)).any(axis=2).sum())
    assert differ == 0, (what, f"{differ} pixels differ", float(np.linalg.norm(a1 - a0) / np.linalg.norm(a0)))
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), what
    assert (k0.path_rays, k0.shadow_rays) == (k1.path_rays, k1.shadow_rays), (what, "ray counts")


def T(scale, translate, rot=None):
    m = glm_scale(scale)
    if rot:
        m = glm_mat4_mul(glm_rotate(rot[0], rot[1]), m)
    return glm_mat4_mul(glm_translate(translate), m)


def small_scene(lights=((0.3, 2.6, 0.4, 0.0),), emitter=False):
    """A box open towards the camera (paths leave through the opening: sky vertices) with a textured, bump-mapped LTC floor
    and back wall, plain diffuse walls, a mirror wall and a glass cube; `lights`: (x, y, z, size) point lights."""
    rng = np.random.default_rng(7)
    sb = SceneBuilder()

    def mat(name, kind, **kw):
        m = sb.new_material(name, kind)
        for k, v in kw.items():
            m[k] = sb.create_solid_texture(v) if k.startswith("tex_") and not isinstance(v, int) else v
        return sb.register_material(m)
    albedo = sb.add_image_texture("albedo", (0.15 + 0.7 * rng.random((16, 16, 3))).astype(np.float32))
    bump = sb.add_image_texture8("bump", rng.integers(0, 256, (16, 16, 3), dtype=np.uint8))
    mat("tiles", capi.BXDF_LTC_GGX_DIFFUSE, tex_diffuse=albedo, tex_color=(0.3, 0.3, 0.25), tex_bump=bump, roughness=0.25)
    mat("bek", capi.BXDF_LTC_BECKMANN, tex_color=(0.8, 0.6, 0.2), tex_bump=bump, roughness=0.3)
    mat("white", capi.BXDF_DIFFUSE, tex_diffuse=(0.7, 0.7, 0.7))
    mat("red", capi.BXDF_DIFFUSE, tex_diffuse=(0.6, 0.1, 0.1))
    mat("mirror", capi.BXDF_MIRROR, tex_color=(0.9, 0.9, 0.9))
    mat("glass", capi.BXDF_DIELECTRIC, tex_color=(1.0, 1.0, 1.0), ior=1.5, flags=capi.MAT_NO_RUSSIAN)
    if emitter:
        mat("lamp", capi.BXDF_DIFFUSE, tex_diffuse=(0.5, 0.5, 0.5), emission=(6.0, 6.0, 5.0))
    sb.add_primitive("plane", T((2, 1, 2), (0, 0, 0)), "tiles", texscale=(3.0, 3.0, 1.0))
    sb.add_primitive("plane", T((2, 1, 2), (0, 3, 0), (np.pi, (1, 0, 0))), "white")
    sb.add_primitive("plane", T((2, 1, 2), (0, 1.5, -2), (np.pi / 2, (1, 0, 0))), "tiles", texscale=(2.0, 2.0, 1.0))
    sb.add_primitive("plane", T((2, 1, 2), (-2, 1.5, 0), (-np.pi / 2, (0, 0, 1))), "red")
    sb.add_primitive("plane", T((2, 1, 2), (2, 1.5, 0), (np.pi / 2, (0, 0, 1))), "mirror")
    sb.add_primitive("cube", T((0.8, 0.8, 0.8), (-0.9, 0.4, -0.5), (0.4, (0, 1, 0))), "glass")
    sb.add_primitive("cube", T((0.5, 0.5, 0.5), (0.6, 0.25, 0.6)), "bek")
    if emitter:
        sb.add_primitive("tri", T((0.4, 1, 0.4), (0.0, 2.9, -0.5), (np.pi, (1, 0, 0))), "lamp")
    for x, y, z, size in lights:
        sb.add_point_light((x, y, z), (1.0, 0.95, 0.8), 9.0, size)
    sb.set_skybox_color((0.55, 0.7, 0.9), 0.8)
    return sb


def camera(lens=0.0):
    return make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=W, yres=H, focus_plane=5.0, lens_size=lens)


def params(depth, reverse=0):
    return make_params(W, H, SPP, depth, clamp=30.0, russian=0.7, bumpscale=2.0, reverse=reverse)


def both_switches(rd, wl, prm, tiles, expect, rounds=2, **tuning):
    """Two rounds of one frame under const_light = 0 and = 1 in fresh scenes, compared bit for bit; returns the switch-1 rounds."""
    off = render_fresh(rd, wl, prm, tiles, rounds=rounds, expect=expect, const_light=0, **tuning)
    on = render_fresh(rd, wl, prm, tiles, rounds=rounds, expect=expect, const_light=1, **tuning)
    for r in range(rounds):
        assert_same_bits(off[r], on[r], (tuning, "round", r))
        assert on[r][2].path_rays > 0 and on[r][2].shadow_rays > 0
    return on


@pytest.mark.parametrize("depth", [1, 2, 5])
def test_const_light_bits_small_scene(rd, depth):
    wl = Frame(small_scene(), camera())
    tiles = rd.generate_task_list(W, H)
    on = both_switches(rd, wl, params(depth), tiles, expect=1)
    assert (on[0][1] == SPP).all() and float(on[0][0].max()) > 0.0


def test_const_light_bits_lens_camera(rd):
    wl = Frame(small_scene(), camera(lens=0.08))
    both_switches(rd, wl, params(5), rd.generate_task_list(W, H), expect=1)


def test_const_light_bits_two_sample_passes(rd):
    """batch_paths = 72 * 40 * 4: the whole pixel list x 2 sample passes of 4 spp; also against the one-pass frame."""
    wl = Frame(small_scene(), camera())
    tiles = rd.generate_task_list(W, H)
    one = render_fresh(rd, wl, params(5), tiles, rounds=2, expect=1, const_light=1)
    two = both_switches(rd, wl, params(5), tiles, expect=1, batch_paths=W * H * SPP // 2)
    for r in range(2):
        assert_same_bits(one[r], two[r], ("one pass against two", r))


def test_const_light_bits_sponza(rd, sponza_small):
    """The real material mix: Workload("sponza-1080p", scale=0.1, spp=8)."""
    wl = sponza_small
    assert wl.reverse == 0
    both_switches(rd, wl, wl.params(), rd.generate_task_list(wl.xres, wl.yres), expect=1)


def test_const_light_small_scene_against_oracle(rd, oracle):
    """The first 8 tiles at depth 2 against the oracle (which keeps the generic pick): relative L2 <= 1e-3, the Sponza tests' gate.
    The measured value goes into the run's parity table through record_parity."""
    wl = Frame(small_scene(), camera())
    prm = params(2)
    tiles = rd.generate_task_list(W, H)
    acc, cnt, _ = render_fresh(rd, wl, prm, tiles, expect=1, const_light=1)[0]
    n_tiles = min(8, len(tiles))
    sub = (capi.Tile * n_tiles)(*tiles[:n_tiles])
    o = oracle.OracleScene(wl.builder.to_desc())
    ao = np.zeros_like(acc); co = np.zeros_like(cnt)
    o.render_round(wl.camera, prm, sub, ao, co)
    m = co > 0
    assert m.sum() > 0 and np.array_equal(cnt[m], co[m])
    img, ref = acc[m] / cnt[m][:, None], ao[m] / co[m][:, None]
    rel = float(np.linalg.norm(img - ref) / np.linalg.norm(ref))
    record_parity("test_const_light_small_scene_against_oracle", rel_l2=rel, pixels=int(m.sum()), size=f"{W}x{H}x{SPP} depth 2")
    assert rel <= 1e-3, rel


@pytest.mark.parametrize("case", ["sized", "two-lights", "light-and-emitter", "negative-zero"])
def test_not_eligible_scenes_report_zero_and_ignore_the_switch(rd, case):
    sb = {"sized": lambda: small_scene(lights=((0.3, 2.6, 0.4, 0.5),)),
          "two-lights": lambda: small_scene(lights=((0.3, 2.6, 0.4, 0.0), (-1.0, 2.0, 1.0, 0.0))),
          "light-and-emitter": lambda: small_scene(emitter=True),
          "negative-zero": lambda: small_scene(lights=((-0.0, 2.6, 0.4, 0.0),))}[case]()
    if case == "light-and-emitter":
        assert len(sb.areal) == 1
    if case == "negative-zero":
        assert np.signbit(np.float32(sb.pointlights[0]["pos"][0]))
    wl = Frame(sb, camera())
    both_switches(rd, wl, params(3), rd.generate_task_list(W, H), expect=0, rounds=1)


def test_bidirectional_round_on_an_eligible_scene(rd, oracle):
    """reverse = 2 stays on the per-path route (the connection kernels read the per-slot light): the round succeeds under both
    switch values and traces the same rays.  Its splats are float atomics, so the image is held per pixel to the oracle's terms
    (tests/bdpt_ref.py): the two switch values give the same bits wherever at most one splat lands, and no pixel falls outside
    the summation-order bound.  The reference is the oracle's round with every ray answered by exhaustive search, the rule the
    GPU's traversal is pinned to: on this scene's bump-mapped floor and wall a connection between two points of one surface
    carries radiance (the shading normal leaves the plane) along a ray that lies IN the surface, and the kd-tree oracle decides
    such rays inside its epsilon band -- against it 39 of the 2880 pixels differ (recorded), without bump maps none."""
    import bdpt_ref as B
    wl = Frame(small_scene(), camera())
    tiles = rd.generate_task_list(W, H)
    prm = params(4, reverse=2)
    (a0, c0, k0), = render_fresh(rd, wl, prm, tiles, expect=1, const_light=0)
    (a1, c1, k1), = render_fresh(rd, wl, prm, tiles, expect=1, const_light=1)
    assert np.array_equal(c0, c1)
    assert (k0.path_rays, k0.shadow_rays) == (k1.path_rays, k1.shadow_rays) and k1.path_rays > 0
    o = oracle.OracleScene(wl.builder.to_desc())
    split = o.render_round_split(wl.camera, prm, oracle.generate_task_list(W, H), exhaustive=True)
    kd = o.render_round_split(wl.camera, prm, oracle.generate_task_list(W, H))
    ao = o.render_round(wl.camera, prm, oracle.generate_task_list(W, H))[0]
    few = split.splat_n <= 1
    assert split.n_splats > 0 and few.any() and np.array_equal(a0[few].view(np.uint32), a1[few].view(np.uint32))
    for switch, a, c in ((0, a0, c0), (1, a1, c1)):
        planes, s = B.check_split(a, c, split)
        record_parity(f"test_bidirectional_round_on_an_eligible_scene:const-light-{switch}", rel_l2=float(np.linalg.norm(a - ao) / np.linalg.norm(ao)),
                      outside_vs_kd_oracle=B.check_split(a, c, kd)[1]["outside"], **B.record_fields(s))
        assert s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["exact_n0"] == s["exact_n1"] == 1.0, (switch, s)
    assert k1.path_rays == split.counters.path_rays == kd.counters.path_rays and k1.shadow_rays <= split.counters.shadow_rays
