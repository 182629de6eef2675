"""GPU suite (-m gpu): the last bounce of a unidirectional pass, k_last_vertex (rgk_amd/csrc/rgk_shade.h, tuning key "last_vertex").

At bounce depth - 1 every vertex of the queue is its path's last, and the fast shading launch is a kernel that neither samples
nor queues a ray and runs the vertex in two halves: the geometry of every queue entry, then the NEE of the live vertices from a
record ring in LDS.  It must give the bits of k_shade (switch 0) -- RGB sums, sample counts, path and shadow ray counts; only
the order of the shadow queue's entries may differ, and one shadow ray per slot and bounce makes the sums independent of it:

  the mixed small scene of test_gpu_const_light.py (LTC + bump, diffuse, mirror, glass: deferral, an opening to the sky) at depth
  2, 3 and 5 -- the last bounce behind 1, 2 and 4 others -- on both light routes, with and without an emitting material
  (e_front and A - B in the second half; the emitter makes the scene ineligible for the constant-light route);
  queues smaller than a workgroup and no multiple of one (8 x 8 x 1 and 20 x 13 x 3 spp): a final partial flush of the ring;
  a quad under the sky: every bounce ray misses, the ring stays empty;
  a closed box with the light inside: every vertex is live, the ring fills and wraps;
  two sample passes, two rounds of a frame; the Sponza workload's materials; and once against the oracle."""
import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder
from rgk_amd.workloads import Workload

from conftest import record_parity
from test_gpu_const_light import Frame, T, assert_same_bits, render_fresh, small_scene

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 40, 8


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def camera(w=W, h=H, pos=(0, 1.5, 5.5), lookat=(0, 1.3, 0)):
    return make_camera(pos, lookat, (0, 1, 0), fov=45, xres=w, yres=h, focus_plane=5.0, lens_size=0.0)


def params(depth, w=W, h=H, spp=SPP):
    return make_params(w, h, spp, depth, clamp=30.0, russian=0.7, bumpscale=2.0, reverse=0)


def both_switches(rd, wl, prm, tiles, rounds=1, **tuning):
    """`rounds` rounds of one frame under last_vertex = 0 and = 1 in fresh scenes, compared bit for bit; returns the switch-1 rounds."""
    off = render_fresh(rd, wl, prm, tiles, rounds=rounds, last_vertex=0, **tuning)
    on = render_fresh(rd, wl, prm, tiles, rounds=rounds, last_vertex=1, **tuning)
    for r in range(rounds):
        assert_same_bits(off[r], on[r], (tuning, "round", r))
    return on


def quad_under_the_sky():
    sb = SceneBuilder()
    m = sb.new_material("white", capi.BXDF_DIFFUSE)
    m["tex_diffuse"] = sb.create_solid_texture((0.7, 0.7, 0.7))
    sb.register_material(m)
    sb.add_primitive("plane", T((1, 1, 1), (0, 0, 0)), "white")
    sb.add_point_light((0.3, 2.6, 0.4), (1.0, 0.95, 0.8), 9.0, 0.0)
    sb.set_skybox_color((0.55, 0.7, 0.9), 0.8)
    return sb


def closed_box():
    """Six diffuse walls around the camera and the light: no ray leaves, every vertex has the light above its horizon."""
    sb = SceneBuilder()
    for name, c in (("white", (0.7, 0.7, 0.7)), ("red", (0.6, 0.1, 0.1)), ("green", (0.1, 0.6, 0.1))):
        m = sb.new_material(name, capi.BXDF_DIFFUSE)
        m["tex_diffuse"] = sb.create_solid_texture(c)
        sb.register_material(m)
    sb.add_primitive("plane", T((2, 1, 2), (0, 0, 0)), "white")
    sb.add_primitive("plane", T((2, 1, 2), (0, 3, 0), (np.pi, (1, 0, 0))), "white")
    sb.add_primitive("plane", T((2, 1, 2), (0, 1.5, -2), (np.pi / 2, (1, 0, 0))), "white")
    sb.add_primitive("plane", T((2, 1, 2), (0, 1.5, 2), (-np.pi / 2, (1, 0, 0))), "white")
    sb.add_primitive("plane", T((2, 1, 2), (-2, 1.5, 0), (-np.pi / 2, (0, 0, 1))), "red")
    sb.add_primitive("plane", T((2, 1, 2), (2, 1.5, 0), (np.pi / 2, (0, 0, 1))), "green")
    sb.add_point_light((0.2, 1.6, 0.1), (1.0, 0.95, 0.8), 9.0, 0.0)
    sb.set_skybox_color((0.55, 0.7, 0.9), 0.8)
    return sb


@pytest.mark.parametrize("emitter", [False, True])
@pytest.mark.parametrize("const_light", [1, 0])
@pytest.mark.parametrize("depth", [2, 3, 5])
def test_last_vertex_bits_small_scene(rd, depth, const_light, emitter):
    wl = Frame(small_scene(emitter=emitter), camera())
    on = both_switches(rd, wl, params(depth), rd.generate_task_list(W, H), const_light=const_light)
    assert (on[0][1] == SPP).all() and float(on[0][0].max()) > 0.0
    assert on[0][2].path_rays > 0 and on[0][2].shadow_rays > 0


@pytest.mark.parametrize("w,h,spp", [(8, 8, 1), (20, 13, 3)])
def test_last_vertex_bits_queues_below_a_workgroup(rd, w, h, spp):
    """64 and 780 paths: the last bounce's queue is shorter than a workgroup of 256, or no multiple of it."""
    wl = Frame(small_scene(), camera(w, h))
    on = both_switches(rd, wl, params(2, w, h, spp), rd.generate_task_list(w, h))
    assert on[0][2].path_rays > w * h * spp and on[0][2].shadow_rays > 0


def test_last_vertex_bits_all_sky(rd):
    """Every bounce ray leaves the quad upwards into the sky: the last launch has sky vertices only, no shadow ray leaves it."""
    wl = Frame(quad_under_the_sky(), camera(32, 24, pos=(0, 2.5, 3.0), lookat=(0, 0, 0)))
    tiles = rd.generate_task_list(32, 24)
    (_, _, first), = render_fresh(rd, wl, params(1, 32, 24, 4), tiles, last_vertex=1)
    on = both_switches(rd, wl, params(2, 32, 24, 4), tiles)
    assert on[0][2].path_rays > first.path_rays and on[0][2].shadow_rays == first.shadow_rays > 0


def test_last_vertex_bits_all_live(rd):
    """A closed box, the light inside: a vertex leaves a shadow ray -- one per path ray, but for the rays that slip through a seam
    between two walls (a sky vertex), well under one in a hundred."""
    w, h, spp = 64, 48, 4
    wl = Frame(closed_box(), camera(w, h, pos=(0, 1.5, 1.8), lookat=(0, 1.4, 0)))
    on = both_switches(rd, wl, params(2, w, h, spp), rd.generate_task_list(w, h))
    assert 0.99 * on[0][2].path_rays <= on[0][2].shadow_rays <= on[0][2].path_rays


def test_last_vertex_bits_two_sample_passes_two_rounds(rd):
    """batch_paths = 72 * 40 * 4: two sample passes of 4 spp, over two rounds of one frame; also against the one-pass frame."""
    wl = Frame(small_scene(), camera())
    tiles = rd.generate_task_list(W, H)
    one = render_fresh(rd, wl, params(3), tiles, rounds=2, last_vertex=1)
    two = both_switches(rd, wl, params(3), tiles, rounds=2, batch_paths=W * H * SPP // 2)
    for r in range(2):
        assert_same_bits(one[r], two[r], ("one pass against two", r))


def test_last_vertex_bits_sponza(rd):
    """The headline's materials and textures: Workload("sponza-1080p", scale=0.05, spp=4), depth 2."""
    wl = Workload("sponza-1080p", scale=0.05, spp=4)
    assert wl.reverse == 0 and wl.depth == 2
    on = both_switches(rd, wl, wl.params(), rd.generate_task_list(wl.xres, wl.yres))
    assert on[0][2].shadow_rays > 0


def test_last_vertex_small_scene_against_oracle(rd, oracle):
    """The first 8 tiles of the mixed scene at depth 2 against the oracle: relative L2 <= 1e-3, the parity tests' gate."""
    wl = Frame(small_scene(), camera())
    prm = params(2)
    tiles = rd.generate_task_list(W, H)
    acc, cnt, _ = render_fresh(rd, wl, prm, tiles, last_vertex=1)[0]
    n_tiles = min(8, len(tiles))
    sub = (capi.Tile * n_tiles)(*tiles[:n_tiles])
    o = oracle.OracleScene(wl.builder.to_desc())
    ao = np.zeros_like(acc); co = np.zeros_like(cnt)
    o.render_round(wl.camera, prm, sub, ao, co)
    m = co > 0
    assert m.sum() > 0 and np.array_equal(cnt[m], co[m])
    img, ref = acc[m] / cnt[m][:, None], ao[m] / co[m][:, None]
    rel = float(np.linalg.norm(img - ref) / np.linalg.norm(ref))
    record_parity("test_last_vertex_small_scene_against_oracle", rel_l2=rel, pixels=int(m.sum()), size=f"{W}x{H}x{SPP} depth 2")
    assert rel <= 1e-3, rel
