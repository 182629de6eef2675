"""CPU suite: the padding helper of tests/pad_ref.py, before the GPU tests rely on it (tests/test_gpu_thresholds.py).

1. The oracle's round does not depend on a material or texture number: orc_render_round of small_scene() (test_gpu_const_light.py)
   and of the material zoo (test_bdpt_cpu.zoo_builder) at 67 x 45 x 8 spp, depth 5, reverse 0 and 3, gives the same accumulator
   bits, sample counts and counters with P in {0, 70} filler materials and K in {0, 3} filler byte tables in front.  The oracle
   has no LDS and no threshold, so this shows -- without the code under test -- that a round is invariant under the renumbering,
   and that the helper renumbers triangles, mix children and texture ids correctly.  The oracle IS invariant on every case here,
   so the GPU tests may hold a padded scene both to its unpadded GPU run and to the oracle.
2. The helper moves what the GPU tests need moved: after 60 fillers the zoo's mix material has one child below id 64 and one at
   or above it, after 64 every triangle's material is >= 64, after K tables the descriptor holds K + 1 distinct byte tables with
   the scene's own last; no filler equals another material; fillers are on no triangle and start no light."""
import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params

import pad_ref as P_
from test_bdpt_cpu import zoo_builder, zoo_camera

W, H, SPP, DEPTH = 67, 45, 8, 5


def small_builder():
    import test_gpu_const_light as CL
    return CL.small_scene()


def small_camera(w=W, h=H):
    return make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=w, yres=h, focus_plane=5.0)


SCENES = {"small": (small_builder, small_camera), "zoo": (zoo_builder, zoo_camera)}


def round_params(reverse):
    return make_params(W, H, SPP, DEPTH, clamp=30.0, russian=0.7, bumpscale=2.0, reverse=reverse)


@pytest.fixture(scope="module")
def base_rounds(oracle):
    """Once: the oracle's round of the unpadded scenes, (scene, reverse) -> (accum, count, counters); never modified."""
    out = {}
    for name, (mk, cam) in SCENES.items():
        sb = mk()                   # (alive while the descriptor is read: it owns the geometry arrays)
        o = oracle.OracleScene(sb.to_desc())
        for reverse in (0, 3):
            a, c, k = o.render_round(cam(W, H), round_params(reverse), oracle.generate_task_list(W, H))
            a.setflags(write=False); c.setflags(write=False)
            out[(name, reverse)] = (a, c, k)
    return out


@pytest.mark.parametrize("pad", [(70, 0), (0, 3), (70, 3)], ids=lambda p: f"P{p[0]}-K{p[1]}")
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_the_oracle_round_does_not_depend_on_material_or_texture_numbers(oracle, base_rounds, scene, pad):
    mk, cam = SCENES[scene]
    sb = P_.pad(mk(), *pad)
    o = oracle.OracleScene(sb.to_desc())
    for reverse in (0, 3):
        a0, c0, k0 = base_rounds[(scene, reverse)]
        a, c, k = o.render_round(cam(W, H), round_params(reverse), oracle.generate_task_list(W, H))
        assert float(a0.max()) > 0.0 and k0.path_rays > W * H * SPP and k0.shadow_rays > 0
        assert np.array_equal(c, c0), (scene, pad, reverse)
        assert np.array_equal(a.view(np.uint32), a0.view(np.uint32)), (scene, pad, reverse, int((a != a0).any(axis=2).sum()))
        assert (k.paths, k.path_rays, k.shadow_rays) == (k0.paths, k0.path_rays, k0.shadow_rays), (scene, pad, reverse)


def _same_but_name(a, b, sb):
    """Two material dicts describe the same material (textures compared by content)."""
    def tex(i):
        if i < 0:
            return None
        t = sb.textures[i]
        return (t["kind"], t["color"], None if t["data"] is None else t["data"].tobytes())
    keys = ("kind", "flags", "emission", "roughness", "ior", "amount", "mix_m1", "mix_m2")
    return all(a[k] == b[k] for k in keys) and all(tex(a[k]) == tex(b[k]) for k in ("tex_diffuse", "tex_color", "tex_bump"))


def test_fillers_are_loud_distinct_and_unused():
    for mk in (small_builder, zoo_builder):
        plain = mk()
        sb = P_.pad_materials(mk(), 200)
        assert len(sb.materials) == len(plain.materials) + 200
        kinds = {m["kind"] for m in sb.materials[:200]}
        assert {capi.BXDF_DIFFUSE, capi.BXDF_MIRROR, capi.BXDF_DIELECTRIC, capi.BXDF_LTC_BECKMANN, capi.BXDF_LTC_GGX_DIFFUSE} <= kinds
        assert all(max(m["emission"]) >= 300.0 for m in sb.materials[:200] if m["kind"] == capi.BXDF_DIFFUSE)
        for i in range(200):
            for j in range(i + 1, len(sb.materials)):
                assert not _same_but_name(sb.materials[i], sb.materials[j], sb), (i, j)
        used = set(int(x) for a in sb.tri_mat for x in a)
        children = {m[k] for m in sb.materials for k in ("mix_m1", "mix_m2") if m["kind"] == capi.BXDF_MIX}
        assert min(used) >= 200 and (not children or min(children) >= 200)
        assert sb.areal == plain.areal and sb.pointlights == plain.pointlights
        for name, i in plain.mat_by_name.items():                     # the name map follows, and names a record with the same content
            j = sb.material_index(name)
            assert j == i + 200 and sb.materials[j]["name"] == name
        d0, d1 = plain.to_desc(), sb.to_desc()
        assert np.array_equal(np.ctypeslib.as_array(d1.tri_material, shape=(d1.n_triangles,)),
                              np.ctypeslib.as_array(d0.tri_material, shape=(d0.n_triangles,)) + 200)


def test_sixty_fillers_split_the_zoo_mix_and_sixty_four_move_every_triangle():
    sb = P_.pad_materials(zoo_builder(), 60)
    mix = sb.materials[sb.material_index("mix")]
    assert mix["kind"] == capi.BXDF_MIX and sb.material_index("mix") >= P_.LDS_MATERIALS
    kids = sorted((mix["mix_m1"], mix["mix_m2"]))
    assert kids[0] < P_.LDS_MATERIALS <= kids[1], kids
    assert {sb.materials[k]["name"] for k in kids} == {"red", "bek"}
    used = np.concatenate(sb.tri_mat)
    assert (used < P_.LDS_MATERIALS).any() and (used >= P_.LDS_MATERIALS).any()      # P = 60: triangles on both sides
    for mk in (zoo_builder, small_builder):
        sb = P_.pad_materials(mk(), 64)
        d = sb.to_desc()
        tm = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,))
        assert d.n_materials > 64 and (tm >= P_.LDS_MATERIALS).all() and (tm < d.n_materials).all()


@pytest.mark.parametrize("K", [0, 1, 2, 3])
def test_filler_tables_come_first_and_are_distinct(K):
    from rgk_amd.scene import gamma_lut
    plain = small_builder()
    sb = P_.pad_tables(small_builder(), K)
    d = sb.to_desc()
    tables = P_.desc_tables(d)
    assert len(tables) == K + 1 and len(set(tables)) == K + 1
    assert tables[-1] == gamma_lut().tobytes()                        # the scene's own byte textures: table offset 256 K
    assert [tables[k] == P_.filler_table(k).tobytes() for k in range(K)] == [True] * K
    assert 256 * K + 256 <= P_.LDS_LUT_FLOATS if K <= 1 else 256 * K + 256 > P_.LDS_LUT_FLOATS
    for k in range(K):
        assert (d.textures[k].kind, d.textures[k].width, d.textures[k].height) == (capi.TEX_RGB8, 1, 1)
    for m0, m1 in zip(plain.materials, sb.materials):                 # every texture id moved by K and names the same texture
        for key in ("tex_diffuse", "tex_color", "tex_bump"):
            assert m1[key] == (m0[key] + K if m0[key] >= 0 else -1)
            if m0[key] >= 0:
                t0, t1 = plain.textures[m0[key]], sb.textures[m1[key]]
                assert t0["kind"] == t1["kind"] and t0["color"] == t1["color"] and (t0["data"] is None or np.array_equal(t0["data"], t1["data"]))
    assert sb.tex_by_path["bump"] == plain.tex_by_path["bump"] + K


def test_the_gpu_tests_scenes_are_what_they_claim():
    """What tests/test_gpu_thresholds.py asserts about its own inputs before it touches the device, run here without one: the unit
    material set's two mixes straddle 64 in both directions under 60 fillers; its texture scenes hold K + 2 caller tables with
    the gamma table at offset 256 K; its round scenes have triangles on both sides of 64 at P = 60."""
    import test_gpu_thresholds as TH
    TH.test_sixty_fillers_put_both_mixes_across_the_threshold()
    for K in (0, 1, 2, 3):
        sb, tex, pal, _ = TH.texture_scene(K)
        tables = P_.desc_tables(sb.to_desc())
        assert len(tables) == K + 2 and tables[K] == TH.gamma_lut().tobytes() and tables[K + 1] == TH.own_table().tobytes()
        assert len(pal) == len(TH.SMALL_SIZES) and all(sb.textures[i]["kind"] == capi.TEX_RGB32F for i in pal)
        assert all(len(np.unique(sb.textures[i]["data"].view(np.uint32))) <= 256 for i in pal)
        both = [i for i in pal if (sb.textures[i]["data"].view(np.uint32) == 0x80000000).any() and (sb.textures[i]["data"].view(np.uint32) == 0).any()]
        assert len(both) == 1
    for scene in TH.ROUND_SCENES:
        for P, K in TH.PADS:
            TH.padded(scene, P, K)


def test_both_paddings_commute():
    a = P_.pad_tables(P_.pad_materials(small_builder(), 7), 2)
    b = P_.pad_materials(P_.pad_tables(small_builder(), 2), 7)
    for m0, m1 in zip(a.materials[7:], b.materials[7:]):
        assert m0 == m1
    assert all(np.array_equal(x, y) for x, y in zip(a.tri_mat, b.tri_mat))
