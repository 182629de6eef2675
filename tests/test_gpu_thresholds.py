"""GPU suite (-m gpu): the shading data paths of scenes with more than 64 materials and more than two byte tables.

rgk_amd/csrc/rgk_device.h picks a load path by scene size: mat_load() reads material ids below RGK_LDS_MATERIALS (64) from the
copy lut_lds_fill() puts in LDS and the others with a record load from global memory; texel_at() / texels_at<N>() decode a byte
texel through LDS while the texture's table ends inside the first RGK_LDS_LUT_FLOATS (512) floats of the table pool and with
three global loads (differently written shifts) beyond.  Every other test scene stays below both numbers.  tests/pad_ref.py
moves a scene's records past them -- P loud filler materials and K filler byte tables in front -- and nothing that is computed
depends on a material's or texture's number (shown on the oracle, which has no thresholds, by tests/test_pad_cpu.py), so:

  unit level   rgk_bxdf_value / rgk_bxdf_sample (both routes) under P in {0, 60, 64, 200}: the bits of P = 0; P = 60 also against
               the oracle with the bounds of test_gpu_parity.test_bxdf_value_and_sample_unit_level.  rgk_texture_sample under
               K in {0, 1, 2, 3} (the scene's table at offset 0, 256: LDS; 512, 768: global): the oracle's bits, on the textures
               of test_texture_lookup_unit_level and on a family of the smallest tiled shapes in three storage forms.
  rounds       unidirectional: accumulator bits, sample counts and counters of the unpadded run under (P, K) in {(64, 0), (0, 3),
               (60, 3)}, last_vertex 0 / 1, const_light 0 / 1; (60, 3) also against the oracle's exhaustive round.  Bidirectional
               (reverse 3): every (P, K) against the oracle's exhaustive split of the padded scene (tests/bdpt_ref.py).
  planes       rgk_render_aov and rgk_render_aov_chain: the unpadded planes, bit for bit.

Every comparison is bit-exact or bdpt_ref.check_split's derived summation-order bound; no tolerance is introduced here.

Temporal reuse is left out on purpose: k_tp_reproject (rgk_post.hip) reads a material's kind with one plain global load of the
record's first word, gld_u32(sc.materials, mat * sizeof(DevMaterial)) -- neither mat_load nor a table in LDS -- so it has one
path at every scene size and belongs to neither threshold; k_tp_blend reads no material."""
import ctypes as C
import functools

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder, gamma_lut

import bdpt_ref as B
import chain_ref as CR
import pad_ref as PAD
from conftest import record_parity
from test_bdpt_cpu import zoo_builder, zoo_camera
from test_gpu_const_light import small_scene
from test_gpu_parity import _unit_dirs, material_zoo

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 67, 45, 8, 5      # the sizes of the exact round tests (test_gpu_exhaustive.py): ragged in x and y
PADS = [(64, 0), (0, 3), (60, 3)]


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN at the same position."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


# ======================================================================= unit level: BxDFs
def unit_materials():
    """The materials of test_gpu_parity.test_bxdf_value_and_sample_unit_level -- the zoo, the five LTC roughnesses, the two black
    lobes -- and IN FRONT of them a second mix, `mixfwd`, whose children come after it.  With 60 fillers in front the zoo's mix
    (a parent at or above 64 with the child `red` below) and mixfwd (a parent below 64, both children at or above) straddle the
    threshold in both directions."""
    sb = material_zoo()
    for k, r in enumerate((0.02, 0.0995, 0.3, 0.6, 1.0)):
        m = sb.new_material(f"ltc{k}", capi.BXDF_LTC_GGX_DIFFUSE if k % 2 else capi.BXDF_LTC_BECKMANN_DIFFUSE)
        m["tex_diffuse"] = sb.create_solid_texture((0.6, 0.5, 0.4)); m["tex_color"] = sb.create_solid_texture((0.3, 0.3, 0.25)); m["roughness"] = r
        sb.register_material(m)
    for k, kind in enumerate((capi.BXDF_LTC_GGX_DIFFUSE, capi.BXDF_LTC_BECKMANN)):
        m = sb.new_material(f"black{k}", kind)
        m["tex_diffuse"] = sb.create_solid_texture((0.6, 0.5, 0.4)); m["tex_color"] = sb.create_solid_texture((0.0, 0.0, 0.0)); m["roughness"] = 0.3
        sb.register_material(m)
    fwd = sb.new_material("mixfwd", capi.BXDF_MIX)
    fwd["mix_m1"], fwd["mix_m2"], fwd["amount"] = sb.material_index("ggxd"), sb.material_index("mirror"), 0.3
    for m in sb.materials:                       # one place in front: every id moves up by one (pad_materials' renumbering)
        for k in ("mix_m1", "mix_m2"):
            if m[k] >= 0:
                m[k] += 1
    fwd["mix_m1"] += 1; fwd["mix_m2"] += 1
    sb.materials.insert(0, fwd)
    sb.mat_by_name = {m["name"]: i for i, m in enumerate(sb.materials)}
    sb.tri_mat = [(a + np.uint32(1)).astype(np.uint32) for a in sb.tri_mat]
    return sb


class UnitInputs:
    """The inputs of test_bxdf_value_and_sample_unit_level (its seed, its n = 4000), made once."""

    def __init__(self):
        rng = np.random.default_rng(21)
        self.n_mat, self.n = len(unit_materials().materials), 4000
        self.mat = (np.arange(self.n) % self.n_mat).astype(np.uint32)
        self.Vi, self.Vr = _unit_dirs(rng, self.n), _unit_dirs(rng, self.n)
        self.Vr[::3] = self.Vi[::3] * np.array([-1, -1, 1], np.float32)
        self.uv = rng.uniform(-1, 2, (self.n, 2)).astype(np.float32)
        self.u = rng.uniform(0, 1, (self.n, 2)).astype(np.float32)


def bxdf_outputs(rd, lib, inp, P):
    """{route: (value, direction, weight, may_leak)} of the unit materials behind P fillers, ids renumbered."""
    sb = PAD.pad_materials(unit_materials(), P)
    assert len(sb.materials) == inp.n_mat + P
    g = rd.Scene(sb.to_desc())
    mat = (inp.mat + np.uint32(P)).astype(np.uint32)
    out = {}
    for route in (0, 1):
        val = np.zeros((inp.n, 3), np.float32); d = np.zeros((inp.n, 3), np.float32); w = np.zeros((inp.n, 3), np.float32); leak = np.zeros(inp.n, np.uint8)
        assert lib.rgk_bxdf_value(g.h, inp.n, route, mat.ctypes.data, inp.Vi.ctypes.data, inp.Vr.ctypes.data, inp.uv.ctypes.data, val.ctypes.data) == 0
        assert lib.rgk_bxdf_sample(g.h, inp.n, route, mat.ctypes.data, inp.Vi.ctypes.data, inp.uv.ctypes.data, inp.u.ctypes.data, d.ctypes.data, w.ctypes.data, leak.ctypes.data) == 0
        out[route] = (val, d, w, leak)
    g.close()
    return out, sb


@pytest.fixture(scope="module")
def unit(rd, product_lib):
    inp = UnitInputs()
    base, _ = bxdf_outputs(rd, product_lib, inp, 0)
    for route in base:
        for a in base[route]:
            a.setflags(write=False)
    return inp, base


def test_sixty_fillers_put_both_mixes_across_the_threshold():
    sb = PAD.pad_materials(unit_materials(), 60)
    T = PAD.LDS_MATERIALS
    mix, fwd = sb.material_index("mix"), sb.material_index("mixfwd")
    kids = lambda i: (sb.materials[i]["mix_m1"], sb.materials[i]["mix_m2"])
    assert sb.materials[mix]["kind"] == sb.materials[fwd]["kind"] == capi.BXDF_MIX
    assert mix >= T and min(kids(mix)) < T <= max(kids(mix)), (mix, kids(mix))          # parent global, one child below 64
    assert fwd < T and min(kids(fwd)) >= T, (fwd, kids(fwd))                           # parent in LDS, children at or above 64
    assert {sb.materials[k]["name"] for k in kids(mix)} == {"red", "bek"} and {sb.materials[k]["name"] for k in kids(fwd)} == {"ggxd", "mirror"}


@pytest.mark.parametrize("P", [60, 64, 200])
def test_bxdf_bits_do_not_depend_on_where_the_record_is_read(rd, oracle, product_lib, unit, P):
    """values, sampled directions, weights and may_leak of both routes under P fillers: the bits of P = 0, NaN positions equal.
    P = 60 splits the set (ids 60 .. 76) and both mixes; 64 and 200 put every record on the global side.  P = 60 is also held to
    the oracle on the padded descriptor with the existing unit test's bounds (libm only: 2e-4 relative on values, 2e-5 on
    directions, weights equal or within 1e-7, may_leak equal): the padded record is the same record on the CPU side too."""
    inp, base = unit
    got, sb = bxdf_outputs(rd, product_lib, inp, P)
    if P == 60:
        ids = inp.mat + 60
        assert (ids < PAD.LDS_MATERIALS).any() and (ids >= PAD.LDS_MATERIALS).any()
    else:
        assert int(inp.mat.min()) + P >= PAD.LDS_MATERIALS
    for route in (0, 1):
        shares, wrong = {}, np.zeros(inp.n, bool)
        for name, a, b in zip(("value", "dir", "weight"), got[route][:3], base[route][:3]):
            same = same_bits(a, b).all(axis=1)
            shares[name] = float(same.mean())
            wrong |= ~same
        shares["leak"] = float((got[route][3] == base[route][3]).mean())
        wrong |= got[route][3] != base[route][3]
        record_parity(f"gpu_thresholds.bxdf[P {P} K 0 route {route}]", n=inp.n, **{k + "_bit_identical": v for k, v in shares.items()},
                      bit_identical=1.0 - float(wrong.mean()), outside=int(wrong.sum()), nonzero_values=float((base[route][0].max(axis=1) > 0).mean()))
        for name, a, b in zip(("value", "dir", "weight"), got[route][:3], base[route][:3]):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (P, route, name)
            bad = ~same_bits(a, b).all(axis=1)
            assert not bad.any(), (P, route, name, int(bad.sum()), np.unique(inp.mat[bad] + P).tolist())
        assert np.array_equal(got[route][3], base[route][3]), (P, route)
    assert (base[0][0].max(axis=1) > 0).mean() > 0.3 and base[0][3].any()
    if P != 60:
        return
    desc = sb.to_desc()
    o = oracle.OracleScene(desc)
    L = oracle.lib()
    n, mat = inp.n, (inp.mat + np.uint32(P)).astype(np.uint32)
    ref_v = np.zeros((n, 3), np.float32); ref_d = np.zeros((n, 3), np.float32); ref_w = np.zeros((n, 3), np.float32); ref_l = np.zeros(n, np.int32)
    for i in range(n):
        L.orc_bxdf_value(o.h, int(mat[i]), inp.Vi[i].ctypes.data, inp.Vr[i].ctypes.data, inp.uv[i].ctypes.data, ref_v[i].ctypes.data)
        ml = C.c_int(0)
        L.orc_bxdf_sample(o.h, int(mat[i]), inp.Vi[i].ctypes.data, inp.uv[i].ctypes.data, inp.u[i].ctypes.data, ref_d[i].ctypes.data, ref_w[i].ctypes.data, C.byref(ml))
        ref_l[i] = ml.value
    for route in (0, 1):
        val, d, w, leak = got[route]
        assert np.array_equal(np.isnan(val), np.isnan(ref_v))
        both_nan = np.isnan(val) & np.isnan(ref_v)
        rel_v = float((np.abs(val - ref_v)[~both_nan] / np.maximum(np.abs(ref_v), 1e-6)[~both_nan]).max())
        ok = ~np.isnan(ref_d).any(axis=1) & (ref_w.max(axis=1) > 0)
        err_d = float(np.abs(d[ok] - ref_d[ok]).max())
        record_parity(f"gpu_thresholds.bxdf-vs-oracle[P 60 K 0 route {route}]", n=n, value_max_rel=rel_v, sample_dir_max_abs=err_d,
                      value_bit_identical=float((bits(val) == bits(ref_v)).all(axis=1).mean()))
        assert rel_v <= 2e-4 and err_d <= 2e-5, (route, rel_v, err_d)
        assert np.array_equal(bits(w), bits(ref_w)) or np.abs(w - ref_w).max() <= 1e-7
        assert np.array_equal(leak.astype(np.int32), ref_l)


# ======================================================================= unit level: textures
SMALL_SIZES = [(1, 1), (1, 5), (9, 1), (4, 8), (5, 9), (4, 16), (3, 7)]    # (height, width): below a tile, exactly one, one texel over, two tiles
N_UV = 400


def own_table():
    """A byte table that is not the gamma table: byte -> (byte / 255)^2 * 3 - 1 (negative entries included)."""
    x = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    return (x * x * np.float32(3.0) - np.float32(1.0)).astype(np.float32)


def texture_scene(K, keep_float=False):
    """(builder, [(name, texture id, height, width)], palettized ids, kamen included): the textures of
    test_texture_lookup_unit_level and the small family, behind K filler tables."""
    from rgk_amd.proxy import shipped_sponza_textures
    sb = SceneBuilder()
    rng = np.random.default_rng(22)
    tex = [("solid", sb.create_solid_texture((0.2, 0.5, 0.9)), 1, 1), ("none", -1, 1, 1),
           ("f32", sb.add_image_texture("f32", rng.random((37, 53, 3)).astype(np.float32) * 3.0), 37, 53),
           ("u8", sb.add_image_texture8("u8", rng.integers(0, 256, (29, 64, 3), dtype=np.uint8)), 29, 64)]
    jpg = shipped_sponza_textures().get("KAMEN.JPG")
    if jpg is not None:
        tex.append(("kamen", sb.add_image_texture8("kamen", np.ascontiguousarray(jpg[::-1])), jpg.shape[0], jpg.shape[1]))
    rng = np.random.default_rng(2200)
    gam = gamma_lut()
    pool = np.concatenate([(rng.random(40) * 4 - 1).astype(np.float32), gam[[3, 77, 200]]]).astype(np.float32)
    pal = []
    for j, (h, w) in enumerate(SMALL_SIZES):
        tex.append((f"{h}x{w}-gamma", sb.add_image_texture8(f"g{j}", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), h, w))
        tex.append((f"{h}x{w}-own", sb.add_image_texture8(f"o{j}", rng.integers(0, 256, (h, w, 3), dtype=np.uint8), lut=own_table()), h, w))
        # few-valued floats: even j from values of the gamma table alone (the texture then shares THAT table, at offset 256 K),
        # odd j from a pool no caller's table holds (a table of the scene's own, behind every caller's table)
        vals = gam[rng.integers(0, 256, 50)] if j % 2 == 0 else pool
        data = rng.choice(vals, size=(h, w, 3)).astype(np.float32)
        if (h, w) == (5, 9):
            data[0, 0, 0], data[0, 1, 0], data[4, 8, 2], data[2, 3, 1] = 0.0, -0.0, -0.0, 0.0     # both zeros, told apart by their bits
            assert np.signbit(data[0, 1, 0]) and not np.signbit(data[0, 0, 0])
        i = sb.add_image_texture(f"p{j}", data)
        tex.append((f"{h}x{w}-palettized", i, h, w))
        pal.append(i)
    m = sb.new_material("m", capi.BXDF_DIFFUSE); m["tex_diffuse"] = tex[0][1]; sb.register_material(m)
    sb.add_primitive("cube", np.eye(4, dtype=np.float32), "m")
    PAD.pad_tables(sb, K)
    if keep_float:
        sb.build_flags = capi.BUILD_KEEP_FLOAT_TEXTURES
    shift = lambda i: i + K if i >= 0 else i
    return sb, [(n, shift(i), h, w) for n, i, h, w in tex], [shift(i) for i in pal], jpg is not None


def texture_uvs(rng, h, w):
    """400 uv: the seam values 0, 1, -1 in both coordinates, every texel centre and corner (a random choice of them when the image
    has too many), the rest uniform in [-2, 3)^2."""
    f = np.float32
    seams = [(a, b) for a in (0.0, 1.0, -1.0) for b in (0.0, 1.0, -1.0)]
    centres = [(f(x + 0.5) / f(w), f(y + 0.5) / f(h)) for y in range(h) for x in range(w)]
    corners = [(f(x) / f(w), f(y) / f(h)) for y in range(h + 1) for x in range(w + 1)]
    for lst in (centres, corners):
        if len(lst) > 120:
            keep = rng.choice(len(lst), 120, replace=False)
            lst[:] = [lst[k] for k in keep]
    fixed = np.array(seams + centres + corners, np.float32)
    assert len(fixed) < N_UV
    return np.concatenate([fixed, rng.uniform(-2, 3, (N_UV - len(fixed), 2)).astype(np.float32)]).astype(np.float32)


def sample_gpu(lib, g, ids, uv):
    n = len(uv)
    rgb = np.zeros((n, 3), np.float32); sr = np.zeros(n, np.float32); sbm = np.zeros(n, np.float32)
    tex = np.ascontiguousarray(ids, dtype=np.int32)
    assert lib.rgk_texture_sample(g.h, n, tex.ctypes.data, uv.ctypes.data, rgb.ctypes.data, sr.ctypes.data, sbm.ctypes.data) == 0
    return rgb, sr, sbm


@pytest.mark.parametrize("K", [0, 1, 2, 3])
def test_texture_bits_do_not_depend_on_where_the_table_is_read(rd, oracle, product_lib, K):
    """rgb, slope_right and slope_bottom of rgk_texture_sample equal orc_texture_sample bit for bit with the scene's gamma table at
    offset 256 K (K <= 1: decoded through LDS, K >= 2: by global loads; the boundary is offset + 256 <= 512), the family's own
    table one further and the scene's palette behind both.  The few-valued float textures also equal the same scene built with
    RGK_BUILD_KEEP_FLOAT_TEXTURES (float4 storage), and rgk_scene_get_info confirms that all seven of them -- and only they --
    took the byte path.  Whether the KAMEN image was shipped (and sampled) is recorded."""
    sb, tex, pal, kamen = texture_scene(K)
    desc = sb.to_desc()
    assert len(PAD.desc_tables(desc)) == K + 2 and PAD.desc_tables(desc)[K] == gamma_lut().tobytes()   # K fillers, gamma at 256 K, the own table
    assert (256 * K + 256 <= PAD.LDS_LUT_FLOATS) == (K <= 1)
    g, o = rd.Scene(desc), oracle.OracleScene(desc)
    sbf, _, _, _ = texture_scene(K, keep_float=True)
    gf = rd.Scene(sbf.to_desc())
    n_float = len(SMALL_SIZES) + 1
    ig, igf = g.info(), gf.info()
    assert (ig.n_float_textures, ig.n_palettized_textures) == (n_float, len(SMALL_SIZES)), (ig.n_float_textures, ig.n_palettized_textures)
    assert (igf.n_float_textures, igf.n_palettized_textures) == (n_float, 0)
    L = oracle.lib()
    rng = np.random.default_rng(2300 + K)
    ids = np.concatenate([np.full(N_UV, i, np.int32) for _, i, _, _ in tex])
    uv = np.concatenate([texture_uvs(rng, h, w) for _, _, h, w in tex])
    n = len(uv)
    rgb, sr, sbm = sample_gpu(product_lib, g, ids, uv)
    frgb, fsr, fsbm = sample_gpu(product_lib, gf, ids, uv)
    ref = np.zeros((n, 3), np.float32); rr = np.zeros(n, np.float32); rb = np.zeros(n, np.float32)
    for i in range(n):
        a, b = C.c_float(0), C.c_float(0)
        L.orc_texture_sample(o.h, int(ids[i]), uv[i].ctypes.data, ref[i].ctypes.data, C.byref(a), C.byref(b))
        rr[i], rb[i] = a.value, b.value
    ok_rgb = (bits(rgb) == bits(ref)).all(axis=1)
    ok_slopes = (bits(sr) == bits(rr)) & (bits(sbm) == bits(rb))
    is_pal = np.isin(ids, pal)
    ok_float = (bits(rgb) == bits(frgb)).all(axis=1) & (bits(sr) == bits(fsr)) & (bits(sbm) == bits(fsbm))
    record_parity(f"gpu_thresholds.texture[P 0 K {K}]", textures=len(tex), n=n, kamen_included=int(kamen), rgb_bit_identical=float(ok_rgb.mean()),
                  slopes_bit_identical=float(ok_slopes.mean()), palettized_vs_float4_bit_identical=float(ok_float[is_pal].mean()),
                  outside=int((~(ok_rgb & ok_slopes)).sum()))
    wrong = sorted({name for (name, i, _, _) in tex if (~(ok_rgb & ok_slopes))[ids == i].any()})
    assert not wrong, (K, wrong, int((~ok_rgb).sum()), int((~ok_slopes).sum()))
    assert ok_float[is_pal].all() and ok_float.all(), (K, int((~ok_float).sum()))
    assert np.abs(ref[ids == tex[3][1]]).max() > 0 and np.abs(rr).max() > 0 and np.abs(rb).max() > 0
    for x in (g, gf):
        x.close()


# ======================================================================= whole kernels: rounds
def small_camera():
    return make_camera((0, 1.5, 5.5), (0, 1.3, 0), (0, 1, 0), fov=45, xres=W, yres=H, focus_plane=5.0)


def small_scene_byte_albedo():
    """small_scene() with its float albedo image (768 values: float4 storage) quantised to bytes under the gamma table, so that the
    colour fetch of the shading kernels (tex_get -> texels_at<4>) decodes bytes too; in small_scene() itself only the bump map's
    slopes (texels_at<3>) do."""
    sb = small_scene()
    t = sb.textures[sb.tex_by_path["albedo"]]
    assert t["kind"] == capi.TEX_RGB32F
    t["data"] = np.ascontiguousarray(np.clip(np.round(t["data"] * 255.0), 0, 255).astype(np.uint8))
    t["kind"], t["lut"] = capi.TEX_RGB8, gamma_lut()
    return sb


ROUND_SCENES = {"small": (small_scene, small_camera), "small-byte-albedo": (small_scene_byte_albedo, small_camera),
                "zoo": (zoo_builder, lambda: zoo_camera(W, H))}


def round_params(reverse=0):
    return make_params(W, H, SPP, DEPTH, clamp=30.0, russian=0.7, bumpscale=2.0, reverse=reverse)


def padded(scene, P, K):
    mk, cam = ROUND_SCENES[scene]
    sb = PAD.pad(mk(), P, K)
    if P:
        tm = np.concatenate(sb.tri_mat)
        assert (tm >= PAD.LDS_MATERIALS).all() if P >= 64 else ((tm < PAD.LDS_MATERIALS).any() and (tm >= PAD.LDS_MATERIALS).any())
    return sb, cam()


def switch_sets(eligible):
    """(last_vertex, const_light) pairs: both light routes where the scene is eligible for the constant-light route."""
    return [(lv, cl) for lv in (0, 1) for cl in ((0, 1) if eligible else (1,))]


@functools.lru_cache(maxsize=None)
def uni_rounds(rd, scene, P, K):
    """{(last_vertex, const_light): [two rounds of one frame]}, info().const_light -- each switch set in a fresh device scene."""
    sb, cam = padded(scene, P, K)
    prm, tiles = round_params(0), rd.generate_task_list(W, H)
    out, eligible = {}, None
    for lv, cl in switch_sets(True):
        g = rd.Scene(sb.to_desc())
        eligible = g.info().const_light
        if cl == 0 and not eligible:
            g.close()
            continue
        g.set_tuning(last_vertex=lv, const_light=cl)
        out[(lv, cl)] = [g.render_round(cam, prm, tiles) for _ in range(2)]
        g.close()
    return out, eligible


@pytest.mark.parametrize("pad", PADS, ids=lambda p: f"P{p[0]}-K{p[1]}")
@pytest.mark.parametrize("scene", sorted(ROUND_SCENES))
def test_unidirectional_rounds_equal_the_unpadded_run(rd, oracle, scene, pad):
    """Two rounds of one frame at 67 x 45 x 8 spp, depth 5, under last_vertex 0 / 1 and (where the scene is eligible) const_light
    0 / 1: accumulator bits, sample counts, paths, path_rays and shadow_rays of the (0, 0) run.  The fillers are on no triangle,
    so info().const_light is the unpadded scene's.  (60, 3) is also held to the oracle's round of the PADDED scene with every ray
    answered by exhaustive search: no pixel outside, every pixel exact (a unidirectional round has no splats: one possible sum),
    paths and path_rays the oracle's; shadow_rays at most the oracle's, the bar of the existing tests (zero-radiance shadow rays
    are skipped on the device) -- their exact number is pinned by the comparison with the unpadded run."""
    base, eligible = uni_rounds(rd, scene, 0, 0)
    got, eligible_padded = uni_rounds(rd, scene, *pad)
    assert eligible_padded == eligible == (0 if scene == "zoo" else 1)
    assert sorted(got) == sorted(base) == sorted(switch_sets(eligible))
    for key in sorted(base):
        for r in range(2):
            (a0, c0, k0), (a1, c1, k1) = base[key][r], got[key][r]
            differ = int((bits(a0) != bits(a1)).any(axis=2).sum())
            record_parity(f"gpu_thresholds.round[{scene} P {pad[0]} K {pad[1]} last_vertex {key[0]} const_light {key[1]} round {r}]",
                          bit_identical=1.0 - differ / (W * H), outside=differ)
            assert float(a0.max()) > 0.0 and k0.path_rays > W * H * SPP and k0.shadow_rays > 1000
            assert np.array_equal(c0, c1) and (c1 == SPP).all(), (scene, pad, key, r)
            assert differ == 0, (scene, pad, key, r, differ)
            assert (k0.paths, k0.path_rays, k0.shadow_rays) == (k1.paths, k1.path_rays, k1.shadow_rays), (scene, pad, key, r)
    if pad != (60, 3):
        return
    sb, cam = padded(scene, *pad)
    split = oracle.OracleScene(sb.to_desc()).render_round_split(cam, round_params(0), oracle.generate_task_list(W, H), exhaustive=True)
    assert split.n_splats == 0
    for key in sorted(got):
        a, c, k = got[key][0]
        planes, s = B.check_split(a, c, split)
        record_parity(f"gpu_thresholds.round-vs-oracle[{scene} P 60 K 3 last_vertex {key[0]} const_light {key[1]}]", **B.record_fields(s),
                      bit_identical=s["exact_n0"], shadow_rays_gpu_over_oracle=k.shadow_rays / max(1, split.counters.shadow_rays))
        assert s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["share_n0"] == 1.0 and s["exact_n0"] == 1.0, (scene, key, s)
        assert (k.paths, k.path_rays) == (split.counters.paths, split.counters.path_rays) and k.shadow_rays <= split.counters.shadow_rays, (scene, key)


@pytest.mark.parametrize("pad", [(0, 0)] + PADS, ids=lambda p: f"P{p[0]}-K{p[1]}")
def test_bidirectional_rounds_against_the_oracle_of_the_padded_scene(rd, oracle, pad):
    """reverse = 3 on small_scene(): k_shade_light, k_connect and the light vertex's mat_load.  Splat order is free, so two GPU
    runs are not compared; each padding is held per pixel to the oracle's exhaustive split of the padded scene with the bars of
    test_gpu_exhaustive.test_rounds_do_not_depend_on_the_stack_variant: no pixel outside the summation-order bound, the bit-exact
    classes exact, counts equal, paths and path_rays exact, shadow_rays at most the oracle's."""
    sb, cam = padded("small", *pad)
    prm = round_params(3)
    g = rd.Scene(sb.to_desc())
    assert g.info().const_light == 1
    a, c, k = g.render_round(cam, prm, rd.generate_task_list(W, H))
    g.close()
    split = oracle.OracleScene(sb.to_desc()).render_round_split(cam, prm, oracle.generate_task_list(W, H), exhaustive=True)
    planes, s = B.check_split(a, c, split)
    exact = float((bits(a) == bits((split.main.astype(np.float64) + split.splat_sum).astype(np.float32))).all(axis=2).mean())
    record_parity(f"gpu_thresholds.bdpt[small P {pad[0]} K {pad[1]} reverse 3]", **B.record_fields(s), bit_identical=exact,
                  path_rays_delta=int(k.path_rays) - int(split.counters.path_rays))
    assert split.n_splats > 0 and generic_light_vertices(split) > 0
    assert s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["exact_n0"] == s["exact_n1"] == 1.0, (pad, s)
    assert k.path_rays == split.counters.path_rays and k.paths == split.counters.paths and k.shadow_rays <= split.counters.shadow_rays, pad


def generic_light_vertices(split):
    return int(sum(split.lv_kind[kind] for kind in (capi.BXDF_MIRROR, capi.BXDF_DIELECTRIC)))


# ======================================================================= whole kernels: feature planes
PLANES = ("albedo", "normal", "depth", "tri", "hops")


def planes_differ(got, want):
    """Pixels that differ, per plane: float planes as bits, integer planes as integers."""
    out = []
    for g_, w_ in zip(got, want):
        d = (bits(g_) != bits(w_)) if g_.dtype == np.float32 else (g_ != w_)
        out.append(int(d.reshape(d.shape[0], d.shape[1], -1).any(axis=-1).sum()))
    return out


@pytest.mark.parametrize("scene", ["small", "small-byte-albedo", "zoo"])
def test_first_hit_planes_equal_the_unpadded_planes(rd, scene):
    """rgk_render_aov (k_aov_gather: surface_point's mat_load, the albedo of the renumbered record, the bump map's slopes through
    the moved table): albedo, normal, depth and triangle id of every (P, K), bit for bit.  The triangle plane does not move with
    the material numbers."""
    prm, tiles = round_params(0), rd.generate_task_list(W, H)
    want = None
    for P, K in [(0, 0)] + PADS:
        sb, cam = padded(scene, P, K)
        g = rd.Scene(sb.to_desc())
        got = g.render_aov(cam, prm, tiles, sentinel=7)
        g.close()
        if want is None:
            want = got
            assert (want[3] >= 0).mean() > 0.5 and float(want[0].max()) > 0.0 and len(np.unique(bits(want[0]).reshape(-1, 3), axis=0)) > 3
            continue
        differ = planes_differ(got, want)
        record_parity(f"gpu_thresholds.aov[{scene} P {P} K {K}]", **{f"{n}_differs": d for n, d in zip(PLANES, differ)},
                      bit_identical=1.0 - max(differ) / (W * H), outside=max(differ))
        assert differ == [0, 0, 0, 0], (scene, P, K, differ)


def test_followed_planes_equal_the_unpadded_planes(rd):
    """rgk_render_aov_chain at max_hops 4 on the hall of tests/chain_ref.py (k_aov_hop: mirrors, glass, a transparent quad, a mix,
    a bump-mapped mirror whose few-valued float bump map is a byte texture with a table of the scene's own) under P = 64, K = 3:
    albedo, normal, depth, triangle id and hops of the unpadded hall, bit for bit."""
    cam, prm, tiles = CR.hall_camera(), CR.hall_params(), rd.generate_task_list(CR.HALL_W, CR.HALL_H)
    out = []
    for P, K in ((0, 0), (64, 3)):
        sb = PAD.pad(CR.hall(), P, K)
        g = rd.Scene(sb.to_desc())
        assert g.info().n_palettized_textures == 2                  # checker and bump: tables at 256 K and 256 (K + 1)
        out.append(g.render_aov_chain(cam, prm, tiles, 4, sentinel=7))
        g.close()
    differ = planes_differ(out[1], out[0])
    record_parity("gpu_thresholds.aov-chain[hall P 64 K 3 max_hops 4]", **{f"{n}_differs": d for n, d in zip(PLANES, differ)},
                  bit_identical=1.0 - max(differ) / (CR.HALL_W * CR.HALL_H), outside=max(differ), followed=float((out[0][4] > 0).mean()))
    assert (out[0][4] > 0).mean() > 0.05 and int(out[0][4].max()) >= 2
    assert differ == [0, 0, 0, 0, 0], differ
