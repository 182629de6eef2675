"""CPU suite: pins and exercises the oracle (oracle/rgk_cpu.cpp) -- no GPU needed.

Pinned against the reference: the Halton radical inverse (golden vectors produced by the
reference's own external/halton_sampler.h, tests/golden/halton_faure.npz, generator
tools/make_fixtures.py).  Everything else is checked against closed forms: the reference
ships no tests or golden vectors and does not build here --
"parity unpinned" there.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from rgk_amd import capi
from rgk_amd.config import make_camera, make_params
from rgk_amd.scene import SceneBuilder

from conftest import ROOT, make_rays

GOLD = os.path.join(ROOT, "tests", "golden")


# ----------------------------------------------------------------------- sampler (a3)
def test_halton_matches_reference_golden_vectors(oracle):
    z = np.load(os.path.join(GOLD, "halton_faure.npz"))
    idx, ref = z["index"], z["values"]
    L = oracle.lib()
    mine = np.array([[L.orc_halton_raw(d, int(i)) for i in idx] for d in range(256)], dtype=np.float32)
    assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32))  # bit-exact, all 256 dimensions


# sha256 of index + values of tests/golden/halton_faure.npz: what the reference's header produced (tools/make_fixtures.py prints it)
HALTON_SHA256 = "98261b5c876f183554e54cd1afdfbc90229adab82ef78b8be8a30c4698b1e454"


def test_halton_fixture_regenerates_from_reference_header():
    """The golden vectors are the header's own output: their checksum is always checked; where oracle/_ref/halton_ref is
    built, the header regenerates them bit for bit."""
    import hashlib
    z = np.load(os.path.join(GOLD, "halton_faure.npz"))
    assert z["index"].dtype == np.uint32 and z["values"].dtype == np.float32 and z["values"].shape == (256, len(z["index"]))
    assert hashlib.sha256(z["index"].tobytes() + z["values"].tobytes()).hexdigest() == HALTON_SHA256
    exe = os.path.join(ROOT, "oracle", "_ref", "halton_ref")
    if not os.path.exists(exe):
        return   # the reference is not at hand: checksum only
    out = subprocess.run([exe, "256"] + [str(int(i)) for i in z["index"]], capture_output=True, check=True).stdout
    assert np.array_equal(np.frombuffer(out, dtype=np.float32).reshape(256, -1).view(np.uint32), z["values"].view(np.uint32))


LTC_SHA256 = {  # rgk_amd/data/ltc_<name>.f32: 64 x 64 x {m0, m2, m4, m6, amplitude} float32
    "ggx": "a7ca69cce519b31231ef769303dd5f19985550642f802b67d3c19752925bed8f",
    "beckmann": "73bbe6061c8e3f2b75c8aaef25854531b65869cfd5676704b555f8021f5271fb",
}


def test_ltc_tables_are_the_references_and_regenerate_from_its_source():
    """a12 pinned at the data level: the LTC fit tables both the oracle and the HIP path interpolate are the numeric initialisers
    of the reference's src/LTC/ltc_ggx.cpp / ltc_beckmann.cpp (tabM, tabAmplitude), rounded to float as mat33::operator
    glm::mat3() rounds them on every read.  The committed files carry a checksum (always checked); where the reference tree is
    present they are regenerated from its source text and must come out byte-identical."""
    import hashlib
    import importlib.util
    for name, want in LTC_SHA256.items():
        blob = open(os.path.join(ROOT, "rgk_amd", "data", f"ltc_{name}.f32"), "rb").read()
        assert len(blob) == 64 * 64 * 5 * 4 and hashlib.sha256(blob).hexdigest() == want, name
    ref = os.environ.get("RGK_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(ref, "src", "LTC", "ltc_ggx.cpp")):
        return   # the reference tree is not at hand: checksum only
    spec = importlib.util.spec_from_file_location("extract_ltc_tables", os.path.join(ROOT, "tools", "extract_ltc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in LTC_SHA256:
        rec = mod.extract(name)
        assert rec.dtype == np.float32 and rec.shape == (4096, 5)
        assert rec.tobytes() == open(os.path.join(ROOT, "rgk_amd", "data", f"ltc_{name}.f32"), "rb").read(), name
        # the oracle reads the same numbers: LTC::get_bilinear at a grid point returns the table entry itself


def test_pinned_libm_is_correctly_rounded_to_half_an_ulp(oracle):
    """include/rgk_libm.h: sin / cos / acos / asin / atan2 as fixed sequences of IEEE double operations (shared with the HIP
    kernels, so both sides produce the same bits).  Against numpy's double-precision functions: never more than 0.501 ulp
    from the exact value, i.e. the correctly rounded float except in ~5e-6 of the cases, where it is the other neighbour."""
    L = oracle.lib()
    rng = np.random.default_rng(0)

    def run(fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(a if b is None else b, np.float32)
        out = np.zeros(len(a), np.float32)
        assert L.orc_libm(fn, len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
        return out

    def max_ulp(got, ref64):
        sp = np.spacing(np.abs(ref64.astype(np.float32))).astype(np.float64)
        sp[sp == 0] = np.finfo(np.float32).tiny
        return float((np.abs(got.astype(np.float64) - ref64) / sp).max())
    x = np.concatenate([rng.uniform(0, 2 * np.pi, 400000), rng.uniform(-100, 100, 100000), [0.0, np.pi / 2, np.pi, 2 * np.pi]]).astype(np.float32)
    assert max_ulp(run(0, x), np.sin(x.astype(np.float64))) < 0.501
    assert max_ulp(run(1, x), np.cos(x.astype(np.float64))) < 0.501
    u = np.concatenate([rng.uniform(-1, 1, 400000), 1 - rng.uniform(0, 1e-3, 50000), -1 + rng.uniform(0, 1e-3, 50000), [1, -1, 0, 0.5, -0.5]]).astype(np.float32)
    assert max_ulp(run(2, u), np.arccos(u.astype(np.float64))) < 0.501
    assert max_ulp(run(3, u), np.arcsin(u.astype(np.float64))) < 0.501
    d = rng.normal(size=(400000, 2)).astype(np.float32)
    assert max_ulp(run(4, d[:, 0], d[:, 1]), np.arctan2(d[:, 0].astype(np.float64), d[:, 1].astype(np.float64))) < 0.501
    assert run(2, [1.0, -1.0])[0] == 0.0 and run(2, [1.0, -1.0])[1] == np.float32(np.pi) and np.isnan(run(2, [1.5, np.nan])).all()
    sp = run(4, [0.0, 0.0, 1.0, -1.0], [1.0, -1.0, 0.0, 0.0])
    assert list(sp) == [0.0, np.float32(np.pi), np.float32(np.pi / 2), -np.float32(np.pi / 2)]


def test_halton_known_values(oracle):
    L = oracle.lib()
    # SURVEY 8(c) probes of the vendored header
    assert L.orc_halton_raw(0, 1) == 0.5
    assert abs(L.orc_halton_raw(1, 1) - 0.333333313) < 1e-9
    assert abs(L.orc_halton_raw(2, 1) - 0.599999905) < 1e-9
    assert abs(L.orc_halton_raw(63, 255) - 0.241157532) < 1e-9


def test_sampler_contract_range_and_rotation(oracle):
    rng = np.random.default_rng(1)
    n = 50000
    seed = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    idx = rng.integers(0, 1 << 20, n).astype(np.uint32)
    dim = rng.integers(0, 80, n).astype(np.uint32)  # beyond 64 -> counter-based fallback
    for is2d in (0, 1):
        u = oracle.sampler_eval(seed, idx, dim, is2d)
        assert (u >= 0).all() and (u < 1).all()
    # same (index, dim), different pixel seed -> a pure toroidal shift of the Halton point
    s0 = np.full(256, 123, np.uint32); s1 = np.full(256, 99999, np.uint32)
    i = np.arange(256, dtype=np.uint32); d = np.full(256, 5, np.uint32)
    a, b = oracle.sampler_eval(s0, i, d, 1), oracle.sampler_eval(s1, i, d, 1)
    sh = np.mod(b - a, 1.0)
    assert np.allclose(sh, sh[0], atol=2e-7) or np.allclose(np.minimum(sh, 1 - sh), np.minimum(sh[0], 1 - sh[0]), atol=2e-7)


def test_halton_2d_points_are_well_distributed(oracle):
    # first 256 points of the low 2-D dimensions cover an 8x8 grid evenly (large prime bases need
    # more points than 256 to stratify in 2-D; those dimensions only drive deep bounces)
    n = 256
    for k in (0, 1, 2, 3):
        u = oracle.sampler_eval(np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), np.full(n, k, np.uint32), 1)
        h, _, _ = np.histogram2d(u[:, 0], u[:, 1], bins=(8, 8), range=((0, 1), (0, 1)))
        assert h.min() >= 1 and h.max() <= 12


def test_reference_stratified_sampler_strata(oracle):
    """src/sampler.cpp:85-116: every 2-D set holds exactly one point per cell of the sqrt(n) grid,
    every 1-D set one point per stratum; 20 spp rounds up to 25 (round_up_to_square :77-84)."""
    L = oracle.lib()
    for spp, n in ((16, 16), (20, 25)):
        nd = 6
        o1 = np.zeros((n, nd), np.float32); o2 = np.zeros((n, nd, 2), np.float32)
        L.orc_stratified_sample(42 + 0x42424242, spp, n, nd, o1.ctypes.data, o2.ctypes.data)
        sq = int(round(math.sqrt(n)))
        for d in range(nd):
            assert sorted(np.floor(o1[:, d] * n).astype(int).tolist()) == list(range(n))
            cells = (np.floor(o2[:, d, 1] * sq) * sq + np.floor(o2[:, d, 0] * sq)).astype(int)
            assert sorted(cells.tolist()) == list(range(n))


# ----------------------------------------------------------------------- geometry helpers
def single_plane_scene(albedo=(0.5, 0.5, 0.5), light=None, sky=None, half=10.0, kind=capi.BXDF_DIFFUSE, **mat):
    sb = SceneBuilder()
    m = sb.new_material("floor", kind)
    m["tex_diffuse"] = sb.create_solid_texture(albedo)
    m.update(mat)
    sb.register_material(m)
    T = np.eye(4, dtype=np.float32); T[0, 0] = T[2, 2] = half
    sb.add_primitive("plane", T, "floor")
    if light:
        sb.add_point_light(*light)
    if sky:
        sb.set_skybox_color(*sky)
    return sb


def test_direct_illumination_closed_form(oracle):
    """One diffuse plane, one point light, depth 1: L = I * color * albedo/pi * cos(theta) / d^2
    at every visible point (path_tracer.cpp:437-457 with BxDFDiffuse::value)."""
    albedo, I, lpos = (0.6, 0.5, 0.4), 50.0, (1.0, 3.0, -0.5)
    sb = single_plane_scene(albedo, light=(lpos, (1.0, 0.9, 0.8), I, 0.0))
    sc = oracle.OracleScene(sb.to_desc())
    W = H = 32
    cam = make_camera((0, 4, 0.001), (0, 0, 0), (0, 1, 0), fov=40, xres=W, yres=H)
    prm = make_params(W, H, 4, 1, clamp=1e7, russian=-1.0)
    acc, cnt, c = sc.render_round(cam, prm, oracle.generate_task_list(W, H))
    img = acc / cnt[..., None]
    # reconstruct hit points of pixel centres
    L = oracle.lib()
    ref = np.zeros_like(img)
    for y in range(H):
        for x in range(W):
            r = np.zeros(6, np.float32)
            L.orc_camera_ray(C.byref(cam), x, y, W, H, np.array([0.5, 0.5], np.float32).ctypes.data, None, r.ctypes.data)
            t = -r[1] / r[4]
            p = r[:3] + t * r[3:]
            v = np.array(lpos) - p
            d2 = float(v @ v)
            cos = v[1] / math.sqrt(d2)
            ref[y, x] = I * np.array([1.0, 0.9, 0.8]) * np.array(albedo) / math.pi * cos / d2
    assert np.allclose(img, ref, rtol=0.03, atol=1e-4)  # 4 jittered samples vs the pixel-centre value
    assert c.shadow_rays == c.paths and c.path_rays == c.paths


def test_sky_only_and_no_light_define_zero_nee(oracle):
    """Q15: with no lights NEE contributes nothing; a sky ray returns color*intensity (scene.cpp:748-751)."""
    sb = single_plane_scene(sky=((0.2, 0.4, 0.8), 0.5), half=0.25)
    sc = oracle.OracleScene(sb.to_desc())
    W = H = 16
    cam = make_camera((0, 1, 0.001), (0, 0, 0), (0, 1, 0), fov=120, xres=W, yres=H)
    prm = make_params(W, H, 2, 1, russian=-1.0)
    acc, cnt, c = sc.render_round(cam, prm, oracle.generate_task_list(W, H))
    img = acc / cnt[..., None]
    assert np.allclose(img[0, 0], [0.1, 0.2, 0.4], atol=1e-6)      # corner pixels miss the small plane
    assert np.allclose(img[H // 2, W // 2], 0.0)                   # the plane itself is unlit
    assert c.shadow_rays == 0


def test_white_furnace_series(oracle):
    """Closed white-ish diffuse box with one emissive wall is hard to close-form under the reference's
    estimator (Q1-Q4); instead check energy monotonicity in depth and the RR unbiasedness on average."""
    from rgk_amd.workloads import Workload
    wl = Workload("cornell-256", scale=0.125, spp=64)
    sc = oracle.OracleScene(wl.builder.to_desc())
    tiles = oracle.generate_task_list(wl.xres, wl.yres)
    means = []
    for depth in (1, 2, 4):
        prm = make_params(wl.xres, wl.yres, wl.multisample, depth, clamp=20.0, russian=-1.0)
        acc, cnt, _ = sc.render_round(wl.camera, prm, tiles)
        means.append(float((acc / cnt[..., None]).mean()))
    assert means[0] < means[1] < means[2]
    prm_rr = make_params(wl.xres, wl.yres, wl.multisample, 4, clamp=1e7, russian=0.74)
    prm_no = make_params(wl.xres, wl.yres, wl.multisample, 4, clamp=1e7, russian=-1.0)
    a, c1, _ = sc.render_round(wl.camera, prm_rr, tiles)
    b, c2, _ = sc.render_round(wl.camera, prm_no, tiles)
    # Q4: 1/r is applied from the 2nd vertex although the roulette also runs at the 1st: E[rr] = r * E[no rr]
    # for everything beyond the first vertex; just check the two are of the same order and rr <= no-rr on average
    assert 0.5 < (a / c1[..., None]).mean() / (b / c2[..., None]).mean() < 1.05


# ----------------------------------------------------------------------- triangle test / traversal (a7, a8)
def test_triangle_intersection_kats(oracle):
    sb = SceneBuilder()
    m = sb.new_material("m", capi.BXDF_DIFFUSE); sb.register_material(m)
    # one triangle in the z=0 plane + a distant one to give the scene a diameter (epsilon = 1e-5 * diag)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [50, 50, 50], [51, 50, 50], [50, 51, 50]], np.float32)
    nrm = np.tile([0, 0, 1], (6, 1)).astype(np.float32)
    sb.add_mesh(pos, nrm, np.zeros((6, 2), np.float32), np.tile([1, 0, 0], (6, 1)).astype(np.float32), [[0, 1, 2], [3, 4, 5]], 0)
    sc = oracle.OracleScene(sb.to_desc())
    L = oracle.lib()
    eps = sc.info().epsilon

    def test(o, d):
        d = np.array(d, np.float64); d /= np.linalg.norm(d)
        ray = np.array(list(o) + list(d) + [0, 1e4], np.float32)
        out = np.zeros(3, np.float32)
        hit = L.orc_test_intersection(sc.h, 0, ray.ctypes.data, out.ctypes.data)
        return hit, out
    hit, (t, a, b) = test((0.25, 0.25, 1), (0, 0, -1))
    assert hit and abs(t - 1) < 1e-6 and abs(a - 0.25) < 1e-6 and abs(b - 0.25) < 1e-6
    assert test((0.25, 0.25, -1), (0, 0, 1))[0]            # no back-face culling
    assert test((0.5, 0.5, 1), (0, 0, -1))[0]              # alpha + beta == 1 is inside
    assert not test((0.51, 0.51, 1), (0, 0, -1))[0]
    assert test((0, 0, 1), (0, 0, -1))[0]                  # vertex
    assert not test((-0.01, 0.5, 1), (0, 0, -1))[0]
    assert not test((0.25, 0.25, 1), (1, 0, -0.5 * eps))[0]   # |d.n| < eps: "parallel" (Q9, scene-scale dependent)
    assert test((0.25, 0.25, 1), (1, 0, -0.1))[0] is not None
    # the "uncommon" branch: |q1.x| < eps in the projected plane (primitives.cpp:141-147)
    sb2 = SceneBuilder(); sb2.register_material(sb2.new_material("m", capi.BXDF_DIFFUSE))
    pos2 = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [50, 50, 50], [51, 50, 50], [50, 51, 50]], np.float32)
    sb2.add_mesh(pos2, nrm, np.zeros((6, 2), np.float32), np.tile([1, 0, 0], (6, 1)).astype(np.float32), [[0, 1, 2], [3, 4, 5]], 0)
    sc2 = oracle.OracleScene(sb2.to_desc())
    ray = np.array([0.25, 0.5, 1, 0, 0, -1, 0, 1e4], np.float32); out = np.zeros(3, np.float32)
    assert L.orc_test_intersection(sc2.h, 0, ray.ctypes.data, out.ctypes.data) == 1
    assert abs(out[1] - 0.5) < 1e-6 and abs(out[2] - 0.25) < 1e-6   # alpha along v1, beta along v2


def test_kd_traversal_equals_brute_force(oracle, cornell):
    sc = oracle.OracleScene(cornell.builder.to_desc())
    L = oracle.lib()
    rng = np.random.default_rng(3)
    n = 400
    o = rng.uniform(-0.9, 0.9, (n, 3)).astype(np.float32); o[:, 1] += 1
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = make_rays(o, d)
    hits, _ = sc.trace_closest(rays)
    ntri = len(cornell.builder.F)
    out = np.zeros(3, np.float32)
    for i in range(n):
        best, bt = -1, np.inf
        for t in range(ntri):
            if L.orc_test_intersection(sc.h, t, rays[i].ctypes.data, out.ctypes.data) and 0 <= out[0] < bt:
                best, bt = t, out[0]
        assert hits["tri"][i] == best and (best < 0 or hits["t"][i] == np.float32(bt))


def test_ignore_triangle_and_visibility(oracle, cornell):
    sc = oracle.OracleScene(cornell.builder.to_desc())
    rays = make_rays(np.array([[0, 1, 0]], np.float32), np.array([[0, -1, 0]], np.float32))
    h, _ = sc.trace_closest(rays)
    assert h["tri"][0] >= 0
    h2, _ = sc.trace_closest(rays, ignore=np.array([h["tri"][0]], np.int32))
    assert h2["tri"][0] != h["tri"][0]
    vis, _ = sc.visibility(np.array([[0, 1, 0.9], [0, 1, 0.9]], np.float32), np.array([[0, 1.5, 0.9], [0, 1, -3.0]], np.float32))
    assert vis.tolist() == [1, 0]


# ----------------------------------------------------------------------- textures, LTC (a12, a14)
def test_texture_sampling_kats(oracle):
    sb = SceneBuilder()
    tex = np.arange(4 * 3 * 3, dtype=np.float32).reshape(3, 4, 3) / 10.0  # h=3, w=4
    t = sb.add_image_texture("t", tex)
    m = sb.new_material("m", capi.BXDF_DIFFUSE); m["tex_diffuse"] = t; sb.register_material(m)
    sb.add_primitive("plane", np.eye(4, dtype=np.float32), "m")
    sc = oracle.OracleScene(sb.to_desc())
    L = oracle.lib()

    def sample(u, v):
        rgb = np.zeros(3, np.float32); r = C.c_float(); b = C.c_float()
        L.orc_texture_sample(sc.h, t, np.array([u, v], np.float32).ctypes.data, rgb.ctypes.data, C.byref(r), C.byref(b))
        return rgb, r.value, b.value
    rgb, r, b = sample((1 + 0.5) / 4, (1 + 0.5) / 3)          # texel centre -> that texel
    assert np.allclose(rgb, tex[1, 1])
    assert np.isclose(r, tex[1, 1].mean() - tex[1, 2].mean()) and np.isclose(b, tex[1, 1].mean() - tex[2, 1].mean())
    rgb2, _, _ = sample(1 + (1 + 0.5) / 4, -2 + (1 + 0.5) / 3)  # repeat wrap (glm::repeat)
    assert np.allclose(rgb2, tex[1, 1])
    rgb3, _, _ = sample(2.0 / 4, 1.5 / 3)                      # halfway between texel 1 and 2 in x
    assert np.allclose(rgb3, 0.5 * (tex[1, 1] + tex[1, 2]))
    _, r_edge, _ = sample(3.5 / 4, 0.5 / 3)                    # clamp-to-edge on the +1 neighbour (Q13)
    assert r_edge == 0.0


def test_8bit_textures_equal_float_textures(oracle):
    """RGK_TEX_RGB8 (bytes + byte->float table) must give exactly the texels of RGK_TEX_RGB32F."""
    from rgk_amd.scene import gamma_lut
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    images = []
    for as_float in (True, False):
        sb = SceneBuilder()
        t = sb.add_image_texture("f", gamma_lut()[img]) if as_float else sb.add_image_texture8("b", img)
        m = sb.new_material("m", capi.BXDF_DIFFUSE); m["tex_diffuse"] = t; m["tex_bump"] = t; sb.register_material(m)
        T = np.eye(4, dtype=np.float32); T[0, 0] = T[2, 2] = 2.0
        sb.add_primitive("plane", T, "m", texscale=(3.0, 2.0, 1.0))
        sb.add_point_light((0.5, 2.0, 0.3), (1, 1, 1), 10.0, 0.0)
        sc = oracle.OracleScene(sb.to_desc())
        cam = make_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), fov=50, xres=48, yres=48)
        acc, cnt, _ = sc.render_round(cam, make_params(48, 48, 4, 2, bumpscale=5.0), oracle.generate_task_list(48, 48))
        images.append(acc)
    assert images[0].max() > 0 and np.array_equal(images[0], images[1])


def test_ltc_pdf_normalisation_and_sampling(oracle):
    """The LTC pdf integrates to ~amplitude * |sin(theta)|^-2-ish scale quirk aside: at normal-ish incidence and
    rough alpha it is a smooth lobe; sampled directions stay in the upper hemisphere and are unit length."""
    sb = SceneBuilder()
    for name, kind in (("ggx", capi.BXDF_LTC_GGX), ("bek", capi.BXDF_LTC_BECKMANN)):
        m = sb.new_material(name, kind); m["roughness"] = 0.5; m["tex_color"] = sb.create_solid_texture((1, 1, 1))
        sb.register_material(m)
    sb.add_primitive("plane", np.eye(4, dtype=np.float32), "ggx")
    sc = oracle.OracleScene(sb.to_desc())
    L = oracle.lib()
    rng = np.random.default_rng(5)
    Vr = np.array([0.6, 0.0, 0.8], np.float32)
    for mat in (0, 1):
        vals = []
        for _ in range(2000):
            u = rng.random(2).astype(np.float32)
            d = np.zeros(3, np.float32); w = np.zeros(3, np.float32); leak = C.c_int()
            L.orc_bxdf_sample(sc.h, mat, Vr.ctypes.data, np.zeros(2, np.float32).ctypes.data, u.ctypes.data, d.ctypes.data, w.ctypes.data, C.byref(leak))
            assert abs(np.linalg.norm(d) - 1) < 1e-5 and d[2] > 0 and leak.value == 0
            out = np.zeros(3, np.float32)
            L.orc_bxdf_value(sc.h, mat, d.ctypes.data, Vr.ctypes.data, np.zeros(2, np.float32).ctypes.data, out.ctypes.data)
            vals.append(out[0])
        vals = np.array(vals)
        assert np.isfinite(vals).all() and (vals >= 0).all() and vals.mean() > 0.05
        out = np.zeros(3, np.float32)   # below the horizon -> 0 (bxdf.hpp:110)
        L.orc_bxdf_value(sc.h, mat, np.array([0, 0.6, -0.8], np.float32).ctypes.data, Vr.ctypes.data, np.zeros(2, np.float32).ctypes.data, out.ctypes.data)
        assert (out == 0).all()


def test_delta_bxdfs(oracle):
    sb = SceneBuilder()
    mir = sb.new_material("mirror", capi.BXDF_MIRROR); mir["tex_color"] = sb.create_solid_texture((0.9, 0.8, 0.7)); sb.register_material(mir)
    die = sb.new_material("glass", capi.BXDF_DIELECTRIC); die["ior"] = 1.5; die["tex_color"] = sb.create_solid_texture((1, 1, 1)); sb.register_material(die)
    tr = sb.new_material("air", capi.BXDF_TRANSPARENT); sb.register_material(tr)
    sb.add_primitive("plane", np.eye(4, dtype=np.float32), "mirror")
    sc = oracle.OracleScene(sb.to_desc())
    L = oracle.lib()
    Vi = np.array([0.6, 0.0, 0.8], np.float32); uv = np.zeros(2, np.float32)

    def samp(mat, u):
        d = np.zeros(3, np.float32); w = np.zeros(3, np.float32); leak = C.c_int()
        L.orc_bxdf_sample(sc.h, mat, Vi.ctypes.data, uv.ctypes.data, np.array(u, np.float32).ctypes.data, d.ctypes.data, w.ctypes.data, C.byref(leak))
        return d, w, leak.value
    d, w, leak = samp(0, (0.3, 0.3))
    assert np.allclose(d, [-0.6, 0, 0.8]) and np.allclose(w, [0.9, 0.8, 0.7]) and not leak
    d, w, leak = samp(2, (0.3, 0.3))
    assert np.allclose(d, -Vi) and leak
    # dielectric: Fresnel reflectance at cos=0.8, eta=1/1.5
    ct = 0.8; eta = 1 / 1.5; st2 = eta * eta * (1 - ct * ct); ctt = math.sqrt(1 - st2)
    Rs = (eta * ct - ctt) / (eta * ct + ctt); Rp = (eta * ctt - ct) / (eta * ctt + ct); R = 0.5 * (Rs * Rs + Rp * Rp)
    d, w, leak = samp(1, (R * 0.5, 0.1))      # u.x < R -> reflect
    assert np.allclose(d, [-0.6, 0, 0.8]) and not leak
    d, w, leak = samp(1, (R + 0.5 * (1 - R), 0.1))  # refract
    assert leak and np.allclose(d, [-0.6 * eta, 0, -ctt], atol=1e-6)


# ----------------------------------------------------------------------- driver / boundary host logic (a1, a2, 8b)
def test_task_list_order_and_seeds(oracle):
    tiles = oracle.generate_task_list(100, 70, seedstart=42, seedcount_base=5)
    assert len(tiles) == 4 * 3
    mids = np.array([((t.x0 + t.x1) / 2, (t.y0 + t.y1) / 2) for t in tiles])
    dist = np.hypot(mids[:, 0] - 50, mids[:, 1] - 35)
    assert (np.diff(dist) >= 0).all()                       # centre-out (render_driver.cpp:42-44)
    assert [t.seed for t in tiles] == [42 + 5 + i for i in range(len(tiles))]
    assert sorted((t.x0, t.y0) for t in tiles) == [(x, y) for x in (0, 32, 64, 96) for y in (0, 32, 64)]
    assert max(t.x1 for t in tiles) == 100 and max(t.y1 for t in tiles) == 70   # ragged last tiles


def test_round_accumulates_and_tiles_are_independent(oracle, cornell):
    sc = oracle.OracleScene(cornell.builder.to_desc())
    prm = cornell.params()
    tiles = oracle.generate_task_list(cornell.xres, cornell.yres)
    acc, cnt, c = sc.render_round(cornell.camera, prm, tiles)
    assert (cnt == prm.multisample).all() and c.paths == cnt.sum()
    # rendering the tile list in two halves gives the same image, bit for bit (seeds ride with the tiles)
    half = len(tiles) // 2
    a2 = np.zeros_like(acc); c2 = np.zeros_like(cnt)
    sc.render_round(cornell.camera, prm, (capi.Tile * half)(*tiles[:half]), a2, c2)
    sc.render_round(cornell.camera, prm, (capi.Tile * (len(tiles) - half))(*tiles[half:]), a2, c2)
    assert np.array_equal(acc, a2) and np.array_equal(cnt, c2)
    # a second round with the next seeds adds on top (EXRTexture::AddPixel)
    tiles2 = oracle.generate_task_list(cornell.xres, cornell.yres, seedcount_base=len(tiles))
    sc.render_round(cornell.camera, prm, tiles2, acc, cnt)
    assert (cnt == 2 * prm.multisample).all()
    assert not np.array_equal(acc, 2 * a2)


def test_stratified_and_halton_estimators_agree(oracle, cornell):
    """The build's Halton sampler and the reference's active StratifiedSampler estimate the same image:
    their difference is within twice the difference of two independent stratified renders."""
    from rgk_amd.workloads import Workload
    wl = Workload("cornell-256", scale=0.125, spp=64)
    sc = oracle.OracleScene(wl.builder.to_desc())

    def render(sampler, base):
        tiles = oracle.generate_task_list(wl.xres, wl.yres, seedcount_base=base)
        acc, cnt, _ = sc.render_round(wl.camera, wl.params(sampler), tiles)
        return acc / cnt[..., None]
    h = render(capi.SAMPLER_HALTON, 0)
    s1, s2 = render(capi.SAMPLER_STRATIFIED, 0), render(capi.SAMPLER_STRATIFIED, 1000)
    n = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert n(h, s1) < 2.0 * n(s2, s1)
    assert abs(h.mean() / s1.mean() - 1) < 0.05


# ----------------------------------------------------------------------- scenes the reference ships complete
REFERENCE_SCENES = ["rubiks-bump", "cube3", "box6", "cornell-box-spheres"]


@pytest.mark.parametrize("name", REFERENCE_SCENES)
def test_reference_scene_fixture_renders_and_regenerates(oracle, name):
    """tests/golden/scene_<name>.npz = the flat arrays the loader hands to Scene for scenes/<name>.json.
    The oracle renders it (finite, non-black, every path counted); where the reference tree is present the
    fixture is rebuilt from its config / mesh / texture files and must come out identical."""
    from rgk_amd.workloads import SceneFixture
    path = os.path.join(ROOT, "tests", "golden", "scene_%s.npz" % name)
    wl = SceneFixture(path, scale=0.06, spp=4)
    o = oracle.OracleScene(wl.builder.to_desc())
    acc, cnt, k = o.render_round(wl.camera, wl.params(), oracle.generate_task_list(wl.xres, wl.yres))
    assert np.isfinite(acc).all() and acc.max() > 0 and (cnt == wl.multisample).all()
    assert k.paths == wl.xres * wl.yres * wl.multisample
    ref = "/root/reference/scenes/%s.json" % name
    if not os.path.exists(ref):
        return
    from rgk_amd.config import Config
    sb = Config(ref).build_scene()
    sb.finalize()
    for a in ("V", "N", "T", "UV", "F", "FM"):
        assert np.array_equal(getattr(sb, a), getattr(wl.builder, a)), a
    assert len(sb.textures) == len(wl.builder.textures)
    for t0, t1 in zip(sb.textures, wl.builder.textures):
        assert t0["kind"] == t1["kind"]
        if t0["kind"] != 0:
            assert np.array_equal(t0["data"], t1["data"])


def test_oracle_reproduces_the_frozen_config0_image(oracle):
    """tests/golden/cornell_config0_half.npz: the oracle's accumulator for BASELINE configs[0] at half resolution,
    frozen when the GPU parity was established.  A change in the oracle shows up here (up to libm's last bits)."""
    from rgk_amd.workloads import Workload
    z = np.load(os.path.join(ROOT, "tests", "golden", "cornell_config0_half.npz"))
    wl = Workload("cornell-256", scale=0.5)
    o = oracle.OracleScene(wl.builder.to_desc())
    acc, cnt, k = o.render_round(wl.camera, wl.params(), oracle.generate_task_list(wl.xres, wl.yres))
    assert np.array_equal(cnt, z["count"])
    assert [k.paths, k.path_rays, k.shadow_rays] == [int(v) for v in z["counters"]]
    assert np.linalg.norm(acc - z["accum"]) / np.linalg.norm(z["accum"]) <= 1e-6
