"""GPU suite (-m gpu): rgk_scene_refit, everything it rewrites, bit for bit.

A refit that gets a shading record, a light table, a frame cache or a pad wrong still renders a plausible picture, so every
bar here is equality of bits against the oracle (rounds with every ray answered by exhaustive search, feature planes composed
from exhaustive first hits, exhaustive closest hits and visibility) or against a fresh scene of the mesh the handle now holds.
The cases and their references are tests/refit_cases.py; that the moves change what they are meant to change is asserted on
the reference side alone, in tests/test_refit_cpu.py.

    a  shading records   k_refit_shade: normals and tangents together, one without the other, after a positions-only refit
    b  light tables      area order inside a light, power shares, total areal power; the kept normals feed vertex-A normals
    c  frame caches      entry points, beams, the pixel list and the constant-light decision across a refit, 16 switch sets
    d  geometry          epsilon by 1e3, flat <-> thick, coincident <-> apart, tiny scenes, no coherence, triangles that collapse
    e  arguments         a refused refit leaves the scene as it was
"""
import functools

import numpy as np
import pytest

import bdpt_ref as B
import refit_cases as RC
import trace_ref as T
from conftest import record_parity
from test_gpu_exhaustive import assert_equal_hits, assert_same_frame, gpu_scene

pytestmark = pytest.mark.gpu

W, H = RC.W, RC.H


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counters(k):
    return (int(k.paths), int(k.path_rays), int(k.shadow_rays))


def assert_round_equals_the_oracle(tag, got, split):
    """The bars of test_gpu_memstate.test_unidirectional_baselines_equal_the_oracle: every pixel exact, counts, paths and
    path_rays the oracle's, shadow_rays at most the oracle's."""
    a, c, k = got
    assert split.n_splats == 0
    _, s = B.check_split(a, c, split)
    k = counters(k)
    record_parity(tag, **B.record_fields(s), bit_identical=s["exact_n0"], shadow_rays_gpu_over_oracle=k[2] / max(1, split.counters.shadow_rays))
    assert (s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["share_n0"] == 1.0 and s["exact_n0"] == 1.0 and
            (k[0], k[1]) == (split.counters.paths, split.counters.path_rays) and k[2] <= split.counters.shadow_rays), \
        (tag, s, k, (split.counters.paths, split.counters.path_rays, split.counters.shadow_rays))


def assert_same_rounds(tag, got, want):
    """Two lists of (accum, count, counters): equal bit for bit, counters too."""
    differ = 0
    for (a0, c0, k0), (a1, c1, k1) in zip(got, want):
        differ += int((bits(a0) != bits(a1)).any(axis=2).sum()) + int((c0 != c1).sum())
        assert counters(k0) == counters(k1), (tag, counters(k0), counters(k1))
    pixels = len(want) * W * H
    record_parity(tag, pixels=pixels, differing=differ, exact=1.0 - differ / pixels)
    assert differ == 0 and len(got) == len(want), (tag, differ)


# ----------------------------------------------------------------------- a. shading records
SHAPES = {   # name -> [(normals passed, tangents passed, mesh the handle then holds)] on the moved vertices; the step back follows
    "all-at-once": [(True, True, "111")],
    "normals-then-tangents": [(True, False, "110"), (False, True, "111")],
    "positions-then-all": [(False, False, "100"), (True, True, "111")],
}
VARIANTS = {"sphere-light-and-emitter": False, "point-light": True}   # name -> refit_cases.shade_case's `point`


@functools.lru_cache(maxsize=None)
def _fresh(rd, family, key, builder, point=False):
    """(feature planes, round) of a fresh scene of mesh `key`, once per builder."""
    c = RC.case_of(family, point)
    g = gpu_scene(rd, RC.with_mesh(c["make"], *c["mesh"][key]), builder)
    tiles = rd.generate_task_list(W, H)
    planes = g.render_aov(c["camera"], c["prm"], tiles) if family == "shade" else None
    round_ = g.render_round(c["camera"], c["prm"], tiles)
    info = g.info()
    g.close()
    return planes, round_, info


def _check_planes(tag, got, fresh, want):
    """Fresh scene: every plane bit for bit.  Oracle composition: the bars of test_gpu_post.test_features_equal_the_oracle_composition
    (triangle differs on at most 0.1 % of the pixels; depth, normal and albedo bit for bit wherever it is the same)."""
    differ = sum(int((bits(x) != bits(y)).sum()) for x, y in zip(got, fresh))
    ga, gn, gz, gt = got
    ra, rn, rz, rt = want
    same = gt == rt
    share = float((~same).mean())
    nb, ab = (int((bits(x[same]) != bits(y[same])).any(axis=-1).sum()) for x, y in ((gn, rn), (ga, ra)))
    zb = int((bits(gz[same]) != bits(rz[same])).sum())
    record_parity(tag, rays=W * H, hits=int((rt >= 0).sum()), differing=differ, tri_differs=share, depth_differs=zb, normal_differs=nb, albedo_differs=ab,
                  exact=1.0 - (zb + nb + ab + int((~same).sum())) / (W * H))
    assert differ == 0, (tag, "against a fresh scene", differ)
    assert share <= 0.001 and zb == 0 and nb == 0 and ab == 0, (tag, "against the oracle", share, zb, nb, ab)
    assert (gt >= 0).mean() > 0.5


def _shade_steps(c, shape):
    V1, N1, T1 = c["mesh"]["111"]
    return [(V1, N1 if n else None, T1 if t else None, key) for n, t, key in SHAPES[shape]] + [c["mesh"]["000"] + ("000",)]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("builder", ["host-sah", "device"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_refitted_shading_records(rd, oracle, variant, builder, shape):
    """k_refit_shade under every call shape.  After each step the feature planes equal, bit for bit, a fresh scene's of the
    vertices, normals and tangents the handle now holds and the oracle's composition, and a unidirectional round equals that
    fresh scene's round with its counters -- a step that passed normals only shows the old tangents with the new normals
    ("110"), so the uv and material words of the records, and the half a call did not name, survive.  Back at the start the
    round is the handle's very first round."""
    point = VARIANTS[variant]
    c = RC.shade_case(point)
    cam, prm, tiles = c["camera"], c["prm"], rd.generate_task_list(W, H)
    g = gpu_scene(rd, c["make"](), builder)
    first = got = g.render_round(cam, prm, tiles)
    for i, (V, N, Tn, key) in enumerate(_shade_steps(c, shape)):
        g.refit(V, N, Tn)
        tag = f"gpu_refit[shade {variant} {builder} {shape} step {i} -> {key}]"
        planes, round_, _ = _fresh(rd, "shade", key, builder, point)
        _check_planes(tag + ":aov", g.render_aov(cam, prm, tiles), planes, RC.oracle_planes(key, point))
        got = g.render_round(cam, prm, tiles)
        assert_same_rounds(tag + ":round against a fresh scene", [got], [round_])
    assert_same_rounds(f"gpu_refit[shade {variant} {builder} {shape} back at the first round]", [got], [first])
    g.close()


@pytest.mark.parametrize("builder", ["host-sah", "device"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_refitted_shading_rounds_equal_the_oracle(rd, oracle, variant, builder):
    """As built and after every step of every call shape, the unidirectional round equals the oracle's
    render_round_split(exhaustive = True) of the mesh the handle holds: every pixel exact, counts, paths and path_rays equal,
    shadow_rays at most the oracle's.

    The sphere-light-and-emitter scene is the first round held to the oracle in which an emitting surface is lit by another
    light.  It found the shading kernels adding B = clamp(emission) * contribution at once and A - B with the shadow ray, 9 of
    3015 pixels of the scene AS BUILT one bit off in a channel (4 to 14 on the moved meshes); the shadow ray now carries
    (sum + A) - (sum + B) (rgk_shade.h slot_add_keep)."""
    point = VARIANTS[variant]
    c = RC.shade_case(point)
    cam, prm, tiles = c["camera"], c["prm"], rd.generate_task_list(W, H)
    g = gpu_scene(rd, c["make"](), builder)
    bad = []

    def held(tag, key):
        try:
            assert_round_equals_the_oracle(f"gpu_refit[shade {variant} {builder} {tag}]:oracle", g.render_round(cam, prm, tiles), RC.oracle_round("shade", key, point=point))
        except AssertionError as e:
            bad.append(str(e)[:300])
    held("as built", "000")
    for shape in SHAPES:
        for i, (V, N, Tn, key) in enumerate(_shade_steps(c, shape)):
            g.refit(V, N, Tn)
            held(f"{shape} step {i} -> {key}", key)
    g.close()
    assert not bad, bad


# ----------------------------------------------------------------------- b. light tables
def _lights_sequence(c):
    V1, N1, _ = c["mesh"]["11"]
    return [("refit(V1)", (V1, None), "10"), ("refit(V1, N1)", (V1, N1), "11"), ("refit(V1, N1), refit(V1)", (V1, None), "11")]


@pytest.mark.parametrize("builder", ["host-sah", "device"])
def test_refitted_light_tables(rd, oracle, builder):
    """Areas, vertices, vertex-A normals, powers and the sort by area, after a stretch that reverses the order inside both
    lights of several triangles and moves every power share.  info() is a fresh scene's and the oracle's; the round is a fresh
    scene's bit for bit after refit(V1), after refit(V1, N1), and after the refit(V1) with no normals that follows -- which a
    fresh scene of (V1, N1) must equal: the normals the scene kept feed the lights' vertex-A normals.  One bidirectional round
    under the bars of test_gpu_memstate.test_bidirectional_rounds_against_the_oracle_in_both_runs."""
    c = RC.lights_case()
    cam, prm, tiles = c["camera"], c["prm"], rd.generate_task_list(W, H)
    g = gpu_scene(rd, c["make"](), builder)
    info0 = g.info()
    for name, (V, N), key in _lights_sequence(c):
        g.refit(V, N)
        _, round_, fi = _fresh(rd, "lights", key, builder)
        gi, oi = g.info(), RC.oracle_scene("lights", key)[0].info()
        for x in (fi, oi):
            assert gi.epsilon == x.epsilon and list(gi.bbox_min) == list(x.bbox_min) and list(gi.bbox_max) == list(x.bbox_max)
        assert gi.total_areal_power == fi.total_areal_power and gi.const_light == fi.const_light == 0
        assert abs(gi.total_areal_power - info0.total_areal_power) > 0.1 * info0.total_areal_power
        assert_same_rounds(f"gpu_refit[lights {builder} {name}]:round against a fresh scene", [g.render_round(cam, prm, tiles)], [round_])
    unmoved, moved, tilted = (_fresh(rd, "lights", k, builder)[1][0] for k in ("00", "10", "11"))
    assert (bits(unmoved) != bits(moved)).any(axis=2).mean() > 0.5 and (bits(moved) != bits(tilted)).any(axis=2).mean() > 0.1
    split = RC.oracle_round("lights", "11", reverse=3)
    a, cnt, k = g.render_round(cam, RC.params(reverse=3), tiles)
    _, s = B.check_split(a, cnt, split)
    k = counters(k)
    record_parity(f"gpu_refit[lights {builder} reverse 3]", **B.record_fields(s), path_rays_delta=k[1] - int(split.counters.path_rays))
    assert split.n_splats > 0
    assert (s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["exact_n0"] == 1.0 and s["exact_n1"] == 1.0 and
            (k[0], k[1]) == (split.counters.paths, split.counters.path_rays) and k[2] <= split.counters.shadow_rays), (s, k)
    g.close()


@pytest.mark.parametrize("builder", ["host-sah", "device"])
def test_refitted_light_rounds_equal_the_oracle(rd, oracle, builder):
    """After refit(V1) the round equals the oracle's exhaustive round on the moved mesh; after refit(V1, N1), and after the
    refit(V1) that follows, the oracle's for (V1, N1).

    The emissive fan and pair of this scene are lit by the quad and the sphere light: before the shading kernels' lit-emitter
    addition was made exact (test_refitted_shading_rounds_equal_the_oracle) 16 to 21 of 3015 pixels were not the oracle's bits."""
    c = RC.lights_case()
    cam, prm, tiles = c["camera"], c["prm"], rd.generate_task_list(W, H)
    g = gpu_scene(rd, c["make"](), builder)
    bad = []
    for name, (V, N), key in _lights_sequence(c):
        g.refit(V, N)
        try:
            assert_round_equals_the_oracle(f"gpu_refit[lights {builder} {name}]:oracle", g.render_round(cam, prm, tiles), RC.oracle_round("lights", key))
        except AssertionError as e:
            bad.append(str(e)[:300])
    g.close()
    assert not bad, bad


# ----------------------------------------------------------------------- c. frame caches
SWITCHES = [dict(entry_points=e, beam=b, last_vertex=l, const_light=c) for e in (0, 1) for b in (0, 2) for l in (0, 1) for c in (0, 1)]
VIEWS = {"host-sah-narrow": ("host-sah", "narrow"), "device-low": ("device", "low")}   # name -> (builder, view of refit_cases.cache_camera)


@pytest.mark.parametrize("tuning", SWITCHES, ids=["-".join(f"{k}{v}" for k, v in t.items()) for t in SWITCHES])
@pytest.mark.parametrize("view", list(VIEWS))
def test_frame_caches_do_not_outlive_a_refit(rd, oracle, view, tuning):
    """One handle of the point-light scene (const_light = 1), one camera, one tile list: two rounds of the frame (the second on
    capped entry lists), the refit, the same two rounds again.  The second pair is a fresh scene's of the moved mesh under the
    same switches, bit for bit with its counters, and the oracle's round; it is not the first pair.  The two (builder, camera)
    pairs are those through which lists kept across the refit were measured to change pixels (test_refit_cpu.py,
    profiles/refit_coverage.txt): on this small scene the entry lists are coarse and a capped ray that finds nothing is traced
    again from the root, so through most cameras stale lists heal themselves."""
    builder, cam_view = VIEWS[view]
    c = RC.shade_case(point=True)
    cam, prm, tiles = RC.cache_camera(cam_view), c["prm"], rd.generate_task_list(W, H)
    g = gpu_scene(rd, c["make"](), builder).set_tuning(**tuning)
    assert g.info().const_light == 1
    before = [g.render_round(cam, prm, tiles) for _ in range(2)]
    g.refit(*c["mesh"]["111"])
    assert g.info().const_light == 1
    after = [g.render_round(cam, prm, tiles) for _ in range(2)]
    g.close()
    f = gpu_scene(rd, RC.with_mesh(c["make"], *c["mesh"]["111"]), builder).set_tuning(**tuning)
    fresh = [f.render_round(cam, prm, tiles) for _ in range(2)]
    f.close()
    tag = f"gpu_refit[caches {view} " + " ".join(f"{k}={v}" for k, v in tuning.items())
    assert_same_rounds(tag + "]", after, fresh)
    for r in range(2):
        assert_round_equals_the_oracle(f"{tag} round {r}]", after[r], RC.oracle_round("shade", "111", point=True, cache_cam=cam_view))
        assert (bits(after[r][0]) != bits(before[r][0])).any(axis=2).mean() > 0.5


# ----------------------------------------------------------------------- d. geometry
GEOMETRY_BUILDERS = ("host-sah", "device", "device-karras")


@pytest.mark.parametrize("builder", GEOMETRY_BUILDERS)
@pytest.mark.parametrize("name", list(RC.GEOMETRY))
def test_refitted_geometry_equals_the_exhaustive_search(rd, oracle, name, builder):
    """After the move and after the move back: epsilon and the padded box are the oracle's of the held vertices; closest hits,
    plain and with the first hit ignored, and visibility equal the exhaustive search for every ray and pair."""
    scene, V0, V1 = RC.geometry_case(name)
    g = gpu_scene(rd, T.SCENES[scene](), builder)
    for step, V, osc, rays, ex, ig, ex2, a, b, vis in RC.geometry_reference(name):
        g.refit(V)
        assert_same_frame(g, osc)
        tag = f"gpu_refit[{name} {builder} {step}]"
        assert_equal_hits(tag + ":closest", rays, g.trace_closest(rays)[0], ex)
        assert_equal_hits(tag + ":ignore-first", rays, g.trace_closest(rays, ig)[0], ex2)
        vg = g.visibility(a, b)[0]
        differ = int((vg != vis).sum())
        record_parity(tag + ":visibility", rays=len(vg), hits=int((vis == 0).sum()), differing=differ, exact=1.0 - differ / len(vg))
        assert differ == 0, (tag, differ, np.nonzero(vg != vis)[0][:10])
    g.close()


# ----------------------------------------------------------------------- e. arguments
def test_a_refused_refit_leaves_the_scene_as_it_was(rd, oracle):
    """rgk_scene_refit with null vertices or a null scene returns -1 and the scene renders the bits it rendered before; the next
    refit, with nothing in flight, succeeds and renders the oracle's round of the moved mesh (point-light scene)."""
    c = RC.shade_case(point=True)
    cam, prm, tiles = c["camera"], c["prm"], rd.generate_task_list(W, H)
    g = gpu_scene(rd, c["make"](), "host-sah")
    lib = g.lib
    first = g.render_round(cam, prm, tiles)
    V1, N1, T1 = c["mesh"]["111"]
    assert lib.rgk_scene_refit(g.h, None, N1.ctypes.data, T1.ctypes.data) == -1 and lib.rgk_last_error()
    assert lib.rgk_scene_refit(None, V1.ctypes.data, None, None) == -1 and lib.rgk_scene_refit(None, None, None, None) == -1
    assert_same_rounds("gpu_refit[after refused refits]", [g.render_round(cam, prm, tiles)], [first])
    g.refit(V1, N1, T1)        # nothing is in flight: a refit after a failed one succeeds
    assert_round_equals_the_oracle("gpu_refit[refit after refused refits]", g.render_round(cam, prm, tiles), RC.oracle_round("shade", "111", point=True))
    g.close()
