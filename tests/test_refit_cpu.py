"""CPU suite: the preconditions of tests/test_gpu_refit.py, asserted on the reference side alone.

A refit test passes vacuously when its move does not change what the refit has to rewrite: area orders that stay, normals whose
bits stay, a picture that stays.  Every condition here is computed from the cases of tests/refit_cases.py in numpy or by the
oracle; a move is adjusted until its condition holds, never the condition."""
import numpy as np
import pytest

import refit_cases as RC


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------- lights
def test_the_stretch_reorders_every_light_and_moves_the_powers():
    c = RC.lights_case()
    sb = c["make"]()
    before, total0 = RC.light_tables(sb, c["mesh"]["00"][0])
    after, total1 = RC.light_tables(sb, c["mesh"]["10"][0])
    assert len(before) >= 2 and sum(len(l["tris"]) >= 2 for l in before) >= 2          # more than one areal light with several triangles
    assert any(len(l["tris"]) >= 3 for l in before) and len(sb.pointlights) == 1 and sb.pointlights[0]["size"] > 0
    fan = next(l for l in before if len(l["tris"]) >= 3)
    a = np.sort(fan["area"])
    assert (a[1:] / a[:-1] > 1.2).all(), a                                              # clearly different areas
    for l0, l1 in zip(before, after):
        if len(l0["tris"]) >= 2:
            assert l0["order"] != l1["order"], (l0["order"], l1["order"])
        s0, s1 = l0["power"] / total0, l1["power"] / total1
        assert abs(s1 - s0) > 0.01 * s0, (s0, s1)
    assert abs(total1 - total0) > 0.1 * total0, (total0, total1)
    pp = RC.point_power(sb)
    assert pp > 0 and abs(pp / (pp + total1) - pp / (pp + total0)) > 0.01 * pp / (pp + total0)


def test_the_tilted_normals_change_every_emissive_vertex_a_normal():
    c = RC.lights_case()
    sb = c["make"]().finalize()
    N0, N1 = c["mesh"]["00"][1], c["mesh"]["11"][1]
    va = sb.F[np.array([t for l in sb.areal for t in l], np.int64), 0].astype(np.int64)
    assert (bits(N0[va]) != bits(N1[va])).any(axis=1).all()
    assert ((N0[va] * N1[va]).sum(axis=1) > 0.9).all()        # tilted, not turned over


def test_the_moved_lights_scene_is_another_picture(oracle):
    s0, s1 = RC.oracle_round("lights", "00"), RC.oracle_round("lights", "10")
    lit = (s0.main > 0).any(axis=2) | (s1.main > 0).any(axis=2)
    differ = (bits(s0.main) != bits(s1.main)).any(axis=2)
    assert lit.mean() > 0.5 and (differ & lit).sum() > 0.5 * lit.sum(), (int(lit.sum()), int((differ & lit).sum()))
    n0, n1 = RC.oracle_round("lights", "10"), RC.oracle_round("lights", "11")
    assert (bits(n0.main) != bits(n1.main)).any(axis=2).sum() > 0.25 * lit.sum()      # the vertex-A normals reach the picture


# ----------------------------------------------------------------------- shade
@pytest.mark.parametrize("point", [False, True], ids=["sphere-light-and-emitter", "point-light"])
def test_the_twist_turns_most_normals_and_tangents(point):
    c = RC.shade_case(point)
    (V0, N0, T0), (V1, N1, T1) = c["mesh"]["000"], c["mesh"]["111"]
    assert (bits(N0) != bits(N1)).any(axis=1).mean() > 0.5 and (bits(T0) != bits(T1)).any(axis=1).mean() > 0.5
    assert (bits(V0) != bits(V1)).any(axis=1).mean() > 0.9
    for a in (N1, T1):
        assert np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_moved_normals_and_tangents_reach_the_first_hit_normal_plane(oracle):
    n111, n100, n110 = (RC.oracle_planes(k)[1] for k in ("111", "100", "110"))
    tri = RC.oracle_planes("111")[3]
    assert np.array_equal(tri, RC.oracle_planes("100")[3]) and np.array_equal(tri, RC.oracle_planes("110")[3])   # same vertices, same hits
    hit = tri >= 0
    assert hit.mean() > 0.5
    by_both = (bits(n111) != bits(n100)).any(axis=2)
    assert (by_both & hit).sum() > 0.25 * hit.sum(), (int(by_both.sum()), int(hit.sum()))
    by_tangent = (bits(n111) != bits(n110)).any(axis=2)
    bumped = RC.bump_mapped_pixels("111")
    assert by_tangent.any() and not (by_tangent & ~bumped).any(), (int(by_tangent.sum()), int((by_tangent & ~bumped).sum()))
    # (of the bump-mapped surfaces the floor alone has tangents that a turn about the vertical axis changes: the back wall's are vertical)
    assert (by_tangent & bumped).sum() > 0.1 * bumped.sum()


def test_the_moved_shade_scene_is_another_picture(oracle):
    for point in (False, True):
        s0, s1 = RC.oracle_round("shade", "000", point=point), RC.oracle_round("shade", "111", point=point)
        assert s0.n_splats == s1.n_splats == 0
        assert (bits(s0.main) != bits(s1.main)).any(axis=2).mean() > 0.5


def test_the_cache_camera_sees_what_its_pixel_groups_did_not_see_before(oracle):
    """Entry lists and their caps are made per group of 8 consecutive pixels from what the group's rays can hit and how far they
    hit.  Through cache_camera("low"), for more than a tenth of the groups every ray hit something before the move and after
    it some ray's first hit lies a quarter beyond the farthest of them, and for another tenth a fifth nearer than the nearest:
    a list or a cap that survived the refit does not hold there.  Through the frame's own camera no group is like either, so
    the frame-cache test does not use it.  (Measured with a library whose refit keeps the lists: through the frame's camera
    and nine others the rounds after the refit were a fresh scene's all the same; through "low" on the device builder's tree 6
    pixels differed, through "narrow" -- which this count does not explain -- 20 on the host builder's:
    profiles/refit_coverage.txt.)"""
    def groups(camera):
        d0, d1 = RC.first_hit_depths("000", camera), RC.first_hit_depths("111", camera)
        beyond = nearer = total = 0
        for x in range(0, RC.W, 8):
            a, b = d0[:, x:x + 8], d1[:, x:x + 8]
            total += RC.H
            ok = np.isfinite(a).all(axis=1)
            beyond += int((ok & (b.max(axis=1) > 1.25 * a.max(axis=1))).sum())
            nearer += int((ok & (b.min(axis=1) < 0.8 * a.min(axis=1))).sum())
        return beyond, nearer, total
    beyond, nearer, total = groups(RC.cache_camera("low"))
    assert beyond > 0.1 * total and nearer > 0.1 * total, (beyond, nearer, total)
    assert groups(RC.shade_case(point=True)["camera"])[:2] == (0, 0)
    for view in ("low", "narrow"):
        s0, s1 = (RC.oracle_round("shade", k, point=True, cache_cam=view) for k in ("000", "111"))
        assert (bits(s0.main) != bits(s1.main)).any(axis=2).mean() > 0.5


# ----------------------------------------------------------------------- geometry
@pytest.mark.parametrize("name", list(RC.GEOMETRY))
def test_geometry_moves_are_accepted_and_their_rays_hit(oracle, name):
    scene, V0, V1 = RC.geometry_case(name)
    steps = RC.geometry_reference(name)
    assert [s[0] for s in steps] == ["moved", "back"] and (bits(V0) != bits(V1)).any()
    for step, V, osc, rays, ex, ig, ex2, a, b, vis in steps:
        eps = osc.info().epsilon
        assert osc.h and np.isfinite(eps) and eps > 0, (name, step, eps)
        assert (ex["tri"] >= 0).mean() > 0.25, (name, step, float((ex["tri"] >= 0).mean()))
        assert len(rays) <= 20000 and len(a) <= 20000 and (scene != "count257" or len(rays) <= 10000)
    e0, e1 = steps[1][2].info().epsilon, steps[0][2].info().epsilon
    if name == "count65-up-1e3":
        assert 500 < e1 / e0 < 2000
    if name == "count65-down-1e-3":
        assert 500 < e0 / e1 < 2000
    P0, P1 = V0.reshape(-1, 3, 3), V1.reshape(-1, 3, 3)
    if name == "flat-lifted":
        assert np.ptp(V0[:, 1]) == 0 and np.ptp(V1[:, 1]) > 1.0
    if name == "count65-flattened":
        assert np.ptp(V0[:, 1]) > 1.0 and np.ptp(V1[:, 1]) == 0
    if name == "duplicates-apart":
        assert (P0[30:39] == P0[30]).all() and len({P1[i].tobytes() for i in range(30, 39)}) == 9
    if name == "count64-collapsed":
        assert np.abs(P1.astype(np.float64).mean(axis=1)).max() < 1e-6 and np.abs(P0.mean(axis=1)).max() > 1
    if name == "count257-scrambled":   # no coherence: the triangles are as large as the scene
        assert np.median(np.ptp(P1, axis=1).max(axis=1)) > 0.3 * np.ptp(V0, axis=0).max()
    if name == "count65-degenerate":
        step, V, osc, rays, ex, ig, ex2, a, b, vis = steps[0]
        aimed = rays[-len(RC.COLLAPSED):]
        for t, r in zip(RC.COLLAPSED, aimed):
            v = P1[t, 0] - r[:3]
            assert np.allclose(v / np.linalg.norm(v), r[3:6], atol=1e-6)
            assert (P1[t, 2] == P1[t, 1]).all() or np.array_equal(P1[t, 2] - P1[t, 1], P1[t, 1] - P1[t, 0])
        for h in (ex, ex2):
            assert not np.isin(h["tri"], RC.COLLAPSED).any()
        back = steps[1]
        assert np.isin(back[4]["tri"], RC.COLLAPSED).any()       # ... and they are answers again after the move back
