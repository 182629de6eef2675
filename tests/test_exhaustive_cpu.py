"""CPU suite: the exhaustive-search traversal reference (oracle/rgk_cpu.cpp Scene::FindExhaustive) -- no GPU needed.

The reference tests every triangle with Scene::TestIntersection under the walkers' stated rule (rgk_amd/csrc/rgk_trace.h): the
nearest accepted hit with t in [t0 - eps, t1 + eps], [t0, t1] = the ray's [near, far] clipped to the epsilon-padded scene box,
exact ties to the higher triangle id, `ignore` skipped; visibility = no accepted hit of Ray(a, b, 20 eps).  Here: hand-made
cases whose answers are known without running anything, and the first measurement of how far the kd-tree oracle -- the
yardstick of every other traversal test -- strays from that rule (DESIGN.md 4 quotes the numbers).
"""
import os

import numpy as np
import pytest

from conftest import ROOT, make_rays, record_parity
import trace_ref as T

F = np.float32
FAR_TRI = [[3, 0, -2], [4, 0, -2], [3, 1, -2]]     # gives the scene box a volume; no ray below goes near it
UNIT_TRI = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]       # plane z = 0, normal (0, 0, -1); corner weights a, b, c in this order
DOWN = (0, 0, -1)


def scene(oracle, tris):
    sb = T.builder_of(np.array(tris, F))        # (alive until the oracle has copied the arrays its descriptor points into)
    return oracle.OracleScene(sb.to_desc())


def one(o, origin, direction, near=0.0, far=10000.0, ignore=None):
    rays = make_rays(np.array([origin], F), np.array([direction], F), near, far)
    h = o.trace_closest_exhaustive(rays, None if ignore is None else np.array([ignore], np.int32))[0]
    k = o.trace_closest(rays, None if ignore is None else np.array([ignore], np.int32))[0][0]
    return h, k


def assert_miss(h):
    assert h["tri"] == -1 and h["t"] == np.inf and (h["a"], h["b"], h["c"]) == (0, 0, 0)


def test_one_triangle_interior_vertex_edge(oracle):
    o = scene(oracle, [UNIT_TRI, FAR_TRI])
    for origin, abc in (((0.25, 0.25, 1), (0.5, 0.25, 0.25)),     # interior
                        ((0, 0, 1), (1, 0, 0)), ((1, 0, 1), (0, 1, 0)), ((0, 1, 1), (0, 0, 1)),   # exactly through each corner
                        ((0.5, 0, 1), (0.5, 0.5, 0)), ((0, 0.5, 1), (0.5, 0, 0.5)), ((0.5, 0.5, 1), (0, 0.5, 0.5))):   # edge midpoints
        h, k = one(o, origin, DOWN)
        assert h["tri"] == 0 and h["t"] == 1.0 and (h["a"], h["b"], h["c"]) == abc, (origin, h)
        assert k == h, (origin, k)                      # one triangle in reach: the kd walk has nothing else to choose
    for origin in ((0.5 + 2.0 ** -20, 0.5, 1), (-2.0 ** -20, 0.5, 1), (0.5, -2.0 ** -20, 1)):      # a hair outside each edge
        assert_miss(one(o, origin, DOWN)[0])
    h, _ = one(o, (0.25, 0.25, -1), (0, 0, 1))           # from behind: no culling
    assert h["tri"] == 0 and h["t"] == 1.0


def test_rays_parallel_to_the_plane_miss(oracle):
    o = scene(oracle, [UNIT_TRI, FAR_TRI])
    eps = float(o.info().epsilon)
    assert_miss(one(o, (-1, 0.25, 0), (1, 0, 0))[0])     # in the plane: dot = 0
    # |dot(d, n)| = 0.5 eps < eps: rejected although the ray does cross the triangle; 2 eps: found
    d = np.array([1, 0, -0.5 * eps]); d /= np.linalg.norm(d)
    assert_miss(one(o, (-0.75, 0.25, 0.5 * eps), d)[0])
    d = np.array([1, 0, -2 * eps]); d /= np.linalg.norm(d)
    h, _ = one(o, (-0.75, 0.25, 2 * eps), d)
    assert h["tri"] == 0 and abs(h["t"] - 1.0) < 1e-4 and abs(h["b"] - 0.25) < 1e-4 and abs(h["c"] - 0.25) < 1e-6


def test_near_far_windows_at_plus_minus_epsilon(oracle):
    """The hit at t = 1 is accepted iff near - eps <= 1 <= far + eps (the box clip leaves these windows alone: the ray is inside
    the padded box from 1 - eps to 3 + eps).  0.9 eps / 1.1 eps on either side: 0.1 eps is ~40 float steps at 1."""
    o = scene(oracle, [UNIT_TRI, FAR_TRI])
    eps = float(o.info().epsilon)
    assert 4e-5 < eps < 5e-5
    for near, far, hit in ((0.0, 1 - 0.9 * eps, True), (0.0, 1 - 1.1 * eps, False), (1 + 0.9 * eps, 10000.0, True), (1 + 1.1 * eps, 10000.0, False),
                           (1.0, 1.0, True), (0.0, 1e30, True), (2.0, 0.5, False), (1.0 + 0.5 * eps, 1.0 - 0.5 * eps, False)):   # the last two: near > far
        h, k = one(o, (0.25, 0.25, 1), DOWN, near, far)
        if hit:
            assert h["tri"] == 0 and h["t"] == 1.0, (near, far, h)
        else:
            assert_miss(h)
        assert k == h, (near, far, k)


def test_coincident_copies_go_to_the_higher_id_and_ignore_takes_it_out(oracle):
    o = scene(oracle, [UNIT_TRI, UNIT_TRI, FAR_TRI, UNIT_TRI])        # copies at 0, 1 and 3
    assert one(o, (0.25, 0.25, 1), DOWN)[0]["tri"] == 3
    assert one(o, (0.25, 0.25, 1), DOWN, ignore=3)[0]["tri"] == 1
    assert one(o, (0.25, 0.25, 1), DOWN, ignore=1)[0]["tri"] == 3
    assert one(o, (0.25, 0.25, 1), DOWN, ignore=0)[0]["tri"] == 3
    h = one(o, (0.25, 0.25, 1), DOWN, ignore=3)[0]
    assert h["t"] == 1.0 and (h["a"], h["b"], h["c"]) == (0.5, 0.25, 0.25)
    # a nearer surface beats a higher id
    o2 = scene(oracle, [[[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]], UNIT_TRI, FAR_TRI])
    assert one(o2, (0.25, 0.25, 1), DOWN)[0]["tri"] == 0 and one(o2, (0.25, 0.25, 1), DOWN, ignore=0)[0]["tri"] == 1


def test_degenerate_triangles_are_never_hit(oracle):
    two_equal = [[0, 0, 0.5], [1, 0, 0.5], [1, 0, 0.5]]
    collinear = [[0, 0, 0.25], [0.5, 0.5, 0.25], [1, 1, 0.25]]
    o = scene(oracle, [two_equal, collinear, UNIT_TRI, FAR_TRI])
    for origin in ((0.25, 0.25, 1), (0.5, 0, 1), (0.5, 0.5, 1), (1, 0, 1)):
        h, k = one(o, origin, DOWN)
        assert h["tri"] == 2 and h["t"] == 1.0 and k == h, (origin, h)
    o = scene(oracle, [two_equal, collinear, FAR_TRI])
    assert_miss(one(o, (0.5, 0.5, 1), DOWN)[0])


def test_visibility_known_answers(oracle):
    o = scene(oracle, [UNIT_TRI, FAR_TRI])
    eps = float(o.info().epsilon)
    a = np.array([[0.25, 0.25, 1]] * 5 + [[2, 2, 1]], F)
    b = np.array([[0.25, 0.25, -1], [0.25, 0.25, 0.5], [0.25, 0.25, -10 * eps], [0.25, 0.25, -30 * eps], [0.9, 0.9, -1], [2, 2, -1]], F)
    # behind the triangle; in front of it; behind it by less than the 20 eps the ray stops short; by more; past the hypotenuse; beside
    want = [0, 1, 1, 0, 1, 1]
    assert list(o.visibility_exhaustive(a, b)) == want
    assert list(o.visibility(a, b)[0]) == want


def test_exhaustive_is_deterministic_and_thread_split_independent(oracle):
    """The rays are split over worker threads: 0, 1, 255, 256, 257 and 4097 rays give the prefix of the answer for all 5000."""
    sb = T.SCENES["duplicates"]()
    o = oracle.OracleScene(sb.to_desc())
    rays = T.ray_mix(o, 5000, seed=3, targets=T.targets_of(sb))
    full = o.trace_closest_exhaustive(rays)
    for n in (0, 1, 255, 256, 257, 4097):
        assert np.array_equal(o.trace_closest_exhaustive(rays[:n]), full[:n]), n
    assert (full["tri"] >= 0).mean() > 0.3


def test_ties_in_coincident_runs_go_to_the_higher_id(oracle):
    """The reference's own answers on `duplicates` (what test_gpu_exhaustive holds the walkers to): rays aimed at a run of
    coincident copies name the run's last member, and with that one ignored the one before it, at the same t to the bit."""
    sb = T.SCENES["duplicates"]()
    o = oracle.OracleScene(sb.to_desc())
    rays = T.ray_mix(o, 20000, seed=5, targets=T.targets_of(sb))
    ex = o.trace_closest_exhaustive(rays)
    ex2 = o.trace_closest_exhaustive(rays, ex["tri"].astype(np.int32))
    runs = {t: first + run - 1 for first, run in ((10, 2), (20, 3), (30, 9)) for t in range(first, first + run)}
    in_run = np.isin(ex["tri"], list(runs))
    assert in_run.sum() > 100
    assert all(runs[t] == t for t in ex["tri"][in_run])                           # always the highest id of its run
    second = in_run & np.isin(ex2["tri"], list(runs))
    assert second.sum() > 100 and np.array_equal(T.bits(ex["t"][second]), T.bits(ex2["t"][second]))
    assert (ex2["tri"][second] == ex["tri"][second] - 1).all()


# ----------------------------------------------------------------------- the kd-tree oracle against the exhaustive one
def fixture_builder(name):
    from rgk_amd.workloads import SceneFixture, Workload
    if name == "cornell":
        return Workload("cornell-256", scale=0.25, spp=1).builder
    return SceneFixture(os.path.join(ROOT, "tests", "golden", "scene_%s.npz" % name)).builder


@pytest.mark.parametrize("name", ["cornell", "cube3", "box6", "rubiks-bump", "cornell-box-spheres"])
def test_kd_oracle_against_exhaustive(oracle, name):
    """20 000 random rays per shipped scene.  Invariants: t_exhaustive <= t_kd for every ray (the kd walk accepts a subset of the
    exhaustive window and stops at the first leaf with a hit), equal bits wherever both name the same triangle.  Where they name
    different ones: exact-t ties (coincident or coplanar surfaces, the kd leaf's list order against "higher id"), hits within
    2 eps (the kd walk's per-leaf windows), and beyond -- held to the bar the GPU suite uses for `unexplained`.
    Measured (seed 7): DESIGN.md 4."""
    sb = fixture_builder(name)
    o = oracle.OracleScene(sb.to_desc())
    i = o.info()
    lo, hi = T.box_of(i)
    oo, dd = T.random_rays(np.random.default_rng(7), lo, hi, 20000)
    rays = make_rays(oo, dd)
    kd, _ = o.trace_closest(rays)
    ex = o.trace_closest_exhaustive(rays)
    m = T.kd_vs_exhaustive(kd, ex, i.epsilon)
    n = len(rays)
    record_parity("test_kd_oracle_against_exhaustive:" + name, rays=n, hits=float((ex["tri"] >= 0).mean()), exact_tie_share=m["exact_ties"] / n,
                  within_2eps_share=m["within_2eps"] / n, beyond_share=m["beyond"] / n, beyond=m["beyond"])
    print(f"[kd vs exhaustive] {name}: {m}")
    assert m["beyond"] <= max(1, 5e-5 * n), m
    # the same with every first hit ignored: the second surfaces
    ig = ex["tri"].astype(np.int32)
    kd2, _ = o.trace_closest(rays, ig)
    ex2 = o.trace_closest_exhaustive(rays, ig)
    m2 = T.kd_vs_exhaustive(kd2, ex2, i.epsilon)
    hit = ex["tri"] >= 0
    assert (ex2["tri"][hit] != ex["tri"][hit]).all()
    record_parity("test_kd_oracle_against_exhaustive:" + name + ":ignore-first", rays=n, exact_tie_share=m2["exact_ties"] / n,
                  within_2eps_share=m2["within_2eps"] / n, beyond_share=m2["beyond"] / n, beyond=m2["beyond"])
    print(f"[kd vs exhaustive, first hit ignored] {name}: {m2}")
    assert m2["beyond"] <= max(1, 5e-5 * n), m2


@pytest.mark.parametrize("name", ["cornell", "cube3"])
def test_kd_visibility_against_exhaustive(oracle, name):
    """Scene::Visibility through the kd walk against the exhaustive window: the kd walk sees a subset of the accepted hits, so a
    pair it calls blocked is blocked; the share it calls visible and the exhaustive search does not goes on record."""
    sb = fixture_builder(name)
    o = oracle.OracleScene(sb.to_desc())
    a, b = T.visibility_pairs(o, 20000, seed=8)
    vk, _ = o.visibility(a, b)
    ve = o.visibility_exhaustive(a, b)
    assert not ((vk == 0) & (ve == 1)).any()
    differ = int((vk != ve).sum())
    record_parity("test_kd_visibility_against_exhaustive:" + name, pairs=len(a), visible=float(ve.mean()), differ=differ)
    assert differ <= max(1, 5e-5 * len(a)), differ
