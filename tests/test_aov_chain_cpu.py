"""Feature planes that follow mirrors and glass (rgk_render_aov_chain[_device]), the part that needs no GPU: known answers of the
reference composition (tests/chain_ref.py) on the hall, that every kind of ending is on screen in the scenes the GPU suite
compares, max_hops = 0 against the first-hit composition (tests/post_ref.py), the ABI and its mirror, and every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rgk_amd import capi

import chain_ref as CR
import post_ref as R
from conftest import ROOT

F = np.float32
ENTRIES = ["rgk_render_aov_chain_device", "rgk_render_aov_chain"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def hall(oracle):
    ch, desc, sb = CR.reference("hall")
    sb.epsilon = float(oracle.OracleScene(desc).info().epsilon)
    return ch, sb


def tri_normal(sb, tri):
    V = np.concatenate(sb.vertices).astype(np.float64)
    i = np.concatenate(sb.tri_idx)[tri]
    n = np.cross(V[i[1]] - V[i[0]], V[i[2]] - V[i[0]])
    return n / np.linalg.norm(n)


# ----------------------------------------------------------------------- known answers of the composition
def test_flat_mirror_reports_the_floor_behind_it(hall):
    """A flat mirror over a flat floor: the chain is as long as the straight ray to the floor (the floor is its own mirror image
    in a vertical plane), the triangle is a floor triangle, the albedo is mirror colour x checker texel, hops = 1."""
    ch, sb = hall
    alb, nrm, z, tri, hops, end = [a.reshape(-1, *a.shape[2:]) for a in CR.planes(ch, 4)]
    px = np.flatnonzero(np.isin(ch.tri[0], sb.parts["mirror"]) & np.isin(ch.tri[1], sb.parts["floor"]) & (ch.event[1] == CR.SURFACE))
    assert len(px) > 100
    assert (hops[px] == 1).all() and (end[px] == CR.SURFACE).all() and np.isin(tri[px], sb.parts["floor"]).all()
    o, d = ch.ray[0, px, :3].astype(np.float64), ch.ray[0, px, 3:].astype(np.float64)
    o1, d1 = ch.ray[1, px, :3].astype(np.float64), ch.ray[1, px, 3:].astype(np.float64)
    t1, t2 = (-3.0 - o[:, 2]) / d[:, 2], -o1[:, 1] / d1[:, 1]  # to the mirror's plane z = -3, from there to the floor's y = 0
    assert np.array_equal(bits(z[px]), bits(ch.depth[1, px])) and np.allclose(ch.depth[0, px], t1, rtol=1e-5) and np.allclose(z[px], t1 + t2, rtol=1e-5)
    assert np.allclose(z[px], -o[:, 1] / d[:, 1], rtol=2e-5)  # ... which is the straight ray's way to the floor
    assert np.allclose(d1, d * [1, 1, -1], atol=1e-6)
    assert np.allclose(nrm[px], [0, 1, 0], atol=1e-6)
    mc = F(CR.MIRROR_COLOR)
    seen = [np.isclose(alb[px], mc * F(c), rtol=1e-5, atol=0).all(axis=-1) for c in CR.CHECKER]
    assert min(s.sum() for s in seen) > 30 and (seen[0] | seen[1]).mean() > 0.6, [int(s.sum()) for s in seen]  # (the rest: blends at a field's edge)


def test_sky_through_the_mirror_is_a_miss_with_one_hop(hall):
    ch, sb = hall
    alb, nrm, z, tri, hops, end = [a.reshape(-1, *a.shape[2:]) for a in CR.planes(ch, 4)]
    px = np.flatnonzero(np.isin(ch.tri[0], sb.parts["mirror"]) & (ch.event[1] == CR.MISS))
    assert len(px) > 50
    assert (hops[px] == 1).all() and (tri[px] == -1).all() and (z[px] == 0).all() and (alb[px] == 0).all() and (nrm[px] == 0).all()
    # ... and with max_hops = 0 the same pixels report the mirror itself: albedo 1, the mirror's normal, its distance
    alb0, nrm0, z0, tri0, hops0, _ = [a.reshape(-1, *a.shape[2:]) for a in CR.planes(ch, 0)]
    assert np.isin(tri0[px], sb.parts["mirror"]).all() and (alb0[px] == 1).all() and np.allclose(nrm0[px], [0, 0, 1], atol=1e-6) and (hops0 == 0).all()


def test_slab_shifts_the_ray_sideways_and_keeps_its_direction(hall):
    """Through two parallel faces: hops = 2, the ray behind the slab is parallel to the ray in front of it and offset sideways by
    thickness * sin(ti - tt) / cos(tt) -- with the two steps of e = 10 epsilon along the normal that the continuation rays start
    with: (thickness - e) inside the glass, and 2 e sin(ti) from the steps themselves."""
    ch, sb = hall
    front, back = list(sb.parts["slab"])[0:2], list(sb.parts["slab"])[2:4]
    px = np.flatnonzero(np.isin(ch.tri[0], front) & np.isin(ch.tri[1], back) & (ch.event[1] == CR.CONTINUES) & np.isin(ch.tri[2], sb.parts["floor"]))
    assert len(px) > 100
    hops, end = CR.planes(ch, 4)[4].reshape(-1), CR.planes(ch, 4)[5].reshape(-1)
    assert (hops[px] == 2).all() and (end[px] == CR.SURFACE).all()
    d0, d2 = ch.ray[0, px, 3:].astype(np.float64), ch.ray[2, px, 3:].astype(np.float64)
    assert np.allclose(d0, d2, atol=2e-6)
    rel = ch.ray[2, px, :3].astype(np.float64) - ch.ray[0, px, :3].astype(np.float64)
    off = np.linalg.norm(rel - (rel * d0).sum(-1, keepdims=True) * d0, axis=-1)
    ti = np.arccos(np.abs(d0[:, 2]))
    tt = np.arcsin(np.sin(ti) / 1.5)
    e = 10 * sb.epsilon
    assert np.allclose(off, (CR.SLAB_THICKNESS - e) * np.sin(ti - tt) / np.cos(tt) + 2 * e * np.sin(ti), atol=2e-5) and off.max() > 0.01 and e < 0.01


def test_prism_reflects_totally_and_the_leak_rule_and_the_mix_end_the_chain(hall):
    ch, sb = hall
    # total internal reflection: inside the prism the sample is the reflection about the face's geometric normal
    k, p = [int(v[0]) for v in np.nonzero(ch.reflected & np.isin(ch.tri, sb.parts["prism"]))]
    assert k >= 1 and ch.kind[k, p] == capi.BXDF_DIELECTRIC and ch.kind[k - 1, p] == capi.BXDF_DIELECTRIC
    d, n = ch.ray[k, p, 3:].astype(np.float64), tri_normal(sb, ch.tri[k, p])
    assert np.allclose(ch.ray[k + 1, p, 3:], d - 2 * d.dot(n) * n, atol=1e-5)
    sin_i = np.sqrt(1 - d.dot(n) ** 2)
    assert sin_i * 1.5 > 1  # beyond the critical angle
    assert ch.reflected.sum() > 50
    # the leak rule: the reflection about the bump-tilted normal dips under the surface; the pixel ends ON the mirror
    alb, nrm, z, tri, hops, end = [a.reshape(-1, *a.shape[2:]) for a in CR.planes(ch, 8)]
    leak = np.flatnonzero(end == CR.LEAK)
    assert len(leak) > 20 and np.isin(tri[leak], sb.parts["bumpy"]).all()
    first = leak[hops[leak] == 0]
    later = leak[hops[leak] > 0]
    assert len(first) and len(later)
    assert (alb[first] == 1).all() and np.allclose(np.linalg.norm(nrm[leak].astype(np.float64), axis=-1), 1, atol=1e-5)
    assert np.array_equal(bits(z[first]), bits(ch.depth[0, first])) and (z[later] > ch.depth[0, later]).all()
    # the mix ends the chain at once with its mixed albedo
    mix = np.flatnonzero(ch.kind[0] == capi.BXDF_MIX)
    assert len(mix) > 50 and (hops[mix] == 0).all() and (end[mix] == CR.SURFACE).all() and np.isin(tri[mix], sb.parts["half"]).all()
    want = F(0.5) * np.ones(3, F) + (F(1) - F(0.5)) * F(CR.PAINT)
    assert (bits(alb[mix]) == bits(want)).all()
    # the transparent quad passes straight through, weight 1
    gh = np.flatnonzero(np.isin(ch.tri[0], sb.parts["ghost"]) & (ch.event[1] == CR.SURFACE))
    assert len(gh) and np.allclose(ch.ray[1, gh, 3:], ch.ray[0, gh, 3:], atol=1e-6) and np.isin(ch.kind[1, gh], [capi.BXDF_DIFFUSE]).all()


# ----------------------------------------------------------------------- what the GPU comparison covers
def endings(ch, max_hops):
    hops, end = CR.planes(ch, max_hops)[4].reshape(-1), CR.planes(ch, max_hops)[5].reshape(-1)
    return {(int(e), bool(h > 0)) for e, h in zip(end, hops)}, hops, end


def test_every_kind_of_ending_is_on_screen_in_the_hall(hall):
    ch, _ = hall
    for H in (1, 2, 4):
        got, hops, end = endings(ch, H)
        for e in (CR.MISS, CR.DROPPED, CR.SURFACE, CR.LEAK):
            assert (e, False) in got, (H, e)
        for e in (CR.MISS, CR.SURFACE, CR.CONTINUES) + ((CR.DROPPED,) if H >= 1 else ()) + ((CR.LEAK,) if H >= 2 else ()):
            assert (e, True) in got, (H, e)  # CONTINUES: a delta vertex made terminal by k == max_hops
        assert (hops[end == CR.CONTINUES] == H).all() and hops.max() == H
    got, hops, end = endings(ch, 0)
    assert (hops == 0).all() and (CR.CONTINUES, False) in got
    got, hops, end = endings(ch, 8)
    assert hops.max() >= 5 and (CR.CONTINUES, True) not in got  # every chain of the hall ends by itself within eight hops
    for k in (capi.BXDF_MIRROR, capi.BXDF_DIELECTRIC, capi.BXDF_TRANSPARENT, capi.BXDF_MIX, capi.BXDF_DIFFUSE):
        assert (ch.kind == k).any(), k


def test_the_endings_of_the_spheres_scene(oracle):
    """The committed Cornell box with spheres has no bump map and no broken normal, so no leak and no dropped vertex: it shows a
    miss, surfaces seen directly and through the glass sphere (two hops), total internal reflection, and one pixel whose ray stays
    inside the sphere -- terminal by k == max_hops at every max_hops."""
    ch, _, _ = CR.reference("spheres")
    got, hops, end = endings(ch, 4)
    assert {(CR.MISS, False), (CR.SURFACE, False), (CR.SURFACE, True), (CR.CONTINUES, True)} <= got
    assert (hops == 2).sum() > 100 and ch.reflected.any() and (ch.kind == capi.BXDF_LTC_BECKMANN).any()


# ----------------------------------------------------------------------- max_hops = 0 is the first-hit composition
def test_max_hops_0_equals_the_first_hit_composition(oracle):
    """On the Cornell frame and the tiles test_gpu_post.py compares (those without an exact tie: the first-hit composition asks the
    kd-tree, which has no rule for one) every plane is equal bit for bit; on that file's material zoo wherever both name the
    same triangle."""
    from test_gpu_post import feature_case
    for name in ("cornell", "zoo"):
        sb, cam, W, H, bump, _ = feature_case(name)
        desc = sb.to_desc()
        osc = oracle.OracleScene(desc)
        ra, rn, rz, rt = R.oracle_features(oracle, osc, desc, cam, W, H, bump)
        ca, cn, cz, ct, hops, _ = CR.planes(CR.chain(oracle, osc, desc, cam, W, H, bump, hops=0), 0)
        assert (hops == 0).all()
        inside = np.zeros((H, W), bool)
        if name == "cornell":
            ties = R.reference_exact_ties(oracle, osc, desc, cam, W, H)
            for t in oracle.generate_task_list(W, H):
                if not ties[t.y0:t.y1, t.x0:t.x1].any():
                    inside[t.y0:t.y1, t.x0:t.x1] = True
            assert 0 < inside.sum() < inside.size and np.array_equal(ct[inside], rt[inside])
        else:
            inside = ct == rt
            assert inside.mean() > 0.999
        for a, b in ((ca, ra), (cn, rn), (cz, rz)):
            assert np.array_equal(bits(a[inside]), bits(b[inside]))
        assert (ct[inside] >= 0).mean() > 0.5


# ----------------------------------------------------------------------- ABI
def test_header_mirror_and_library_agree_on_the_entries(product_lib):
    hdr = open(os.path.join(ROOT, "include", "rgk.h")).read()
    declared = set(re.findall(r"\b(rgk_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS)
    for name in ENTRIES:
        assert name in declared and getattr(product_lib, name) is not None
        proto = re.search(r"int " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto).split(",")]
        assert len(args) == len(getattr(product_lib, name).argtypes) == 11
        assert args[5] == "uint32_t max_hops" and getattr(product_lib, name).argtypes[5] is C.c_uint32
        assert args[10].startswith("uint8_t *")
    assert int(re.search(r"#define RGK_AOV_MAX_HOPS (\d+)", hdr).group(1)) == capi.AOV_MAX_HOPS == CR.MAX_HOPS == 8


def test_argument_errors_need_no_gpu(product_lib):
    """Reported before the scene or a device is touched: the `scene` below is 64 bytes of nothing."""
    lib, INVALID = product_lib, -1
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    cam, prm, tiles = capi.Camera(), capi.Params(), (capi.Tile * 1)()
    prm.xres, prm.yres = 8, 8
    tiles[0].x0, tiles[0].x1, tiles[0].y0, tiles[0].y1 = 0, 8, 0, 8
    p = np.zeros(8 * 8 * 3, np.float32).ctypes.data
    for fn in (lib.rgk_render_aov_chain_device, lib.rgk_render_aov_chain):
        assert fn(scene, C.byref(cam), C.byref(prm), tiles, 1, 9, p, p, p, p, p) == INVALID and b"max_hops" in lib.rgk_last_error()
        assert fn(scene, C.byref(cam), C.byref(prm), tiles, 1, 0xFFFFFFFF, None, None, None, None, None) == INVALID
        assert fn(None, C.byref(cam), C.byref(prm), tiles, 1, 4, p, p, p, p, p) == INVALID
        assert fn(scene, None, C.byref(prm), tiles, 1, 4, p, p, p, p, p) == INVALID and b"null" in lib.rgk_last_error()
        assert fn(scene, C.byref(cam), None, tiles, 1, 4, p, p, p, p, p) == INVALID
        assert fn(scene, C.byref(cam), C.byref(prm), None, 1, 4, p, p, p, p, p) == INVALID
        bad = capi.Params.from_buffer_copy(prm)
        bad.xres = 70000
        assert fn(scene, C.byref(cam), C.byref(bad), tiles, 1, 4, p, p, p, p, p) == INVALID
        tiles[0].x1 = 9
        assert fn(scene, C.byref(cam), C.byref(prm), tiles, 1, 8, p, p, p, p, p) == INVALID and b"outside the frame" in lib.rgk_last_error()
        tiles[0].x1 = 8
    n = C.c_uint32(0)
    assert lib.rgk_scene_get_post_timing(scene, 7, None, C.byref(n)) == INVALID
    assert lib.rgk_scene_get_post_timing(scene, 6, None, C.byref(n)) == INVALID and b"scene handle" in lib.rgk_last_error()


# ----------------------------------------------------------------------- driver and command line
def test_driver_and_cli_refusals(tmp_path, capsys):
    from rgk_amd import render_driver as rd
    from rgk_amd.__main__ import main

    class Cfg:
        xres, yres, render_rounds, render_minutes = 8, 8, 1, None
        get_params = staticmethod(lambda sampler=0, flags=0: capi.Params())
    with pytest.raises(ValueError, match="history"):
        rd.RenderDriver(None, Cfg, None, device="cpu", history=rd.TemporalHistory(), aov_hops=2)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="aov_hops"):
            rd.RenderDriver(None, Cfg, None, device="cpu", aov_hops=bad)
    cfg = str(tmp_path / "absent.json")  # refused before the file is looked at
    for args, word in ((["--aov-hops", "4"], "needs --aov or --denoise"), (["--aov-hops", "4", "--denoise", "--temporal"], "--temporal"),
                       (["--aov-hops", "9", "--aov"], "Invalid argument"), (["--aov-hops", "-1", "--denoise"], "Invalid argument"),
                       (["--aov-hops", "0", "--denoise", "--temporal"], "--temporal")):
        assert main([cfg] + args) == 1
        assert word in capsys.readouterr().out, args
    assert main([cfg, "--aov-hops", "4", "--aov", "-q"]) == 1 and "Failed to load config file" in capsys.readouterr().out  # accepted: it got as far as the file
