"""GPU suite (-m gpu): results must not depend on what device memory held before.

Every other parity test runs the library in a young process on buffers hipMalloc has just handed out, and fresh pages are zero in
practice: a kernel that reads a queue slot, counter, cap, stack entry or scratch word before anything wrote it reads 0 there and
passes.  Here every entry of the library (the named cases of tests/memstate_ref.py) runs twice:

  baseline   in this process, RGK_POISON unset (asserted), on fresh scene handles; rgk_debug_poisoned_bytes() stays 0;
  poisoned   in a child process with RGK_POISON=1, one child per family and never two at a time: every fresh device allocation of
             the library -- the scene's buffers and the device builder's and refit's scratch, hipcub's storage included -- starts
             as 0xFF bytes (NaN as float, out of range as index), and so do the caller's output planes of the _device entries.

The bar is equality of bits, no tolerance: every array of every unidirectional case np.array_equal on its uint32 words between
the two runs, and no NaN the baseline does not hold.  "Equal to each other" must not mean "equally wrong": every unidirectional
round is also held once to the oracle's round with every ray answered by exhaustive search, bit for bit; builder and refit cases
to the exhaustive reference for every ray; bidirectional rounds, whose splat order is not repeatable, in both runs to the
oracle's terms with the bars of test_gpu_bdpt.check_case at cap = 0 (tests/bdpt_ref.py).  The stale pair -- two small frames on
a handle that has rendered a larger, different one, against the same two on a fresh handle -- is compared inside each run.

A child that times out or dies of a signal ends the whole session (pytest.exit, return code 3): nothing else may start on a GPU
that has just faulted.  Also here: the frame accumulator's entries (rgk_accum_upload / _add / _set_tag), the other place where the
library hands back memory it allocated itself."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from rgk_amd import capi

import bdpt_ref as B
import memstate_ref as M
from conftest import record_parity

pytestmark = pytest.mark.gpu

FATAL_STATUS = (134, 139, 124, 137)   # abort, segmentation fault, a time limit's two ways out
CHILD_TIMEOUT = 300                   # seconds: what test_with_poisoned_allocations_every_output_element_is_written gives its child


@pytest.fixture(scope="module")
def rd(product_lib):
    from rgk_amd import render_driver
    assert product_lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    return render_driver


# ----------------------------------------------------------------------- the two runs
_BASELINE, _CHILD = {}, {}


def baseline(rd, family):
    """The family's cases in this process, once, on fresh handles, without the switch; never changed afterwards."""
    if family not in _BASELINE:
        assert "RGK_POISON" not in os.environ, "the baseline must run without RGK_POISON"
        res = M.run_cases(rd, M.FAMILIES[family])
        assert M.poisoned() == 0, "rgk_debug_poisoned_bytes() must stay 0 without RGK_POISON"
        for arrays in res.values():
            for a in arrays.values():
                a.setflags(write=False)
        _BASELINE[family] = res
    return _BASELINE[family]


def poisoned_child(family, tmp_path_factory):
    """The family's cases in a child with RGK_POISON=1, once: {case: {key: array}}.  One child at a time (subprocess.run waits)."""
    if family not in _CHILD:
        out = tmp_path_factory.mktemp("memstate") / f"{family}.npz"
        env = dict(os.environ, RGK_POISON="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, os.path.abspath(M.__file__), "--family", family, "--out", str(out)]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned child of family `{family}` did not finish in {CHILD_TIMEOUT} s: nothing else may start on the GPU\n"
                        f"{(e.stderr or '')[-2000:] if isinstance(e.stderr, str) else ''}", returncode=3)
        if r.returncode < 0 or r.returncode in FATAL_STATUS:
            pytest.exit(f"the poisoned child of family `{family}` ended with status {r.returncode}: nothing else may start on the GPU\n"
                        f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}", returncode=3)
        assert r.returncode == 0 and "memstate ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
        with np.load(str(out)) as z:
            _CHILD[family] = M.unflatten(z)
        for name in M.FAMILIES[family]:
            assert int(_CHILD[family][name]["_poisoned_total"][0]) > 0, (name, "the child poisoned nothing")
    return _CHILD[family]


def outputs(arrays):
    return sorted(k for k in arrays if not k.startswith("_"))


def compare_bits(tag, base, got, poisoned_total):
    """Records arrays, words compared, differing and the poisoned byte total; returns (differing, NaNs the baseline does not hold)."""
    assert outputs(base) == outputs(got), (tag, outputs(base), outputs(got))
    words = differing = new_nan = 0
    worst = None
    for k in outputs(base):
        a, b = base[k], got[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape, a.dtype, b.dtype)
        d = int((M.bits(a) != M.bits(b)).sum())
        words += M.bits(a).size
        differing += d
        if d and worst is None:
            worst = (k, d)
        if a.dtype.kind == "f":
            new_nan += int((np.isnan(b) & ~np.isnan(a)).sum())
    record_parity(f"gpu_memstate[{tag}]", arrays=len(outputs(base)), words=words, differing=differing, new_nans=new_nan, poisoned_bytes=int(poisoned_total))
    return differing, new_nan, worst


def assert_family_equal(rd, family, tmp_path_factory, names=None):
    base, got = baseline(rd, family), poisoned_child(family, tmp_path_factory)
    assert sorted(got) == sorted(base) == sorted(M.FAMILIES[family]), "a case was left out"
    bad = []
    for name in names or M.FAMILIES[family]:
        total = int(got[name]["_poisoned_total"][0])
        differing, new_nan, worst = compare_bits(name, base[name], got[name], total)
        if differing or new_nan or total <= 0:
            bad.append((name, differing, new_nan, worst, total))
    assert not bad, bad
    return base, got


# ----------------------------------------------------------------------- poisoned against fresh, bit for bit
@pytest.mark.parametrize("family", ["unit", "rounds", "post"])
def test_poisoned_allocations_change_no_bit(rd, tmp_path_factory, family):
    """unit: rgk_trace_closest (n = 1, 65, 4097; plain, with `ignore`, counting), rgk_trace_visibility, rgk_bxdf_value / _sample on
    both routes, rgk_texture_sample, rgk_sampler_eval, rgk_libm_eval (n = 193).  rounds: the small scene under all 16 combinations
    of const_light x last_vertex x beam x entry_points (two rounds of a frame each: the second on capped entry lists), with two
    sample passes, at 5 x 3 x 1 spp depth 1 (queues shorter than a workgroup), the material zoo through a lens at depth 8 without
    roulette, the deep tree on the overflow area, a scene padded past both LDS thresholds, sphere light, emissive quad, float
    environment map, and the point-light scene on a handle refitted with moved vertices, normals and tangents (k_refit_shade) under
    both builders.  post: rgk_render_aov over every other tile (pixels outside keep the sentinel), rgk_render_aov_chain with 8
    hops, both denoisers, the noise estimate at tile size 5 with and without the variance plane, the round fold -- the output
    planes of the _device entries start as 0xFF bytes and no written element may still hold them (asserted where they are made)."""
    assert_family_equal(rd, family, tmp_path_factory)


def test_stale_buffers_change_no_bit(rd, tmp_path_factory):
    """DevBuf::alloc keeps a buffer when the new request is not larger.  On one handle of the small scene a 100 x 70 x 16 spp
    depth 8 reverse 3 round, an 8-hop feature chain and a 4097-ray probe, then the 33 x 31 x 5 spp depth 3 round and the 5 x 3
    round: those two equal the same two on a fresh handle -- in this process, in the poisoned child, and across the two."""
    base, got = assert_family_equal(rd, "stale", tmp_path_factory)
    for run, res in (("fresh memory", base), ("poisoned", got)):
        differing, new_nan, _ = compare_bits(f"stale against a fresh handle, {run}", res["stale.fresh-handle"], res["stale.after-a-larger-frame"],
                                             res["stale.after-a-larger-frame"].get("_poisoned_total", [0])[0])
        assert differing == 0 and new_nan == 0, run
    k = base["stale.fresh-handle"]["33x31.counters"]
    assert (base["stale.fresh-handle"]["33x31.count"] == 5).all() and k[1] > 33 * 31 * 5 and k[2] > 100 and float(base["stale.fresh-handle"]["33x31.accum"].max()) > 0


# ----------------------------------------------------------------------- the builder's scratch
def hits_of(arrays, prefix):
    n = len(arrays[f"{prefix}.tri"])
    h = np.zeros(n, dtype=[("t", "f4"), ("tri", "i4"), ("a", "f4"), ("b", "f4"), ("c", "f4")])
    for f in ("t", "tri", "a", "b", "c"):
        h[f] = arrays[f"{prefix}.{f}"]
    return h


def test_device_builder_and_refit_on_poisoned_scratch(rd, tmp_path_factory):
    """count257, duplicates and deep under device, device-karras and device-karras-rotate4; closed and count257 through the
    moved / back refit under host-sah and device, and the shade and lights cases of refit_cases.py through theirs with normals
    and tangents.  In both runs: n_nodes, max_depth and n_leaf_refs are the baseline's, and closest
    hits (plain and with the first hit ignored) and visibility bytes equal the exhaustive reference for EVERY ray -- node numbers
    come from atomics, so two builds may differ in their nodes' order, never in an answer.  In the poisoned run the byte total
    rises across rgk_scene_create by at least the builder's scratch arrays, n references x their summed element sizes, and across
    rgk_scene_refit by at least the refit's.  The refit's figure is the tight one: the second refit of a handle allocates no
    DevBuf at all, so every byte of its rise went through Tmp::alloc, the allocator both functions of rgk_build.hip share
    (measured: exactly refs x 24 + nodes x 36); the create's rise also holds the scene's own buffers and hipcub's storage."""
    base, got = baseline(rd, "builder"), poisoned_child("builder", tmp_path_factory)
    assert sorted(got) == sorted(base) == sorted(M.FAMILIES["builder"]), "a case was left out"
    bad = []
    for name in M.FAMILIES["builder"]:
        kind, rest = name.split(".", 1)
        rays = words = differing = 0
        for run, res in (("fresh", base[name]), ("poisoned", got[name])):
            assert np.array_equal(res["info"], base[name]["info"]), (name, run, res["info"], base[name]["info"])
            words += res["info"].size
            if kind == "builder":
                scene = rest.split("-", 1)[0]
                ref = M.exhaustive_ref(scene)
                checks = [(hits_of(res, "closest"), ref["ex"]), (hits_of(res, "ignore-first"), ref["ex2"])]
                vis = [(res["visible"], ref["vis"])]
            else:
                scene = rest.split("-", 1)[0]
                _, steps = M.refit_setup(scene)
                checks = [(hits_of(res, f"{step}.closest"), osc.trace_closest_exhaustive(rays_)) for step, V, osc, rays_, a, b in steps]
                vis = [(res[f"{step}.visible"], osc.visibility_exhaustive(a, b)) for step, V, osc, rays_, a, b in steps]
            assert (checks[0][1]["tri"] >= 0).mean() > 0.25
            for h, want in checks:
                differing += int(M.T.differing(h, want).sum()); rays += len(h); words += 5 * len(h)
            for v, want in vis:
                differing += int((v != want).sum()); rays += len(v); words += len(v)
        n_nodes, _, n_refs = (int(x) for x in base[name]["info"])
        if kind == "builder":
            rose = int(got[name]["_poisoned_by_create"][0])
            need = n_refs * (M.BUILD_TMP_BYTES + (M.PLOC_TMP_BYTES if rest.endswith("-device") else 0))
            assert int(base[name]["_poisoned_by_create"][0]) == 0
        else:
            rose = int(got[name]["_poisoned_by_refit.back"][0])   # (the first refit also allocates the scene's vertex buffer)
            assert int(got[name]["_poisoned_by_refit.moved"][0]) >= rose and int(base[name]["_poisoned_by_refit.back"][0]) == 0
            need = n_refs * M.REFIT_REF_BYTES + n_nodes * M.REFIT_NODE_BYTES
        record_parity(f"gpu_memstate[{name}]", arrays=len(outputs(base[name])), words=words, rays=rays, differing=differing,
                      poisoned_bytes=int(got[name]["_poisoned_total"][0]), scratch_poisoned=rose, scratch_at_least=need)
        if differing or rose < need:
            bad.append((name, differing, rose, need))
    assert not bad, bad


# ----------------------------------------------------------------------- never "equally wrong": the oracle
@functools.lru_cache(maxsize=None)
def oracle_split(oracle_key):
    """The oracle's round of a RoundSpec with every ray answered by exhaustive search, once per scene."""
    from oracle import rgk_oracle as O
    spec = next(s for s in M.ROUNDS.values() if s.oracle_key == oracle_key)
    sb, cam = spec.make()
    return O.OracleScene(sb.to_desc()).render_round_split(cam, spec.prm, O.generate_task_list(spec.prm.xres, spec.prm.yres), exhaustive=True)


UNI_KEYS = sorted({s.oracle_key for n, s in M.ROUNDS.items() if n in M.FAMILIES["rounds"]})


@pytest.mark.parametrize("oracle_key", UNI_KEYS)
def test_unidirectional_baselines_equal_the_oracle(rd, oracle, oracle_key):
    """Every round of every unidirectional case, as rendered on fresh memory, against the oracle's render_round_split(reverse = 0,
    exhaustive = True) of its scene: every pixel exact (no splats: one possible sum), sample counts, paths and path_rays the
    oracle's, shadow_rays at most the oracle's (zero-radiance shadow rays are skipped on the device) -- the bars of
    test_gpu_thresholds.test_unidirectional_rounds_equal_the_unpadded_run.  The poisoned run equals this baseline bit for bit."""
    base = baseline(rd, "rounds")
    split = oracle_split(oracle_key)
    assert split.n_splats == 0
    bad = []
    for name in M.FAMILIES["rounds"]:
        spec = M.ROUNDS[name]
        if spec.oracle_key != oracle_key:
            continue
        for r in range(spec.rounds):
            a, c, k = base[name][f"round{r}.accum"], base[name][f"round{r}.count"], [int(x) for x in base[name][f"round{r}.counters"]]
            _, s = B.check_split(a, c, split)
            record_parity(f"gpu_memstate.oracle[{name} round {r}]", **B.record_fields(s), bit_identical=s["exact_n0"],
                          shadow_rays_gpu_over_oracle=k[2] / max(1, split.counters.shadow_rays))
            ok = (s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["share_n0"] == 1.0 and s["exact_n0"] == 1.0 and
                  (k[0], k[1]) == (split.counters.paths, split.counters.path_rays) and k[2] <= split.counters.shadow_rays)
            if not ok:
                bad.append((name, r, s, k, (split.counters.paths, split.counters.path_rays, split.counters.shadow_rays)))
    assert not bad, bad


@pytest.mark.parametrize("name", M.FAMILIES["bidirectional"])
def test_bidirectional_rounds_against_the_oracle_in_both_runs(rd, oracle, tmp_path_factory, name):
    """The small scene at reverse 3 and Cornell at reverse 7, depth 8, 64 x 64 x 4 spp.  The splat order is not repeatable, so the
    two runs are not compared with each other: each is held to bdpt_ref.check_split against the oracle's exhaustive split with the
    bars of test_gpu_bdpt.check_case at cap = 0 -- no pixel outside the summation-order bound, the exact classes exact, sample
    counts, paths and path_rays the oracle's, shadow_rays at most the oracle's."""
    base, got = baseline(rd, "bidirectional"), poisoned_child("bidirectional", tmp_path_factory)
    assert sorted(got) == sorted(base) == sorted(M.FAMILIES["bidirectional"]), "a case was left out"
    split = oracle_split(M.ROUNDS[name].oracle_key)
    assert split.n_splats > 0
    bad = []
    for run, res in (("fresh", base[name]), ("poisoned", got[name])):
        a, c, k = res["round0.accum"], res["round0.count"], [int(x) for x in res["round0.counters"]]
        _, s = B.check_split(a, c, split)
        record_parity(f"gpu_memstate[{name} {run}]", arrays=len(outputs(res)), words=int(a.size + c.size + 3), differing=s["outside"], **B.record_fields(s),
                      path_rays_delta=k[1] - int(split.counters.path_rays), poisoned_bytes=int(res.get("_poisoned_total", [0])[0]))
        ok = (s["counts_equal"] and s["bad_values"] == 0 and s["outside"] == 0 and s["exact_n0"] == 1.0 and s["exact_n1"] == 1.0 and
              (k[0], k[1]) == (split.counters.paths, split.counters.path_rays) and k[2] <= split.counters.shadow_rays)
        if not ok:
            bad.append((run, s, k, (split.counters.paths, split.counters.path_rays, split.counters.shadow_rays)))
        assert np.array_equal(res["info"], base[name]["info"])
    assert not bad, bad


# ----------------------------------------------------------------------- the frame accumulator
def test_accumulator_upload_add_tag_round_trip(product_lib, tmp_path):
    """rgk_accum_upload / _download / _add / _set_tag / _save / _load on a ragged 37 x 29 accumulator: an upload comes back as it
    went up, `add` is the float32 / uint32 numpy sum bit for bit, a size mismatch is refused and leaves both operands as they were,
    and a checkpoint carries its tag: loaded under the same tag or under none, refused under another."""
    lib = product_lib
    assert lib.rgk_device_count() >= 1, "no HIP device: the product path has no fallback"
    Wa, Ha = 37, 29
    rng = np.random.default_rng(47)

    def planes(w=Wa, h=Ha):
        rgb = (rng.standard_normal((h, w, 3)) * 10.0 ** rng.uniform(-20, 20, (h, w, 3))).astype(np.float32)
        return rgb, rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)

    def make(w=Wa, h=Ha):
        a = C.c_void_p()
        capi.check(lib, lib.rgk_accum_create(w, h, 0, C.byref(a)))
        return a

    def down(a, w=Wa, h=Ha):
        rgb, cnt = np.full((h, w, 3), 7.5, np.float32), np.full((h, w), 7, np.uint32)
        capi.check(lib, lib.rgk_accum_download(a, rgb.ctypes.data, cnt.ctypes.data))
        return rgb, cnt

    def same(x, y):
        return np.array_equal(M.bits(x[0]), M.bits(y[0])) and np.array_equal(x[1], y[1])
    a, b, other = make(), make(), make(Wa + 1, Ha)
    try:
        zero = down(a)
        assert not zero[0].any() and not zero[1].any()                   # created clear
        pa, pb, po = planes(), planes(), planes(Wa + 1, Ha)
        for acc, p in ((a, pa), (b, pb), (other, po)):
            capi.check(lib, lib.rgk_accum_upload(acc, p[0].ctypes.data, p[1].ctypes.data))
        assert same(down(a), pa) and same(down(b), pb)                   # upload then download
        assert lib.rgk_accum_add(a, other) == -1 and lib.rgk_last_error() and lib.rgk_accum_add(other, a) == -1
        assert same(down(a), pa) and same(down(other, Wa + 1, Ha), po)   # refused: both operands unchanged
        capi.check(lib, lib.rgk_accum_add(a, b))
        want = ((pa[0] + pb[0]).astype(np.float32), pa[1] + pb[1])       # (uint32 addition wraps on both sides)
        got = down(a)
        differing = int((M.bits(got[0]) != M.bits(want[0])).sum() + (got[1] != want[1]).sum())
        record_parity("gpu_memstate[accumulator add 37x29]", arrays=2, words=int(want[0].size + want[1].size), differing=differing)
        assert differing == 0 and same(down(b), pb)
        # the tag travels with a checkpoint
        path = str(tmp_path / "acc.ckpt").encode()
        capi.check(lib, lib.rgk_accum_set_tag(a, 0x1122334455667788))
        capi.check(lib, lib.rgk_accum_save(a, path, 3, 18))
        r, s = C.c_uint32(0), C.c_uint32(0)
        capi.check(lib, lib.rgk_accum_set_tag(b, 0x1122334455667788))
        capi.check(lib, lib.rgk_accum_load(b, path, C.byref(r), C.byref(s)))
        assert (r.value, s.value) == (3, 18) and same(down(b), want)
        capi.check(lib, lib.rgk_accum_upload(b, pb[0].ctypes.data, pb[1].ctypes.data))
        capi.check(lib, lib.rgk_accum_set_tag(b, 0x1122334455667789))    # one bit off, in the low word
        assert lib.rgk_accum_load(b, path, C.byref(r), C.byref(s)) == -1 and b"different scene" in lib.rgk_last_error()
        capi.check(lib, lib.rgk_accum_set_tag(b, 0x0122334455667788))    # ... and in the high word
        assert lib.rgk_accum_load(b, path, C.byref(r), C.byref(s)) == -1
        assert same(down(b), pb)                                         # a refused load leaves the accumulator alone
        capi.check(lib, lib.rgk_accum_set_tag(b, 0))                     # untagged: not compared
        capi.check(lib, lib.rgk_accum_load(b, path, C.byref(r), C.byref(s)))
        assert same(down(b), want)
        assert lib.rgk_accum_load(other, path, C.byref(r), C.byref(s)) == -1   # another size
    finally:
        for acc in (a, b, other):
            lib.rgk_accum_destroy(acc)
