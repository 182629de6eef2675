"""GPU suite (-m gpu): demodulated rounds must not depend on what device memory held before.

The cases of test_gpu_demod.py's tests 1 to 3 (tests/demod_cases.py: every round case through both entries, and every A / D case)
run once more in ONE child process with RGK_POISON=1, where every fresh device allocation of
the library -- the per-slot divisor buffer and the second pixel-sum buffer of a demodulated round among them -- starts as 0xFF bytes:
a slot of hit[] the bounce-0 walk left unwritten, a divisor read before it was written or a pixel sum read on a pixel's first sample
pass would show as a NaN or as other bits.  The bar is equality of bits with this process's run on fresh memory, which
test_gpu_demod.py holds to the plain entry and to the restatement.  One child at a time; a child that times out or dies of a signal
ends the whole session (pytest.exit, return code 3), as in test_gpu_memstate.py: nothing else may start on a GPU that has just
faulted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import demod_cases as DC
import memstate_ref as M
from conftest import record_parity
from test_gpu_demod import rd, run_of  # noqa: F401  (the fixture, and the in-process baseline both files share)

pytestmark = pytest.mark.gpu

FATAL_STATUS = (134, 139, 124, 137)   # abort, segmentation fault, a time limit's two ways out
CHILD_TIMEOUT = 240                   # seconds
CASES = DC.MEMSTATE_ROUND_CASES + list(DC.SUM_CASES)
_CHILD = {}


def poisoned_child(tmp_path_factory):
    if not _CHILD:
        out = tmp_path_factory.mktemp("demod_memstate") / "cases.npz"
        env = dict(os.environ, RGK_POISON="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, os.path.abspath(DC.__file__), "--out", str(out)]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned child did not finish in {CHILD_TIMEOUT} s: nothing else may start on the GPU\n"
                        f"{(e.stderr or '')[-2000:] if isinstance(e.stderr, str) else ''}", returncode=3)
        if r.returncode < 0 or r.returncode in FATAL_STATUS:
            pytest.exit(f"the poisoned child ended with status {r.returncode}: nothing else may start on the GPU\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", returncode=3)
        assert r.returncode == 0 and "demod cases ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
        with np.load(str(out)) as z:
            _CHILD.update(DC.unflatten(z))
    return _CHILD


def test_poisoned_allocations_change_no_bit(rd, tmp_path_factory):  # noqa: F811
    assert DC.MEMSTATE_ROUND_CASES == list(DC.ROUND_CASES) and "RGK_POISON" not in os.environ
    got = poisoned_child(tmp_path_factory)
    assert sorted(got) == sorted(CASES), "a case was left out"
    assert M.poisoned() == 0, "rgk_debug_poisoned_bytes() must stay 0 without RGK_POISON"
    bad, words = [], 0
    for name in CASES:
        base = run_of(rd, name)
        keys = sorted(k for k in base if not k.startswith("_"))
        assert keys == sorted(k for k in got[name] if not k.startswith("_")), name
        for k in keys:
            a, b = base[k], got[name][k]
            assert a.shape == b.shape and a.dtype == b.dtype, (name, k)
            d = int((M.bits(a) != M.bits(b)).sum())
            words += M.bits(a).size
            new_nan = int((np.isnan(b) & ~np.isnan(a)).sum()) if a.dtype.kind == "f" else 0
            if d or new_nan:
                bad.append((name, k, d, new_nan))
    totals = [int(got[name]["_poisoned_total"][0]) for name in CASES]
    record_parity("gpu_demod_memstate", cases=len(CASES), words=words, differing=sum(b[2] for b in bad), poisoned_bytes=totals[-1])
    assert not bad, bad[:10]
    assert totals[0] > 0 and totals == sorted(totals), "every case's allocations are counted"


def test_the_new_buffers_are_counted(rd, tmp_path_factory):  # noqa: F811
    """rgk_debug_poisoned_bytes() across the round call itself, on fresh scenes of one configuration: the demodulated entry's rise
    exceeds the plain entry's by exactly the two new buffers -- 32 B per pixel of the round and 16 B per path of the batch, which on a
    fresh scene is the paths of one pass: min(P, B) pixels x the plan's samples per pass (rgk_plan.h rgk_plan_passes; B: the
    case's batch_paths, else more than the frame).  Without the switch both rises are 0."""
    got = poisoned_child(tmp_path_factory)
    bad = []
    for name in DC.MEMSTATE_ROUND_CASES:
        case, base = DC.ROUND_CASES[name], run_of(rd, name)
        assert int(base["_plain.poisoned_by_round"][0]) == 0 and int(base["_demod.poisoned_by_round"][0]) == 0
        plain, demod = int(got[name]["_plain.poisoned_by_round"][0]), int(got[name]["_demod.poisoned_by_round"][0])
        P = case.size[0] * case.size[1]
        B = case.tuning.get("batch_paths", P * case.spp)
        npix = min(P, B)
        ns_max = max(1, min(case.spp, B // npix))
        n_sample_passes = -(-case.spp // ns_max)
        batch = npix * -(-case.spp // n_sample_passes)
        assert -(-P // npix) * n_sample_passes == case.passes, name
        extra, want = demod - plain, 32 * P + 16 * batch
        if plain <= 0 or extra != want:
            bad.append((name, plain, demod, extra, want))
    record_parity("gpu_demod_memstate.new_buffers", cases=len(DC.MEMSTATE_ROUND_CASES), bad=len(bad))
    assert not bad, bad
