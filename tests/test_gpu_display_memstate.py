"""GPU suite (-m gpu): the display stage must not depend on what device memory held before.

Every bit case of test_gpu_display.py (tests/display_cases.py: all images, with and without counts, both exposure modes, the three
operators, the threshold pixels) runs once more in ONE child process with RGK_POISON=1, where every fresh device allocation of the
library -- the histogram buffer and the transfer table among them -- starts as 0xFF bytes: a histogram that was not cleared on the
stream before the launch that adds to it would count from 0xFFFFFFFF, and a table read before its upload would compare against
NaNs.  The bar is equality of bits with this process's run on fresh memory, which test_gpu_display.py holds to the restatement.
One child; a child that times out or dies of a signal ends the whole session (pytest.exit, return code 3), as in
test_gpu_memstate.py: nothing else may start on a GPU that has just faulted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import display_cases as DC
import memstate_ref as M
from conftest import record_parity
from test_gpu_display import bit_runs, rd  # noqa: F401  (the fixtures: the in-process baseline both files share)

pytestmark = pytest.mark.gpu

FATAL_STATUS = (134, 139, 124, 137)   # abort, segmentation fault, a time limit's two ways out
CHILD_TIMEOUT = 240                   # seconds


def test_poisoned_allocations_change_no_bit_and_only_the_new_buffers_are_counted(bit_runs, tmp_path):  # noqa: F811
    _, results, thresholds, _, _ = bit_runs
    assert "RGK_POISON" not in os.environ and M.poisoned() == 0, "rgk_debug_poisoned_bytes() must stay 0 without RGK_POISON"
    out = tmp_path / "cases.npz"
    env = dict(os.environ, RGK_POISON="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.abspath(DC.__file__), "--out", str(out)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit(f"the poisoned display child did not finish in {CHILD_TIMEOUT} s: nothing else may start on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode in FATAL_STATUS:
        pytest.exit(f"the poisoned display child ended with status {r.returncode}: nothing else may start on the GPU\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", returncode=3)
    assert r.returncode == 0 and "display cases ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    want = {f"{name}##{key}": a for name, res in results.items() for key, a in res.items()}
    want.update({f"thresholds##{key}": a for key, a in thresholds.items()})
    words, bad = 0, []
    with np.load(str(out)) as z:
        assert sorted(k for k in z.files if not k.startswith("_")) == sorted(want), "a case was left out"
        for key, a in want.items():
            b = z[key]
            assert a.shape == b.shape and a.dtype == b.dtype, key
            d = int((M.bits(a) != M.bits(b)).sum())
            words += M.bits(a).size
            if d:
                bad.append((key, d))
        before, after = (int(v) for v in z["_poisoned"])
    record_parity("gpu_display_memstate", arrays=len(want), words=words, differing=sum(d for _, d in bad), poisoned_before=before, poisoned_by_display=after - before)
    assert not bad, bad[:10]
    # the scene's own allocations were poisoned before the first display call; all the display calls together add exactly the
    # histogram (256 bins + the dark count) and the table, each allocated once
    assert before > 0 and after - before == DC.NEW_BUFFER_BYTES == 2052
