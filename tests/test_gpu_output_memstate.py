"""GPU suite (-m gpu): the device output path must not depend on what device memory held before.

Every EXR and PNG case of test_gpu_output.py (tests/output_cases.py) runs once more in ONE child process with RGK_POISON=1, where
every fresh device allocation of the library -- the output byte buffer among them -- starts as 0xFF bytes: a byte of the file region
that no kernel wrote, a partial maximum read before it was stored, or a checksum piece left out would show in the file.  The bar is
equality of bytes with this process's run on fresh memory, which test_gpu_output.py holds to the host writers.  One child; a child
that times out or dies of a signal ends the whole session (pytest.exit, return code 3), as in test_gpu_memstate.py: nothing else
may start on a GPU that has just faulted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import memstate_ref as M
import output_cases as OC
from conftest import record_parity
from test_gpu_output import rd, runs  # noqa: F401  (the fixtures: the in-process baseline both files share)

pytestmark = pytest.mark.gpu

FATAL_STATUS = (134, 139, 124, 137)   # abort, segmentation fault, a time limit's two ways out
CHILD_TIMEOUT = 240                   # seconds


def test_poisoned_allocations_change_no_byte_and_only_the_output_buffer_is_counted(runs, tmp_path):  # noqa: F811
    got, _, _, exrs, pngs = runs
    assert "RGK_POISON" not in os.environ and M.poisoned() == 0, "rgk_debug_poisoned_bytes() must stay 0 without RGK_POISON"
    out = tmp_path / "cases.npz"
    env = dict(os.environ, RGK_POISON="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(OC.__file__), "--out", str(out)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30)
    except subprocess.TimeoutExpired:
        pytest.exit(f"the poisoned output child did not finish in {CHILD_TIMEOUT} s: nothing else may start on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode in FATAL_STATUS:
        pytest.exit(f"the poisoned output child ended with status {r.returncode}: nothing else may start on the GPU\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", returncode=3)
    assert r.returncode == 0 and "output cases ok" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    total, bad = 0, []
    with np.load(str(out)) as z:
        assert sorted(k for k in z.files if not k.startswith("_")) == sorted(got), "a case was left out"
        for key, a in got.items():
            b = z[key]
            total += a.size
            if a.shape != b.shape or a.dtype != b.dtype or int((M.bits(a) != M.bits(b)).sum()):
                bad.append(key)
        before, after = (int(v) for v in z["_poisoned"])
    record_parity("gpu_output_memstate", arrays=len(got), bytes=total, differing_arrays=len(bad), poisoned_before=before, poisoned_by_output=after - before)
    assert not bad, bad[:10]
    # the scene and its rounds were poisoned before the first output call; all the output calls together add the one device byte
    # buffer, once per time it had to grow
    assert before > 0 and after - before == OC.expected_growth(exrs, pngs)
