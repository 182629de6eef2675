"""The record ring of k_last_vertex (rgk_amd/csrc/rgk_ring.h) on the CPU, under ASan + UBSan: tests/cpp/ring_main.cpp includes
that header and rgk_plan.h and nothing else of the library, and checks

  values     capacity, wrap, append and read positions, and how many records a take consumes, written out;
  workgroup  the kernel's loop over a ring of record numbers -- all sky, all live, the headline's 45 %, block - 1 per iteration,
             a queue below a workgroup: every record read once and in order, none overwritten unread, full takes inside the
             loop only, the final flush short of a workgroup, nothing left behind;
  plan       which bounce is a pass's last (rgk_last_bounce) and the launch's grids.

Exit status 0 = every condition held and neither sanitizer spoke."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

CASES = ["values", "workgroup", "plan"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ring") / "ring_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "ring_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("case", CASES)
def test_ring_unit_on_the_cpu(harness, case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([harness, case], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
