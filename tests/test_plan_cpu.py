"""The launch-plan unit (rgk_amd/csrc/rgk_plan.h) on the CPU, under ASan + UBSan: tests/cpp/plan_main.cpp includes that one
header and nothing else of the library, and checks per case, against values written out from the formulas the launch wrappers
and the host carried before and from the pass plans tests/test_gpu_invariance.py names

  grids    the persistent walkers' grids (8 / 16 / 32 LDS entries: 2048 / 2048 / 1280), bounded grids (0 items -> 1, no 32-bit
           overflow), the shade pair at bounce 0 (blocks of 512: 1024 and 512) and later (256: 2048 and 1024), the light
           sub-path's launches, the connections, the bundle walker's bound;
  resolve  the per-pixel resolve (at most 4096 blocks) and the tiled one (pixels per tile, LDS bytes, at most 16384 tiles);
  walker   the <STACK, LDSN> variant of a stack configuration, and the whole truth table of the bundle walk;
  passes   the pass plans of Cornell 512 x 512 x 16 and 256 x 256 x 32 at the invariance tests' batch sizes, gshift, and the
           pixel groups of a pass.

A wrong grid bound never changes an image (every consumer is persistent or grid-stride), so no image test can see one: this
one does.  Exit status 0 = every condition held and neither sanitizer spoke.  That the harness links at all, without the HIP
runtime, is the check that the unit calls nothing of it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

CASES = ["grids", "resolve", "walker", "passes"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "plan_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("case", CASES)
def test_plan_unit_on_the_cpu(harness, case):
    # the switches of the environment must not reach the harness
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([harness, case], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
