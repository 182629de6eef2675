"""The host runtime's GPU-free arithmetic (rgk_amd/csrc/rgk_round_plan.h) on the CPU, under ASan + UBSan:
tests/cpp/round_plan_main.cpp includes that header and nothing else of the library, and checks per case, against values written
out from the formulas the host file carried before

  workspace  bytes per path (180 unidirectional; the old literal at reverse 1, 3, 7) and every plane's elements per path;
  counters   a pass's counter blocks -> path rays, shadow rays and per-kernel units: depth 1 and 5, reverse 0 and 3, the first
             shadow launch with and without light-side entries, the light rays culled before the queue;
  fold       the kernel classes; launch times and traversal read-backs folded into the per-kernel records and the class sums;
  tiles      tile lists -> pixel-list offsets (no tiles, reversed ranges, a pixel outside the frame, 2^31 pixels), the centre-out
             task list, and what the key of a frame's cached lists depends on;
  stack      the traversal-stack configuration of shallow, deep and too-deep trees.

These numbers reach the benchmark's ray counts and the size of every pass, and until now only end-to-end GPU tests saw them.
Exit status 0 = every condition held and neither sanitizer spoke; that the harness links without the HIP runtime is the check
that the unit calls nothing of it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

CASES = ["workspace", "counters", "fold", "tiles", "stack"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("round_plan") / "round_plan_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "round_plan_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def run(harness, case):
    # the switches of the environment must not reach the harness
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    return subprocess.run([harness, case], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("case", CASES)
def test_round_plan_unit_on_the_cpu(harness, case):
    r = run(harness, case)
    assert r.returncode == 0, r.stderr + r.stdout


def test_task_list_is_the_oracles(harness):
    """67 x 45 in tiles of 32 (ragged right and bottom): the order and the seeds of the reference's GenerateTaskList, as the CPU
    oracle restates it."""
    from oracle import rgk_oracle as oracle
    r = run(harness, "print-tasks")
    assert r.returncode == 0, r.stderr + r.stdout
    got = [tuple(int(w) for w in line.split()) for line in r.stdout.splitlines()]
    want = [(t.x0, t.x1, t.y0, t.y1, t.seed) for t in oracle.generate_task_list(67, 45, seedstart=42, tile_size=32)]
    assert len(want) == 6 and got == want
