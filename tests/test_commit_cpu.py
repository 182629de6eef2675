"""The GPU-free half of scene commit (rgk_amd/csrc/rgk_commit.cpp) on the CPU, under ASan + UBSan: tests/cpp/commit_main.cpp
links that one translation unit and nothing else of the library, makes its inputs from a fixed seed, and checks per case

  geom-*    647 triangles (small ones, two that span the scene and are pre-split, five with a NaN plane, 40 coincident copies)
            under the default build options and with leaf size 1 / 16, pre-split off, reinsertion off; and a 3-triangle scene
            that is one leaf: the leaves cover every reference exactly once, the listed triangles are the finite-plane ones,
            every point of a 13-step barycentric lattice on every triangle is found through the DECODED 8-bit boxes alone
            (tolerance zero: the boxes are epsilon-padded and rounded outward), max_depth is the walk's, two runs are
            byte-identical;
  refit-pieces  the box rgk_scene_refit gives a pre-split reference (piece_box, rgk_tree.h -- the function the device kernel
            calls): every proper piece of that geometry under three affine moves of its triangle, a 13 x 13 lattice over its
            parameter box evaluated in double, every point inside the box with tolerance zero;
  textures  six textures in one descriptor: palette detection (+0.0, -0.0 and a NaN among the values), table sharing, the
            caller's table, the 257-value texture that stays float, tiled byte texels bit-equal to their sources;
  pool-*    assign_palettes + pack_texels on textures alone.  tables: three caller tables at offsets 0, 256, 512 in the order of
            their first appearance (the kernels decode a table through LDS while offset + 256 <= 512, by global loads beyond:
            tests/test_gpu_thresholds.py) and two few-valued float textures sharing one table at 768; limits: 256 distinct
            values become bytes + table, 257 stay float; bits: +0.0, -0.0, NaNs of different payloads and signs, infinities and
            denormals are different values, every texel decodes to its own bits; small: (height, width) 1 x 1, 1 x 5, 9 x 1,
            4 x 8, 5 x 9, 4 x 16, 3 x 7 as byte and as few-valued float textures -- texel (x, y) at tex_row(y) + tex_col(x)
            (rgk_device.h, restated in the harness), padding zero, every texture on the 32-dword boundary where the one
            before ended;
  small     commit_bounds, const_light_eligible, build_areal_tables.

Exit status 0 = every condition held and neither sanitizer spoke.  That the harness links at all, without the HIP runtime,
is the check that the unit calls nothing of it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "rgk_amd", "csrc")

CASES = ["geom-default", "geom-leaf1", "geom-leaf16", "geom-nosplit", "geom-noopt", "geom-single", "refit-pieces", "textures", "pool-tables", "pool-limits",
         "pool-bits", "pool-small", "small"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("commit") / "commit_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "commit_main.cpp"), os.path.join(CSRC, "rgk_commit.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("case", CASES)
def test_commit_unit_on_the_cpu(harness, case):
    # the build switches of the environment must not reach the harness: it sets its options itself
    env = {k: v for k, v in os.environ.items() if not k.startswith("RGK_")}
    r = subprocess.run([harness, case], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout

