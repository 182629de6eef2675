"""Compile the HIP product library in-tree: rgk_amd/csrc/librgk_hip.so (gfx950).

Every source is compiled on its own (FLAGS + SOURCE_FLAGS[source] + extra), the objects are linked into the library."""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "librgk_hip.so")
SOURCES = ["rgk_kernels.hip", "rgk_shade_kernels.hip", "rgk_post.hip", "rgk_pack.hip", "rgk_build.hip", "rgk_scene.cpp", "rgk_round.cpp", "rgk_probe.cpp", "rgk_post_host.cpp", "rgk_commit.cpp", "rgk_output.cpp", "rgk_accum.cpp", "rgk_comm.cpp"]
HEADERS = ["rgk_kernels.h", "rgk_plan.h", "rgk_ring.h", "rgk_round_plan.h", "rgk_scene_impl.h", "rgk_adapt.h", "rgk_build.h", "rgk_commit.h", "rgk_tree.h", "rgk_device.h", "rgk_trace.h", "rgk_shade.h", "rgk_bdpt.h", "rgk_resolve.h", "rgk_probe_kernels.h", "rgk_entry.h", "rgk_poison.h", "rgk_display.h", "rgk_pack.h", "device_types.h", os.path.join("..", "..", "include", "rgk.h"), os.path.join("..", "..", "include", "rgk_libm.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
         # CPU/GPU agreement: no FMA contraction on either side (DESIGN.md "Numerics")
         "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-x", "hip"]
# Per-source flags, behind FLAGS and in front of `extra` (so a tuning variant can take one back: extra=["-fslp-vectorize"]).
# The shading kernels are built without SLP vectorisation: no packed fp32 (v_pk_mul_f32 / v_pk_add_f32) on their most loaded
# resource, the non-fp32 VALU pipe; the walkers in rgk_kernels.hip keep the default.
SOURCE_FLAGS = {"rgk_shade_kernels.hip": ["-fno-slp-vectorize"]}
LINK_FLAGS = ["--offload-arch=gfx950", "-fPIC", "-shared"]
LIBS = ["-ldl"]


def up_to_date():
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    return all(os.path.getmtime(os.path.join(CSRC, f)) <= t for f in SOURCES + HEADERS)


def compile_command(hipcc, source, obj, extra=()):
    """The command that compiles one source of SOURCES to `obj`."""
    return [hipcc] + FLAGS + SOURCE_FLAGS.get(source, []) + list(extra) + ["-c", os.path.join(CSRC, source), "-o", obj]


def build(force=False, verbose=True, extra=(), out=None):
    """`extra` / `out`: tuning variants (-DRGK_TOP_NODES=...), built beside the product library."""
    if out is None and up_to_date() and not force:
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    work = tempfile.mkdtemp(prefix="rgk_build_")
    try:
        objs, procs = [], []
        for s in SOURCES:  # all at once: a dozen compilations, two of them long
            obj = os.path.join(work, os.path.splitext(s)[0] + ".o")
            cmd = compile_command(hipcc, s, obj, extra)
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            objs.append(obj)
            procs.append((cmd, subprocess.Popen(cmd)))
        failed = [cmd for cmd, p in procs if p.wait() != 0]
        if failed:
            raise subprocess.CalledProcessError(1, failed[0])
        cmd = [hipcc] + LINK_FLAGS + objs + ["-o", out or LIB] + LIBS
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out or LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
