"""tools/device_code_diff.sh, the gate of refactors that must leave the device code alone: this tree against itself.

Compiler output only -- no GPU, nothing executed.  Both sides are compiled (three device sources each, side by side), the
checkout path and the compilation-unit word are normalised, and every kernel must come out `same`: the normalisation is complete,
the per-kernel split finds the kernels, and two compilations of one source agree."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc: the tool compares compiler output")
def test_device_code_diff_of_the_tree_against_itself():
    r = subprocess.run([os.path.join(ROOT, "tools", "device_code_diff.sh"), ROOT, ROOT], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    sources = [ln for ln in lines if re.match(r"rgk_(kernels|post|build)\.s  parent [0-9a-f]{64}  head [0-9a-f]{64}  ", ln)]
    assert len(sources) == 3 and all(ln.endswith("  identical") for ln in sources), sources
    kernels = [ln for ln in lines if ln.startswith("  ")]
    assert len(kernels) > 100 and all(ln.rstrip().endswith(" same") for ln in kernels), [ln for ln in kernels if not ln.rstrip().endswith(" same")][:5]
    shown = [ln.split()[0] for ln in kernels]
    # the walkers in every variant a launch can pick, spelled as a profiler prints them (rgk_amd/capi.py KERNEL_NAMES)
    for name in ("k_trace_closest", "k_trace_camera", "k_trace_shadow", "k_trace_shadow_first", "k_trace_shadow_cl", "k_trace_shadow_first_cl", "k_trace_shadow_jobs"):
        assert sum(ln.strip().startswith(name + "<") for ln in kernels) == 6, name
    assert sum(ln.strip().startswith("k_trace_camera_beam<") for ln in kernels) == 2 and "k_raygen_light" in shown
    # the shading kernels in every variant rgk_launch_shade / rgk_launch_shade_light can pick, and the plain kernels of the headers
    # rgk_kernels.hip includes: a split that loses an instantiation or a header fails here
    assert sum(ln.strip().startswith("k_shade<") for ln in kernels) == 12
    assert sum(ln.strip().startswith("k_shade_light<") for ln in kernels) == 2
    for name in ("k_connect", "k_resolve", "k_resolve_tiled", "k_entry_points", "k_entry_points_light"):
        assert name in shown, name
    # a call it cannot serve ends with status 2, never with 0
    assert subprocess.run([os.path.join(ROOT, "tools", "device_code_diff.sh"), ROOT], capture_output=True).returncode == 2
