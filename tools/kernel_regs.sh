#!/bin/bash
# Registers / scratch / occupancy of every kernel, from the gfx950 assembly (no GPU needed): tools/kernel_regs.sh [extra hipcc flags]
# SRC=rgk_shade_kernels (or rgk_post, rgk_build) lists that device source's kernels instead of rgk_kernels.hip's.  A source is compiled
# with the flags rgk_amd/build.py SOURCE_FLAGS gives it; tools/kernel_mix.sh adds the instruction mix.
src=${SRC:-rgk_kernels}
out=${TMPDIR:-/tmp}/$src.s
case $src in rgk_shade_kernels) own=-fno-slp-vectorize ;; *) own= ;; esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math $own -x hip --cuda-device-only -S "$@" \
    -I$(dirname $0)/../include $(dirname $0)/../rgk_amd/csrc/$src.hip -o $out 2>/dev/null || exit 1
awk '/^_Z[0-9]+k_[a-z_]+/{n=$1; sub(/^_Z[0-9]+/,"",n); sub(/(8DevScene|10PassParams|ILb|ILi|Pj|j).*/,"",n); name=n}
     /; NumVgprs:/{v=$3} /; ScratchSize:/{s=$3} /; Occupancy:/{printf "%-24s vgprs %3d scratch %4d occupancy %d\n", name, v, s, $3}' $out
