#!/bin/bash
# Device code of two checkouts, compared kernel by kernel (no GPU needed): tools/device_code_diff.sh <parent-tree> <head-tree>
#
# Compiles rgk_kernels.hip, rgk_shade_kernels.hip, rgk_post.hip, rgk_pack.hip and rgk_build.hip of both trees to gfx950 assembly with the command
# recorded in profiles/host_split_device_code.txt (per source: the flags rgk_amd/build.py SOURCE_FLAGS gives it), normalises what
# differs between two checkouts of the SAME source (the checkout path and the compilation-unit word __hip_cuid_<16 hex digits>)
# and prints
#   per source: the sha256 of the normalised .s on both sides;
#   per kernel: `same`, or the two rows of VGPRs, scratch bytes, LDS bytes, occupancy and code bytes.
# A kernel is `same` when its whole block of the assembly -- instructions, descriptor, register and scratch figures -- is
# byte-identical.  Exit status: 0 every kernel same, 1 some differ or exist on one side only, 2 usage or compiler failure.
set -uo pipefail
[ $# -eq 2 ] || { echo "usage: $0 <parent-tree> <head-tree>" >&2; exit 2; }
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
command -v "$HIPCC" >/dev/null || { echo "$0: no hipcc ($HIPCC)" >&2; exit 2; }
CXXFILT=$(dirname "$(readlink -f "$(command -v "$HIPCC")")")/../llvm/bin/llvm-cxxfilt
[ -x "$CXXFILT" ] || CXXFILT=$(command -v llvm-cxxfilt || command -v c++filt || echo cat)
SOURCES="rgk_kernels rgk_shade_kernels rgk_post rgk_pack rgk_build"
# rgk_amd/build.py SOURCE_FLAGS: the shading kernels are built without SLP vectorisation
source_flags() { case $1 in rgk_shade_kernels) echo -fno-slp-vectorize ;; esac; }
work=$(mktemp -d) || exit 2
trap 'rm -rf "$work"' EXIT

pids=()
for side in parent head; do
    if [ $side = parent ]; then tree=$1; else tree=$2; fi
    tree=$(cd "$tree" && pwd) || exit 2
    mkdir -p "$work/$side"
    for f in $SOURCES; do
        [ -e "$tree/rgk_amd/csrc/$f.hip" ] || { : >"$work/$side/$f.s"; continue; } # a tree from before the source existed: its kernels show as absent
        (cd "$tree" && "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math $(source_flags $f) -x hip --cuda-device-only -S -Iinclude \
             rgk_amd/csrc/$f.hip -o "$work/$side/$f.raw" 2>"$work/$side/$f.err" &&
         sed -e "s|$tree|TREE|g" -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid_X/g' "$work/$side/$f.raw" >"$work/$side/$f.s") &
        pids+=($!)
    done
done
for p in "${pids[@]}"; do
    wait "$p" || { echo "$0: compilation failed" >&2; cat "$work"/*/*.err >&2; exit 2; }
done

# one file per kernel (its label up to its `; Occupancy:` line) and an index line: name, file, vgprs, scratch, lds, occupancy, code
split_kernels() { # <file.s> <directory>
    mkdir -p "$2"
    awk -v dir="$2" '
        /^\t\.type\t.*,@function/ { fn = $2; sub(/,.*/, "", fn) }
        !inb && /^[A-Za-z_$.0-9]+:/ { s = $1; sub(/:.*/, "", s); if (s == fn) { inb = 1; n++; out = dir "/" n ".txt"; name = s } }
        inb { print > out }
        inb && /^; codeLenInByte/ { code = $4 }
        inb && /^; NumVgprs:/ { v = $3 }
        inb && /^; ScratchSize:/ { sc = $3 }
        inb && /^; LDSByteSize:/ { l = $3 }
        inb && /^; Occupancy:/ { printf "%s\t%s\t%d\t%d\t%d\t%d\t%d\n", name, out, v, sc, l, $3, code; close(out); inb = 0 }' "$1" >"$2/index"
}

status=0
for f in $SOURCES; do
    hp=$(sha256sum <"$work/parent/$f.s" | cut -d' ' -f1); hh=$(sha256sum <"$work/head/$f.s" | cut -d' ' -f1)
    printf '%s.s  parent %s  head %s  %s\n' $f $hp $hh "$([ $hp = $hh ] && echo identical || echo differs)"
    split_kernels "$work/parent/$f.s" "$work/parent/$f.k"
    split_kernels "$work/head/$f.s" "$work/head/$f.k"
    [ -s "$work/head/$f.k/index" ] || { echo "$0: no kernel found in $f.s" >&2; exit 2; }
    # parent's kernels in their order, then those only the head has
    { cut -f1 "$work/parent/$f.k/index"; cut -f1 "$work/head/$f.k/index"; } | awk '!seen[$0]++' | while read -r sym; do
        shown=$(echo "$sym" | "$CXXFILT" | sed -e 's/(anonymous namespace):://g' -e 's/^void //' -e 's/>(.*$/>/' -e 's/^\([A-Za-z_0-9]*\)(.*$/\1/')
        rp=$(awk -F'\t' -v s="$sym" '$1 == s' "$work/parent/$f.k/index"); rh=$(awk -F'\t' -v s="$sym" '$1 == s' "$work/head/$f.k/index")
        row() { echo "$2" | awk -F'\t' -v side=$1 '{ printf "    %-6s vgprs %3d  scratch %4d  lds %6d  occupancy %d  code %6d\n", side, $3, $4, $5, $6, $7 }'; }
        if [ -n "$rp" ] && [ -n "$rh" ] && cmp -s "$(echo "$rp" | cut -f2)" "$(echo "$rh" | cut -f2)"; then
            printf '  %-72s same\n' "$shown"
        else
            printf '  %s\n' "$shown"
            if [ -n "$rp" ]; then row parent "$rp"; else echo "    parent (absent)"; fi
            if [ -n "$rh" ]; then row head "$rh"; else echo "    head   (absent)"; fi
            echo differs >>"$work/differs"
        fi
    done
done
[ -e "$work/differs" ] && status=1
exit $status
