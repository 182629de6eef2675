#!/bin/bash
# Static instruction mix of every kernel, from the gfx950 assembly (no GPU needed): tools/kernel_mix.sh [extra hipcc flags]
#
# What tools/kernel_regs.sh prints, and the instructions behind it.  Per kernel, counted in the kernel's own block of the assembly:
#   valu      vector-ALU instructions (every v_*; loads, stores, LDS and scalar instructions are not among them)
#   pk_f32    packed fp32 among them (v_pk_mul_f32, v_pk_add_f32, v_pk_fma_f32, v_pk_mov_b32 is not one)
#   rdlane / wrlane   v_readlane_b32 / v_writelane_b32: SGPR spills to VGPR lanes and their reloads
#   s_nop     hazard and wait-state fillers
#   v_mov     v_mov_b32
#   f64       fp64 VALU instructions (v_*_f64)
#   vgprs, sgprs (with VCC), scratch bytes, occupancy (waves per SIMD), code bytes
# The counts are static: an instruction in a loop or on a rare branch counts once.
# SRC="rgk_kernels rgk_shade_kernels" (default) | rgk_post | rgk_build: the device sources; each is compiled with the flags
# rgk_amd/build.py SOURCE_FLAGS gives it, then the extra flags.  TREE=<checkout>: another tree's sources (a source it lacks is skipped).
# ONLY=<regex>: kernels whose shown name matches.
R=${TREE:-$(cd "$(dirname "$0")/.." && pwd)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CXXFILT=$(dirname "$(readlink -f "$(command -v "$HIPCC")")")/../llvm/bin/llvm-cxxfilt
[ -x "$CXXFILT" ] || CXXFILT=$(command -v llvm-cxxfilt || command -v c++filt || echo cat)
work=$(mktemp -d) || exit 2
trap 'rm -rf "$work"' EXIT
printf '%-44s %5s %6s %6s %6s %5s %5s %4s %5s %5s %7s %3s %6s\n' kernel valu pk_f32 rdlane wrlane s_nop v_mov f64 vgprs sgprs scratch occ code
for src in ${SRC:-rgk_kernels rgk_shade_kernels}; do
    [ -e "$R/rgk_amd/csrc/$src.hip" ] || continue
    case $src in rgk_shade_kernels) own=-fno-slp-vectorize ;; *) own= ;; esac
    "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math $own -x hip --cuda-device-only -S "$@" \
        -I"$R/include" "$R/rgk_amd/csrc/$src.hip" -o "$work/$src.s" 2>"$work/$src.err" || { cat "$work/$src.err" >&2; exit 1; }
    awk '
        /^\t\.type\t.*,@function/ { fn = $2; sub(/,.*/, "", fn) }
        !inb && /^[A-Za-z_$.0-9]+:/ { s = $1; sub(/:.*/, "", s); if (s == fn) { inb = 1; name = s; valu = pk = rl = wl = nop = mov = f64 = 0 } }
        inb && /^\tv_/ { valu++ }
        inb && /^\tv_pk_[a-z]+_f32/ { pk++ }
        inb && /^\tv_readlane_b32/ { rl++ }
        inb && /^\tv_writelane_b32/ { wl++ }
        inb && /^\ts_nop/ { nop++ }
        inb && /^\tv_mov_b32/ { mov++ }
        inb && /^\tv_[a-z0-9_]+_f64/ { f64++ }
        inb && /^; codeLenInByte/ { code = $4 }
        inb && /^; TotalNumSgprs:/ { sg = $3 }
        inb && /^; NumVgprs:/ { vg = $3 }
        inb && /^; ScratchSize:/ { sc = $3 }
        inb && /^; Occupancy:/ { printf "%s\t%d %d %d %d %d %d %d %d %d %d %d %d\n", name, valu, pk, rl, wl, nop, mov, f64, vg, sg, sc, $3, code; inb = 0 }' "$work/$src.s" |
    while IFS=$'\t' read -r sym rest; do
        shown=$(echo "$sym" | "$CXXFILT" | sed -e 's/(anonymous namespace):://g' -e 's/^void //' -e 's/>(.*$/>/' -e 's/^\([A-Za-z_0-9]*\)(.*$/\1/')
        case $shown in k_*) ;; *) continue ;; esac
        [ -n "${ONLY:-}" ] && ! echo "$shown" | grep -Eq "$ONLY" && continue
        printf '%-44s %5d %6d %6d %6d %5d %5d %4d %5d %5d %7d %3d %6d\n' "$shown" $rest
    done
done
