#!/bin/bash
# usage: tools/pmc_passes.sh <tag> [bench args...]   -- separate rocprofv3 --pmc passes (counters only) of one bench round
# run on the GPU box; writes $OUT/pmc_<tag>_<pass>/ (default out/) and prints the per-kernel averages
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT:-$R/out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
i=0
while read -r line; do
  [ -z "$line" ] && continue
  i=$((i+1))
  out=$O/pmc_${tag}_$i
  rm -rf $out
  echo "pass $i: $line"
  timeout -k 10 240 rocprofv3 --pmc $line -d $out --output-format csv -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline "$@" > $out.json 2> $out.err
  python3 $R/tools/pmc_summary.py $out | grep -v "k_init\|k_build\|k_resolve\|k_raygen" 
done < <(cat ${PASSES:-$R/tools/pmc_default.txt})
