# usage: tools/var_sweep.sh a b c ...   -- bench each tuning variant librgk_var_<x>.so ("base" = product library; lines: $OUT/var_*, default out/)
O=${OUT:-out}
mkdir -p $O
for v in "$@"; do
  if [ "$v" = base ]; then unset RGK_LIB; else export RGK_LIB=$PWD/rgk_amd/csrc/librgk_var_$v.so; fi
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 2 $BENCH_ARGS > $O/var_$v.json 2> $O/var_$v.err || { echo "variant $v failed"; tail -3 $O/var_$v.err; exit 1; }
  python - <<PY
import json
d=json.load(open("$O/var_$v.json"))
r=d["roofline"]
print("variant $v", d["value"], "ms/step", d["ms_per_step"], "nodes", r["whole_round"]["nodes_per_path_ray"], {k["kernel"]: k["ms_per_step"] for k in r["kernels"]})
PY
done
