export BENCH_ARGS="--workload dragon-sponza-1080p"
O=${OUT:-out}
mkdir -p $O
for v in ploc host karras; do
  case $v in ploc) unset RGK_BVH_BUILD RGK_LBVH_PLOC;; host) export RGK_BVH_BUILD=host;; karras) unset RGK_BVH_BUILD; export RGK_LBVH_PLOC=0;; esac
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 2 $BENCH_ARGS > $O/dragon_$v.json 2> $O/dragon_$v.err || { echo "failed $v"; tail -3 $O/dragon_$v.err; exit 1; }
  python - <<PY
import json
d=json.load(open("$O/dragon_$v.json"))
r=d["roofline"]
print("$v", d["value"], "ms/step", d["ms_per_step"], {k["kernel"]: k["ms_per_step"] for k in r["kernels"]})
PY
done
