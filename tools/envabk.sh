#!/bin/bash
# tools/envabk.sh VAR "v1 v2 ..." [bench args]: per-kernel A/B of one build under VAR=v for each value on ONE GPU box,
# two interleaved repetitions; prints steps/s and the kernel table (us per launch) of every run.  The lines (bench.py
# --full: the kernel table is read) go to $OUT (default: out/).
var=$1; vals=$2; shift; shift
O=${OUT:-out}
mkdir -p $O
for rep in 1 2; do
  for v in $vals; do
    env $var=$v python bench.py --full --no-cpu --no-512 "$@" > $O/envk_${var}_${v}_${rep}.json 2> $O/envk_${var}_${v}_${rep}.err || { echo "$var=$v FAILED"; tail -3 $O/envk_${var}_${v}_${rep}.err; continue; }
    python - <<PY
import json
d=json.load(open("$O/envk_${var}_${v}_${rep}.json"))
print("$var=$v", "$rep", d["value"], {k.replace("k_",""): round(1e3*x["avg_ms"],1) for k,x in sorted(d["roofline"]["kernels"].items())})
PY
  done
done
