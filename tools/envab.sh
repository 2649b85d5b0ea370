#!/bin/bash
# tools/envab.sh VAR "v1 v2 ..." [bench args] : bench the current build under VAR=v for each value, two interleaved
# repetitions on one GPU; the lines (bench.py --full: the per-entry-point times are read) go to $OUT (default: out/)
var=$1; vals=$2; shift; shift
O=${OUT:-out}
mkdir -p $O
for rep in 1 2; do
  for v in $vals; do
    env $var=$v python bench.py --full --no-cpu "$@" > $O/env_${var}_${v}_${rep}.json
    python - <<PY
import json
d=json.load(open("$O/env_${var}_${v}_${rep}.json"))
print("$var=$v", "$rep", d["value"], {k: round(x["ms_per_step"],4) for k,x in d["roofline"]["entry_points"].items()})
PY
  done
done
