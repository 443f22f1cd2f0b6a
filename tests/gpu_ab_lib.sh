#!/bin/bash
# usage (GPU box): tests/gpu_ab_lib.sh LIB_A LIB_B [reps] — bench.py's headline step, whole-pair leg and solver leg under two
# builds of the library, alternating on the same box (boxes differ by a few per cent, runs by ~1.5 %)
A=$1; B=$2; reps=${3:-3}
R=$(cd "$(dirname "$0")/.." && pwd); J=$(mktemp); trap 'rm -f "$J"' EXIT
for r in $(seq $reps); do
  for lib in $A $B; do
    QTR_LIB=$lib timeout -k 10 200 python $R/bench.py --full --steps 60 --cpu-seconds 0 --legs pair,solver5k > $J 2>/dev/null || exit $?
    python - "$(basename $lib)" "$J" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
rr = d.get("repeat_regions", {})
print(sys.argv[1], round(d["value"], 1), "reg/s", "ms_per_step", round(d["ms_per_step"], 4), "repeat median", rr.get("median"),
      "| whole pair ms", round(d.get("whole_pair_leg", {}).get("ms_per_step", 0), 4), "| solver5k ms",
      round(d.get("solver_L5000_leg", {}).get("ms_per_solve", 0), 4))
PY
  done
done
