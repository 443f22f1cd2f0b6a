#!/bin/bash
# usage (GPU box): tests/gpu_ab_batch.sh VAR v1 v2 ... — bench.py's batched leg (256 composite pairs) on the test-engine build
# under values of one environment variable, two rounds, same box
var=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd); J=$(mktemp); trap 'rm -f "$J"' EXIT
export QTR_LIB=$R/quatro_amd/libquatro_hip_testengines.so
for r in 1 2; do
  for v in "$@"; do
    env $var=$v timeout -k 10 300 python $R/bench.py --full --steps 10 --cpu-seconds 0 --legs batch > $J 2>/dev/null || exit $?
    python - "$var=$v" "$J" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
b = d.get("batch256_leg", {})
print(sys.argv[1], "batch256", round(b.get("value", 0), 1), "reg/s", "| scan pairs", round(b.get("scan_pairs", {}).get("value", 0), 1))
PY
  done
done
