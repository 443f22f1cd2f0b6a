#!/bin/bash
# usage (GPU box): tests/gpu_ab_nn.sh [reps] — k_nn_f16 A/B on one box: the library of HEAD~ (libquatro_hip_base.so), the
# current one, and the current test-engine build with one workgroup per compute unit (QTR_NN_WGS_PER_CU=1)
reps=${1:-2}
R=$(cd "$(dirname "$0")/.." && pwd); J=$(mktemp); trap 'rm -f "$J"' EXIT
run() {  # label, env assignments...
  label=$1; shift
  env "$@" timeout -k 10 200 python $R/bench.py --full --steps 60 --cpu-seconds 0 --legs pair > $J 2>/dev/null || exit $?
  python - "$label" "$J" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
r = d["roofline"]
print(sys.argv[1], "ms_per_step", round(d["ms_per_step"], 4), "| nn launch us", round(1e3 * r["mean_launch_ms"], 2), "frac", round(r["frac"], 3),
      "| stages", {k: round(v, 4) for k, v in d.get("stage_ms", {}).items() if isinstance(v, (int, float))})
PY
}
for r in $(seq $reps); do
  run base QTR_LIB=$R/quatro_amd/libquatro_hip_base.so
  run new QTR_LIB=$R/quatro_amd/libquatro_hip.so
  run new_1wg QTR_LIB=$R/quatro_amd/libquatro_hip_testengines.so QTR_NN_WGS_PER_CU=1
done
