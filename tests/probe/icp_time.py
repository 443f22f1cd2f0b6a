"""Device time of the ICP refinement on a 16 k-voxel pair (synth.kitti64_pair_16k(0), target tilted by roll 1.5 deg /
pitch -1.0 deg, refined from the registration's result): per refine (grid build + iterations, hipEvent based) and per
iteration, for both methods: medians over --reps repetitions (20), and under "spread" every figure's median, min and max.
The launch counts come from a run under `rocprofv3 --kernel-trace --stats -- python
tests/probe/icp_time.py --once`.  QTR_ICP_BLOCK=n in the environment: n launches between read-backs of the stop flag.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def main():
    import torch  # noqa: F401
    import icp_restate as R
    from quatro_amd import lib as ql
    from quatro_amd import synth
    once = "--once" in sys.argv
    h = ql.Handle(0)
    s, t, Tgt = synth.kitti64_pair_16k(0)
    t = R.apply(R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3)), t)
    r = h.register_pair(s, t, ql.default_frontend_params(seed=0))
    out = {"n_src": r["n_src"], "n_tgt": r["n_tgt"], "icp_block": int(os.environ.get("QTR_ICP_BLOCK", "0"))}
    for name, method in (("point_to_plane", 0), ("point_to_point", 1)):
        prm = ql.default_icp_params(method=method)
        reps = 1 if once else (int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20)
        grid, iters, wall, its = [], [], [], 0
        for _ in range(reps):
            t0 = time.perf_counter()
            g = h.refine_pair(None, prm)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = h.debug_fetch(ql.DBG_ICP_TIMES, np.float32)
            grid.append(float(ms[0]))
            iters.append(float(ms[1]))
            its = g["iterations"]
        # a fixed-count run (no early stop) gives the cost of one iteration
        fixed = ql.default_icp_params(method=method, max_iterations=30, transformation_epsilon=0.0,
                                      euclidean_fitness_epsilon=0.0)
        per = []
        for _ in range(reps):
            g30 = h.refine_pair(None, fixed)
            per.append(float(h.debug_fetch(ql.DBG_ICP_TIMES, np.float32)[1]) / max(g30["iterations"], 1))
        out[name] = {"iterations": its, "stop_reason": g["stop_reason"], "grid_ms": float(np.median(grid)),
                     "loop_ms": float(np.median(iters)), "refine_wall_ms": float(np.median(wall)),
                     "per_iteration_ms": float(np.median(per)), "fixed_run_iterations": g30["iterations"],
                     "spread": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}
                                for k, v in (("grid_ms", grid), ("loop_ms", iters), ("refine_wall_ms", wall), ("per_iteration_ms", per))}}
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
