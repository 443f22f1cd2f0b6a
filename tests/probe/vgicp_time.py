"""Device time of voxelised plane-to-plane (method 3, VGICP) beside plane-to-plane (method 2) in the SAME run, the two
alternating repetition by repetition on the same handle:
  single:  kitti64_pair_16k(0), target tilted by roll 1.5 deg / pitch -1.0 deg, refined from the registration's result:
           updates to the stop, the enqueued loop and one iteration of a fixed-count run of 30 updates (hipEvent based,
           QTR_DBG_ICP_TIMES[1]), the grid build (QTR_DBG_ICP_TIMES[0]: box, read-back, counting sort - and for method 3 the
           voxel records, so the difference of the two columns is k_icp_voxel_order + k_icp_voxel_stats), the whole
           qtr_refine_pair wall; --reps repetitions (at least 10);
  batched: the 64 tilted 16 k-voxel pairs of icp_batch_time.py on one handle of --slots slots: register_batch_refine
           pairs/s for both methods, and the refined records against register_pair + refine_pair on 8 of the pairs.
Every figure as median, min and max.  Prints one JSON line and writes it to profiles/vgicp_time.json.
--once: one refine of each method and one refining batch of each, for a kernel trace of its own."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

METHODS = (("plane_to_plane", 2), ("voxel_plane_to_plane", 3))


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def single(ql, reps):
    import icp_restate as R
    from quatro_amd import synth
    h = ql.Handle(0)
    s, t, Tgt = synth.kitti64_pair_16k(0)
    tilt = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
    t, Tgt = R.apply(tilt, t), tilt @ Tgt
    r = h.register_pair(s, t, ql.default_frontend_params(seed=0))
    out = {"n_src": r["n_src"], "n_tgt": r["n_tgt"]}
    for name, method in METHODS:  # (warm-up: arenas, code objects)
        h.refine_pair(None, ql.default_icp_params(method=method))
    acc = {name: {"loop": [], "wall": [], "per": [], "grid": []} for name, _ in METHODS}
    last = {}
    for _ in range(reps):  # (the two methods alternate inside every repetition)
        for name, method in METHODS:
            prm = ql.default_icp_params(method=method)
            fixed = ql.default_icp_params(method=method, max_iterations=30, transformation_epsilon=0.0,
                                          euclidean_fitness_epsilon=0.0)
            t0 = time.perf_counter()
            g = h.refine_pair(None, prm)
            acc[name]["wall"].append((time.perf_counter() - t0) * 1e3)
            tm = h.debug_fetch(ql.DBG_ICP_TIMES, np.float32)
            acc[name]["grid"].append(float(tm[0]))
            acc[name]["loop"].append(float(tm[1]))
            g30 = h.refine_pair(None, fixed)
            acc[name]["per"].append(float(h.debug_fetch(ql.DBG_ICP_TIMES, np.float32)[1]) / max(g30["iterations"], 1))
            last[name] = (g, g30)
    for name, _ in METHODS:
        g, g30 = last[name]
        out[name] = {"iterations": g["iterations"], "stop_reason": g["stop_reason"], "n_corr": g["n_corr"],
                     "rot_err_deg": R.rot_err_deg(g["T"], Tgt),
                     "trans_err_m": float(np.linalg.norm(g["T"][:3, 3] - Tgt[:3, 3])),
                     "loop_ms": _stats(acc[name]["loop"]), "grid_build_ms": _stats(acc[name]["grid"]),
                     "refine_wall_ms": _stats(acc[name]["wall"]), "per_iteration_ms": _stats(acc[name]["per"]),
                     "fixed_run_iterations": g30["iterations"]}
    h.close()
    return out


def batched(ql, reps, slots, once):
    from icp_batch_time import make_pairs
    pairs = make_pairs()
    B = len(pairs)
    h = ql.Handle(0, n_slots=slots)
    out = {"pairs": B, "slots": slots}
    if not once:
        h.register_batch(pairs[:slots])  # (warm-up)
        for name, method in METHODS:
            h.register_batch_refine(pairs[:slots], icp=ql.default_icp_params(method=method))
    for name, method in METHODS:
        icp = ql.default_icp_params(method=method)
        rate, refined = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            _, refined = h.register_batch_refine(pairs, icp=icp, want_lists=False)
            rate.append(B / (time.perf_counter() - t0))
        same = 0
        for k in range(0, B, 8):
            s, t, seed = pairs[k]
            h.register_pair(s, t, ql.default_frontend_params(seed=seed))
            a, b = h.refine_pair(None, icp), refined[k]
            same += int(np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)) and a["iterations"] == b["iterations"])
        out[name] = {"register_batch_refine_pairs_per_s": _stats(rate),
                     "iterations_mean": float(np.mean([g["iterations"] for g in refined])),
                     "bit_equal_to_sequential": f"{same}/{len(range(0, B, 8))}"}
    h.close()
    return out


def main():
    import torch  # noqa: F401
    from quatro_amd import lib as ql
    once = "--once" in sys.argv
    reps = 1 if once else _arg("--reps", 5)
    out = {"single": single(ql, 1 if once else max(reps, 10)), "batched": batched(ql, reps, _arg("--slots", 16), once)}
    print(json.dumps(out))
    if not once:
        prof = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles"))
        os.makedirs(prof, exist_ok=True)
        with open(os.path.join(prof, "vgicp_time.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
