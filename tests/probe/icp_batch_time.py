"""Throughput of the batched refinement (qtr_submit_batch_refine) against the batch without it and the sequential
single-pair path, on 64 tilted 16 k-voxel pairs (synth.kitti64_pair_16k(0..15), each target tilted four ways by a seeded
roll / pitch of 0.5-2 deg), one batch handle:
  (a) register_batch pairs/s
  (b) register_batch_refine pairs/s, point-to-plane and point-to-point
  (c) register_pair + refine_pair pairs/s on slot 0 of the same handle
Every figure is repeated (--reps) and reported as median, min and max; the refined records of (b) are checked bit for
bit against (c) in the same run.  Prints one JSON line.
--once --slots N: one refining batch only, for `rocprofv3 --kernel-trace --stats -- python tests/probe/icp_batch_time.py
--once --slots N` (lanes of N / 2 pairs: k_icp_iter_group at G = N / 2)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def make_pairs():
    import icp_restate as R
    from quatro_amd import synth
    rng = np.random.default_rng(20261016)
    out = []
    for k in range(16):
        s, t, _ = synth.kitti64_pair_16k(k)
        for j in range(4):
            roll, pitch = rng.uniform(0.5, 2.0, 2) * rng.choice([-1, 1], 2)
            tilt = R.rigid(R.rot(np.radians(roll), np.radians(pitch), 0.0), np.zeros(3))
            out.append((s, R.apply(tilt, t), 4 * k + j))
    return out


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def main():
    import torch  # noqa: F401
    from quatro_amd import lib as ql
    reps = _arg("--reps", 3)
    slots = _arg("--slots", 16)
    pairs = make_pairs()
    B = len(pairs)
    h = ql.Handle(0, n_slots=slots)
    if "--once" in sys.argv:
        res, ref = h.register_batch_refine(pairs)
        h.close()
        print(json.dumps({"pairs": B, "slots": slots, "refined": sum(g["status"] == ql.QTR_OK for g in ref)}))
        return
    h.register_batch(pairs[:slots])  # (warm-up: arenas, code objects)
    h.register_batch_refine(pairs[:slots])
    out = {"pairs": B, "slots": slots, "icp_block": int(os.environ.get("QTR_ICP_BLOCK", "0"))}
    rate = []
    for _ in range(reps):
        t0 = time.perf_counter()
        h.register_batch(pairs, want_lists=False)
        rate.append(B / (time.perf_counter() - t0))
    out["a_register_batch_pairs_per_s"] = _stats(rate)
    for name, method in (("point_to_plane", 0), ("point_to_point", 1)):
        icp = ql.default_icp_params(method=method)
        rate, refined = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            _, refined = h.register_batch_refine(pairs, icp=icp, want_lists=False)
            rate.append(B / (time.perf_counter() - t0))
        seq_rate, seq_refine_ms, seq = [], [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            seq, tr = [], 0.0
            for s, t, seed in pairs:
                h.register_pair(s, t, ql.default_frontend_params(seed=seed))
                t1 = time.perf_counter()
                seq.append(h.refine_pair(None, icp))
                tr += time.perf_counter() - t1
            seq_rate.append(B / (time.perf_counter() - t0))
            seq_refine_ms.append(tr * 1e3 / B)
        same = sum(np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)) and a["iterations"] == b["iterations"]
                   and a["n_corr"] == b["n_corr"] for a, b in zip(refined, seq))
        a_ms = 1e3 / out["a_register_batch_pairs_per_s"]["median"]
        b_ms = 1e3 / float(np.median(rate))
        c_ms = 1e3 / float(np.median(seq_rate))
        out[name] = {"b_register_batch_refine_pairs_per_s": _stats(rate), "c_sequential_pairs_per_s": _stats(seq_rate),
                     "refine_added_ms_per_pair": b_ms - a_ms, "sequential_ms_per_pair": c_ms,
                     "sequential_refine_ms_per_pair": _stats(seq_refine_ms),
                     "target_ms_per_pair": 0.25 * float(np.median(seq_refine_ms)),
                     "iterations_mean": float(np.mean([g["iterations"] for g in refined])),
                     "bit_equal_to_sequential": f"{same}/{B}"}
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
