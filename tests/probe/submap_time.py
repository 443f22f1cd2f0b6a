"""Time of a submap built on the device against the only route there was before qtr_keyframe_merge, one handle, same process.

  (a) host route: K x Keyframe.fetch(KF_VOX) + the numpy transform and concatenation + Handle.keyframe(host cloud)
  (b) Handle.merge_keyframes(members, poses)
for K = 5, 11, 51 members of kitti64_trajectory(0, 51, 1.0, **KITTI16K) (~16 k voxels each) around the middle of the path,
alternating (a, b, a, b ...) after a warm-up of both, the host clock around calls that end in a synchronise; per repetition
the mean over --rounds calls, reported as median [min - max] of the repetitions.  Also: api.close_loop with k = 16 on the
revisit, without submaps and with submap_half_width = 2.  Writes one JSON object (--out) and prints it.

  python tests/probe/submap_time.py [--reps 5] [--rounds 10] [--out profiles/submap_time.json]
  python tests/probe/submap_time.py --trace    # a short run for a kernel trace (k_kf_gather's duration)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def _mmm(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--scans", type=int, default=51)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from quatro_amd import lib as ql
    from quatro_amd import api, synth
    import submap_restate as sr

    n, mid = a.scans, a.scans // 2
    scans, poses = synth.kitti64_trajectory(0, n, 1.0, **synth.KITTI16K)
    h = ql.Handle(0, max_points=1 << 20, max_voxels=1 << 18, n_slots=16)
    h.set_stage_events(False)
    fp = ql.default_frontend_params()
    kfs = [h.keyframe(s, slot=i % 16) for i, s in enumerate(scans)]
    out = {"members": f"kitti64_trajectory(0, {n}, 1.0, **KITTI16K)", "unit": "ms",
           "n_voxels": _mmm([k.info["n_voxels"] for k in kfs])}

    def window(K):
        ids = list(range(max(mid - K // 2, 0), min(mid + K // 2 + 1, n)))
        return ids, np.stack([np.linalg.inv(poses[mid]) @ poses[i] for i in ids])

    def host_route(ids, rel):
        t0 = time.perf_counter()
        cat = sr.merge([kfs[i].fetch(ql.KF_VOX) for i in ids], rel)
        kf = h.keyframe(cat, fp)
        return (time.perf_counter() - t0) * 1e3, kf

    def device_route(ids, rel):
        t0 = time.perf_counter()
        kf = h.merge_keyframes([kfs[i] for i in ids], rel, fp)
        return (time.perf_counter() - t0) * 1e3, kf

    if a.trace:
        for K in (5, 11, n):
            ids, rel = window(K)
            for _ in range(4):
                device_route(ids, rel)[1].close()
        h.close()
        return
    for K in sorted({5, 11, n}):
        ids, rel = window(K)
        ka, kb = host_route(ids, rel)[1], device_route(ids, rel)[1]  # warm-up of both, and the bits
        assert ka.info == kb.info and np.array_equal(ka.fetch(ql.KF_FPFH).view(np.uint32), kb.fetch(ql.KF_FPFH).view(np.uint32)), K
        rec = {"members": len(ids), "voxels_in": ka.info["n_points"], "voxels_out": ka.info["n_voxels"]}
        ka.close()
        kb.close()
        rep_a, rep_b = [], []
        for _ in range(a.reps):
            ta = tb = 0.0
            for _ in range(a.rounds):
                t, k = host_route(ids, rel)
                k.close()
                ta += t
                t, k = device_route(ids, rel)
                k.close()
                tb += t
            rep_a.append(ta / a.rounds)
            rep_b.append(tb / a.rounds)
        rec["host_route"], rec["merge_keyframes"] = _mmm(rep_a), _mmm(rep_b)
        rec["ratio_host_over_merge"] = statistics.median(rep_a) / statistics.median(rep_b)
        rec["merge_max_below_host_min"] = max(rep_b) < min(rep_a)
        out[f"K{len(ids)}"] = rec

    with h.place_index(n) as ix:
        for kf in kfs[:n]:
            ix.add(kf)
        q = kfs[n]
        for hw in (0, 2):
            api.close_loop(h, ix, kfs, q, 16, fp=fp, poses=poses, submap_half_width=hw)
        ca, cb = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            api.close_loop(h, ix, kfs, q, 16, fp=fp)
            ca.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            r = api.close_loop(h, ix, kfs, q, 16, fp=fp, poses=poses, submap_half_width=2)
            cb.append((time.perf_counter() - t0) * 1e3)
        out["close_loop_k16_single_keyframes"] = _mmm(ca)
        out["close_loop_k16_submaps_hw2"] = _mmm(cb)
        out["close_loop_best_id"] = r["best_id"]
    h.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
