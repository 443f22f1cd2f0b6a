"""Time of a registration evaluation on the device against the host route callers had before qtr_evaluate_keyframes, one
handle, same process, on the 16k pool of DESIGN §10.

  (a) host route: two Keyframe.fetch(KF_VOX) (+ KF_NORMALS of the target) + scipy.spatial.cKDTree query + the numpy sums
      (overlap, inlier RMSE, sum G^T G, sum J^T J)
  (b) Handle.evaluate_keyframes on the same pair
  (c) Handle.evaluate_keyframes_batch on 16 pairs (one query against 16 targets), per batch and per pair
(a), (b), (c) alternate call by call; median [min - max] of --reps repetitions of --rounds calls.  With --one the process
makes one evaluate_keyframes and one single-iteration point-to-plane ICP on pair 0 and exits: the run to put under
`rocprofv3 --kernel-trace --stats` for k_eval's own duration beside one k_icp_iter launch.  Writes one JSON object (--out).

  python tests/probe/eval_time.py [--reps 5] [--rounds 10] [--out profiles/eval_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)


def _mmm(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def host_route(ql, ks, kt, T, max_d):
    from scipy.spatial import cKDTree
    s, t, n = ks.fetch(ql.KF_VOX), kt.fetch(ql.KF_VOX), kt.fetch(ql.KF_NORMALS)
    q = s[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d, j = cKDTree(t[:, :3].astype(np.float64)).query(q, distance_upper_bound=max_d)
    has = np.isfinite(d)
    tt, qq, nn = t[j[has], :3].astype(np.float64), q[has], n[j[has], :3].astype(np.float64)
    G = np.zeros((tt.shape[0], 3, 6))
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = tt[:, 2], -tt[:, 1], -tt[:, 2], tt[:, 0], tt[:, 1], -tt[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    J = np.concatenate([np.cross(qq, nn), nn], axis=1)
    return {"overlap": has.mean(), "inlier_rmse": float(np.sqrt((d[has] ** 2).mean())),
            "information": np.einsum("nij,nik->jk", G, G), "hessian_plane": J.T @ J}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--one", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401
    from quatro_amd import lib as ql
    from quatro_amd import synth
    h = ql.Handle(0, n_slots=1)
    fp = ql.default_frontend_params(seed=0)
    prm = ql.default_eval_params(max_correspondence_distance=0.5)
    kfs = []
    for k in range(1 if a.one else 16):
        s, t, _ = synth.kitti64_pair_16k(k)
        kfs.append((h.keyframe(s, fp), h.keyframe(t, fp)))
    T = h.register_keyframes(kfs[0][0], kfs[0][1], fp)["T"]
    if a.one:
        h.evaluate_keyframes(kfs[0][0], kfs[0][1], T, prm)
        h.refine_pair(T, ql.default_icp_params(max_iterations=1, max_correspondence_distance=0.5))
        h.close()
        return
    pairs = [(kfs[0][0], kt, T) for _, kt in kfs]
    want, got = host_route(ql, kfs[0][0], kfs[0][1], T, 0.5), h.evaluate_keyframes(kfs[0][0], kfs[0][1], T, prm)  # warm-up
    h.evaluate_keyframes_batch(pairs, prm)
    out = {"pool": "kitti64_pair_16k(0..15)", "unit": "ms", "max_d": 0.5, "n_source": got["n_source"], "n_corr": got["n_corr"],
           "overlap_device": got["overlap"], "overlap_host_route": float(want["overlap"])}
    ra, rb, rc = [], [], []
    for _ in range(a.reps):
        ta = tb = tc = 0.0
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            host_route(ql, kfs[0][0], kfs[0][1], T, 0.5)
            t1 = time.perf_counter()
            h.evaluate_keyframes(kfs[0][0], kfs[0][1], T, prm)
            t2 = time.perf_counter()
            h.evaluate_keyframes_batch(pairs, prm)
            t3 = time.perf_counter()
            ta, tb, tc = ta + t1 - t0, tb + t2 - t1, tc + t3 - t2
        ra.append(1e3 * ta / a.rounds)
        rb.append(1e3 * tb / a.rounds)
        rc.append(1e3 * tc / a.rounds)
    out["host_route"], out["evaluate_keyframes"], out["batch_16"] = _mmm(ra), _mmm(rb), _mmm(rc)
    out["batch_16_per_pair"] = _mmm(np.asarray(rc) / 16)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    h.close()


if __name__ == "__main__":
    main()
