"""Time of evaluating poses against the voxel map (qtr_voxel_map_evaluate_batch) beside the routes it stands next to, all of
them alternating inside every repetition of ONE run on one MI355X (--reps repetitions, at least 10, after one warm-up
repetition; every figure as median, min and max with its count n):
  G:          1, 64 and 1024 poses.
  shared:     ONE keyframe (the source scan of synth.kitti64_pair_16k(0), about 16 k voxels) under G poses around the pair's
              transform, against a map of the target scan's keyframe (tests/probe/vmap_batch_time.py's "shared").
  eval_batch: VoxelMap.evaluate_batch of the G items; wall_ms is time.perf_counter around the call, dev_ms the library's own
              events around upload and launch (QTR_VMAP_EVAL_TIMES).
  eval_loop:  G single VoxelMap.evaluate_keyframe calls (wall).
  reg_batch:  VoxelMap.register_batch of the same G guesses, the default 30 iterations and epsilons (wall; 64 per chain).
  relocalize: api.relocalize on the room of tests/vmap_batch_cases.py under a 243-hypothesis grid (3 yaws x 9 x 9 offsets
              half a voxel side apart), without keep and with keep = 27 (wall), whether both name the same winner, where
              the full batch's winner stands in the scores' order, and how far apart and how far from the truth the two
              winners end.
Batch and loop must give the same bits (asserted once per G).
Not measured here: a map near its capacity; several slots evaluating at once; host-resident clouds (their staging copy);
the composite benchmark (bench.py), whose kernels this code does not touch (--bench-this / --bench-parent FILE: its
headline lines of the same session, recorded as given).
Prints one JSON line and writes it to profiles/vmap_eval_time.json (--out PATH: elsewhere)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def _offset(k):
    import icp_restate as R
    rng = np.random.default_rng(900 + k)
    return R.rigid(R.rot(*rng.uniform(-0.01, 0.01, 3)), rng.uniform(-0.15, 0.15, 3))


def main():
    import vmap_batch_cases as BC
    from quatro_amd import api, synth
    from quatro_amd import lib as ql
    reps = max(_arg("--reps", 10), 10)
    fp = ql.default_frontend_params()
    src, tgt, Tgt = synth.kitti64_pair_16k(0)
    h = ql.Handle(0)
    kf_s, kf_t = h.keyframe(src, fp), h.keyframe(tgt, fp)
    vm = h.voxel_map(1.0, 1 << 16)
    vm.insert_keyframe(kf_t, None)
    all_items = [(kf_s, np.asarray(Tgt) @ _offset(j)) for j in range(1024)]
    out = {"reps": reps, "shared": {"map_voxels": len(vm), "scan_voxels": int(kf_s.info["n_voxels"])}}
    for G in (1, 64, 1024):
        items = all_items[:G]
        acc = {k: [] for k in ("eval_batch_wall_ms", "eval_batch_dev_ms", "eval_loop_wall_ms", "reg_batch_wall_ms")}
        for rep in range(reps + 1):  # (the first repetition is the warm-up: the arenas, code objects)
            t0 = time.perf_counter()
            got = vm.evaluate_batch(items)
            t1 = time.perf_counter()
            dev = float(vm.eval_fetch(0, ql.VMAP_EVAL_TIMES)[0])
            t2 = time.perf_counter()
            one = [vm.evaluate_keyframe(kf, T) for kf, T in items]
            t3 = time.perf_counter()
            vm.register_batch(items)
            t4 = time.perf_counter()
            if rep == 0:
                assert all(a["n_corr"] == b["n_corr"] and np.array_equal(a["hessian"].view(np.uint64), b["hessian"].view(np.uint64))
                           for a, b in zip(got, one)), "batch and loop differ"
                continue
            for key, x in (("eval_batch_wall_ms", (t1 - t0) * 1e3), ("eval_batch_dev_ms", dev), ("eval_loop_wall_ms", (t3 - t2) * 1e3),
                           ("reg_batch_wall_ms", (t4 - t3) * 1e3)):
                acc[key].append(x)
        r = {k: _stats(x) for k, x in acc.items()}
        r.update(grid=[-(-int(kf_s.info["n_voxels"]) // 256), G],
                 loop_over_batch_wall=r["eval_loop_wall_ms"]["median"] / r["eval_batch_wall_ms"]["median"],
                 register_over_evaluate_wall=r["reg_batch_wall_ms"]["median"] / r["eval_batch_wall_ms"]["median"])
        out["shared"][f"G_{G}"] = r
    vm.destroy()
    # relocalisation on the room, 243 hypotheses
    room = BC.room_map(h.voxel_map)
    _, (q, qa), _ = BC.room()
    base = api.pose_hypothesis(BC.ROOM_TRUE, 0.05, 0.45, -0.35)
    offs = [(0.5 * BC.ROOM_SIDE * (i - 4), 0.5 * BC.ROOM_SIDE * (j - 4)) for i in range(9) for j in range(9)]
    hyp = api.pose_hypotheses(base, BC.ROOM_YAWS, offs)
    assert hyp.shape == (243, 4, 4)
    acc = {"relocalize_all_wall_ms": [], "relocalize_keep27_wall_ms": [], "score_wall_ms": []}
    same = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        full = api.relocalize(h, room, (q, qa), hyp)
        t1 = time.perf_counter()
        kept = api.relocalize(h, room, (q, qa), hyp, keep=27)
        t2 = time.perf_counter()
        sc = api.score_hypotheses(h, room, (q, qa), hyp)
        t3 = time.perf_counter()
        if rep == 0:
            rank = sc["order"].index(full["best"]) + 1 if full["best"] >= 0 else -1
            fb, kb = full["results"][full["best"]], kept["results"][kept["best"]]
            winners = {"all": [full["best"], fb["n_corr"], fb["rmse"]], "keep27": [kept["best"], kb["n_corr"], kb["rmse"]],
                       "apart_m": float(np.linalg.norm(fb["T"][:3, 3] - kb["T"][:3, 3])),
                       "all_from_truth_m": float(np.linalg.norm(fb["T"][:3, 3] - BC.ROOM_TRUE[:3, 3])),
                       "keep27_from_truth_m": float(np.linalg.norm(kb["T"][:3, 3] - BC.ROOM_TRUE[:3, 3]))}
            continue
        same.append(bool(kept["best"] == full["best"]))
        for key, x in (("relocalize_all_wall_ms", (t1 - t0) * 1e3), ("relocalize_keep27_wall_ms", (t2 - t1) * 1e3),
                       ("score_wall_ms", (t3 - t2) * 1e3)):
            acc[key].append(x)
    out["room_243"] = {k: _stats(x) for k, x in acc.items()}
    out["room_243"].update(winner_rank_in_scores=rank, keep27_names_the_same_winner=all(same), winners=winners, map_voxels=len(room),
                           scan_points=int(q.shape[0]))
    room.destroy()
    for k in (kf_s, kf_t):
        k.close()
    h.close()
    for name in ("--bench-this", "--bench-parent"):  # bench.py's headline lines of the same session, recorded as given
        path = _arg(name, None, str)
        if path and os.path.exists(path):
            lines = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
            out[name[2:].replace("-", "_")] = [{k: ln[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")}
                                               for ln in lines]
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "vmap_eval_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
