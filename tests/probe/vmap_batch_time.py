"""Time of the grouped map registration (qtr_voxel_map_register_batch) against the route it replaces — G sequential
qtr_voxel_map_register_keyframe calls on the same slot — the two alternating inside every repetition of ONE run on one
MI355X (--reps repetitions, at least 10, after one warm-up repetition; every figure as median, min and max with its count n):
  G:          1, 8 and 64 hypotheses.
  shared:     ONE keyframe (the source scan of synth.kitti64_pair_16k(0), about 16 k voxels) under G guesses around the pair's
              transform, against a map of the target scan's keyframe.
  distinct:   64 keyframe OBJECTS against a map of the six-scan trajectory (synth.kitti64_trajectory(0, n_scans=6), scans 0 - 5
              under the scene's poses).  The trajectory has seven scans (six and the revisit): the 64 keyframes are made of them
              in turn, so their contents repeat every seven while their device arrays are 64 different allocations.
  loop:       the default 30 iterations and the default epsilons.
  QTR_ICP_BLOCK: unset and 4, on two handles of the same process (a handle reads the variable when it is made).
  wall_ms:    time.perf_counter around the call(s).  event_ms: events on the slot's stream around them.
  dev_ms:     what the library's own events report: QTR_VMAP_BATCH_TIMES of the batch ([before the loop, the loop]), and the sum
              over the G single calls of QTR_DBG_ICP_TIMES.
  grid:       the launch grid of one iteration, (chunks of the largest item, G) for the batch and (chunks,) per single call.
  batch_faster_in: in how many repetitions the batch's wall time was below the loop's.
Both routes must give the same bits (asserted once per configuration).
Not measured here: a map near its capacity; several slots batching at once; more than 64 items (chunks of 64 in a Python
loop); the composite benchmark (bench.py), whose kernels this code does not touch.
Prints one JSON line and writes it to profiles/vmap_batch_time.json (--out PATH: elsewhere)."""
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


def _handle(block):
    from quatro_amd import lib as ql
    keep = os.environ.pop("QTR_ICP_BLOCK", None)
    if block:
        os.environ["QTR_ICP_BLOCK"] = str(block)
    try:
        return ql.Handle(0)
    finally:
        os.environ.pop("QTR_ICP_BLOCK", None)
        if keep is not None:
            os.environ["QTR_ICP_BLOCK"] = keep


def _offset(k):
    import icp_restate as R
    rng = np.random.default_rng(900 + k)
    return R.rigid(R.rot(*rng.uniform(-0.01, 0.01, 3)), rng.uniform(-0.15, 0.15, 3))


def main():
    import torch
    from quatro_amd import lib as ql
    from quatro_amd import synth
    reps = max(_arg("--reps", 10), 10)
    fp = ql.default_frontend_params()
    src, tgt, Tgt = synth.kitti64_pair_16k(0)
    scans, gt = synth.kitti64_trajectory(0, n_scans=6)
    out = {"reps": reps, "max_iterations": 30}
    for block in (0, 4):
        h = _handle(block)
        st = torch.cuda.ExternalStream(h.stream_ptr(0))
        kf_s, kf_t = h.keyframe(src, fp), h.keyframe(tgt, fp)
        shared_map = h.voxel_map(1.0, 1 << 16)
        shared_map.insert_keyframe(kf_t, None)
        base = [h.keyframe(s, fp) for s in scans[:6]]
        traj_map = h.voxel_map(1.0, 1 << 17)
        for k in range(6):
            traj_map.insert_keyframe(base[k], gt[k])
        many = [h.keyframe(scans[j % 7], fp) for j in range(64)]
        configs = {"shared": (shared_map, [(kf_s, np.asarray(Tgt) @ _offset(j)) for j in range(64)]),
                   "distinct": (traj_map, [(many[j], np.asarray(gt[j % 7]) @ _offset(100 + j)) for j in range(64)])}
        res = {}
        for name, (vm, all_items) in configs.items():
            res[name] = {"map_voxels": len(vm)}
            for G in (1, 8, 64):
                items = all_items[:G]
                chunks = [-(-int(kf.info["n_voxels"]) // 256) for kf, _ in items]
                acc = {k: [] for k in ("batch_wall_ms", "batch_event_ms", "batch_dev_before_ms", "batch_dev_loop_ms", "loop_wall_ms",
                                       "loop_event_ms", "loop_dev_ms")}
                wins, iters = 0, None
                for rep in range(reps + 1):  # (the first repetition is the warm-up: the arena, code objects)
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    e[0].record(st)
                    t0 = time.perf_counter()
                    got = vm.register_batch(items)
                    t1 = time.perf_counter()
                    e[1].record(st)
                    dev = vm.batch_fetch(0, ql.VMAP_BATCH_TIMES)
                    e[2].record(st)
                    t2 = time.perf_counter()
                    one, dev_loop = [], 0.0
                    for kf, g in items:
                        one.append(vm.register_keyframe(kf, g))
                        dev_loop += float(h.debug_fetch(ql.DBG_ICP_TIMES, np.float32).sum())
                    t3 = time.perf_counter()
                    e[3].record(st)
                    e[3].synchronize()
                    if rep == 0:
                        assert all(np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)) and a["iterations"] == b["iterations"]
                                   for a, b in zip(got, one)), "the two routes differ"
                        iters = [r["iterations"] for r in got]
                        continue
                    bw, lw = (t1 - t0) * 1e3, (t3 - t2) * 1e3
                    wins += int(bw < lw)
                    for key, x in (("batch_wall_ms", bw), ("batch_event_ms", float(e[0].elapsed_time(e[1]))),
                                   ("batch_dev_before_ms", float(dev[0])), ("batch_dev_loop_ms", float(dev[1])), ("loop_wall_ms", lw),
                                   ("loop_event_ms", float(e[2].elapsed_time(e[3]))), ("loop_dev_ms", dev_loop)):
                        acc[key].append(x)
                r = {k: _stats(x) for k, x in acc.items()}
                r.update(grid_batch=[max(chunks), G], grid_single=sorted(set(chunks)), iterations=iters, batch_faster_in=[wins, reps],
                         loop_over_batch_wall=r["loop_wall_ms"]["median"] / r["batch_wall_ms"]["median"])
                res[name][f"G_{G}"] = r
        out["icp_block_%d" % block if block else "icp_block_unset"] = res
        for k in [kf_s, kf_t] + base + many:
            k.close()
        shared_map.destroy()
        traj_map.destroy()
        h.close()
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "vmap_batch_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
