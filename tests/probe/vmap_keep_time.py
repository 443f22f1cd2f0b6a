"""Time of the voxel map's upkeep (qtr_voxel_map_evict / qtr_voxel_map_restore), the compared variants alternating inside
every repetition of ONE run on one handle (--reps repetitions, at least 10; every figure as median, min and max):
  evict:     maps of a lattice ball of voxels plus a two-voxel shell around it, restored from host sections, in a
             default-capacity table (1 << 20 voxels, 2^21 slots) and in a 1 << 17-slot table (capacity 1 << 16), at two
             sizes: the window keeps 2109 and 50 883 voxels (radius 8 and 23) and rejects the shell.  Per variant and repetition: the restore
             (wall), the eviction that rejects the shell (wall, and events on the slot's stream around the call), then the
             same window again, which rejects nothing (wall and events): one pass over the keys and one read-back.
  odometry:  api.scan_to_map_odometry over kitti64_trajectory(0)'s first 11 scans (keyframes made before), wall per scan,
             without a window and with window_radius = 25 m.
  load:      Handle.load_voxel_map of the file VoxelMap.save wrote for api.build_map's map of those 11 keyframes under
             the scene's own poses, against that build_map (both wall).
  parent:    tests/probe/vmap_time.py's iteration and insert figures re-measured in this run (their kernels are untouched).
Prints one JSON line and writes it to profiles/vmap_keep_time.json (--out PATH: elsewhere)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def _ball(r_keep, shell=2):
    """Sections of every lattice voxel within r_keep + shell of the origin: (coords, count, sums, how many lie within r_keep)."""
    r = r_keep + shell
    g = np.arange(-r, r + 1)
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    d2 = (c.astype(np.int64) ** 2).sum(axis=1)
    c = np.ascontiguousarray(c[d2 <= r * r], dtype=np.int32)
    rng = np.random.default_rng(r)
    count = rng.integers(1, 9, c.shape[0]).astype(np.int32)
    sums = np.zeros((c.shape[0], 9))
    sums[:, :3] = (c + 0.5) * count[:, None]
    sums[:, 3], sums[:, 6], sums[:, 8] = count * 0.2, count * 0.3, count * 0.5
    return c, count, sums, int((d2 <= r_keep * r_keep).sum())


def evict(ql, torch, reps):
    h = ql.Handle(0)
    st = torch.cuda.ExternalStream(h.stream_ptr(0))
    variants = []
    for r_keep in (8, 23):
        c, k, s, n_keep = _ball(r_keep)
        for cap in (1 << 20, 1 << 16):
            variants.append({"name": f"keep_{n_keep}_of_{c.shape[0]}_slots_{2 * cap}", "map": h.voxel_map(1.0, cap), "c": c, "k": k,
                             "s": s, "radius": float(r_keep), "n_keep": n_keep,
                             "acc": {x: [] for x in ("restore_wall_ms", "evict_wall_ms", "evict_event_ms", "nothing_wall_ms",
                                                     "nothing_event_ms")}})

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(st)
        e1.synchronize()
        return out, wall, float(e0.elapsed_time(e1))

    out = {}
    for rep in range(reps + 1):  # (the first repetition is the warm-up: staging, code objects)
        for v in variants:
            m = v["map"]
            m.clear()
            t0 = time.perf_counter()
            m.restore(v["c"], v["k"], v["s"])
            t_restore = (time.perf_counter() - t0) * 1e3
            a, wall_a, ev_a = timed(lambda: m.evict((0.5, 0.5, 0.5), v["radius"]))
            b, wall_b, ev_b = timed(lambda: m.evict((0.5, 0.5, 0.5), v["radius"]))
            assert a["n_kept"] == v["n_keep"] and a["n_evicted"] == v["c"].shape[0] - v["n_keep"] and b["n_evicted"] == 0
            if rep:
                for key, x in (("restore_wall_ms", t_restore), ("evict_wall_ms", wall_a), ("evict_event_ms", ev_a),
                               ("nothing_wall_ms", wall_b), ("nothing_event_ms", ev_b)):
                    v["acc"][key].append(x)
    for v in variants:
        out[v["name"]] = {"n_restored": int(v["c"].shape[0]), "n_kept": v["n_keep"], **{k: _stats(x) for k, x in v["acc"].items()}}
        v["map"].destroy()
    h.close()
    return out


def odometry_and_load(ql, reps):
    from quatro_amd import api, synth
    h = ql.Handle(0)
    scans, poses = synth.kitti64_trajectory(0)
    fp = ql.default_frontend_params(seed=0)
    kfs = [h.keyframe(s, fp) for s in scans[:11]]
    rel = np.stack([np.linalg.inv(poses[0]) @ p for p in poses[:11]])
    acc = {"odometry_per_scan_ms": [], "windowed_odometry_per_scan_ms": [], "build_map_ms": [], "load_voxel_map_ms": [],
           "save_ms": []}
    last = {}
    path = os.path.join(tempfile.mkdtemp(prefix="vmap_keep_"), "map.npz")
    for rep in range(reps + 1):  # (the first repetition is the warm-up)
        t0 = time.perf_counter()
        p0, m0 = api.scan_to_map_odometry(h, kfs, fp, 1.0, capacity=1 << 16)
        t1 = time.perf_counter()
        p1, m1 = api.scan_to_map_odometry(h, kfs, fp, 1.0, capacity=1 << 16, window_radius=25.0)
        t2 = time.perf_counter()
        bm = api.build_map(h, kfs, rel, 1.0, 1 << 16)
        t3 = time.perf_counter()
        bm.save(path)
        t4 = time.perf_counter()
        lm = h.load_voxel_map(path)
        t5 = time.perf_counter()
        if rep:
            for k, v in (("odometry_per_scan_ms", (t1 - t0) / 11), ("windowed_odometry_per_scan_ms", (t2 - t1) / 11),
                         ("build_map_ms", t3 - t2), ("save_ms", t4 - t3), ("load_voxel_map_ms", t5 - t4)):
                acc[k].append(v * 1e3)
        last = {"scans": 11, "odometry_voxels": len(m0), "windowed_odometry_voxels": len(m1), "build_map_voxels": len(bm),
                "loaded_voxels": len(lm), "pose_difference_max": float(np.abs(p0 - p1).max())}
        for m in (m0, m1, bm, lm):
            m.destroy()
    out = dict(last)
    out.update({k: _stats(v) for k, v in acc.items()})
    for k in kfs:
        k.close()
    h.close()
    return out


def main():
    import torch
    from quatro_amd import lib as ql
    import vmap_time
    reps = max(_arg("--reps", 10), 10)
    out = {"evict": evict(ql, torch, reps), "odometry_and_load": odometry_and_load(ql, reps),
           "parent": {"iteration": vmap_time.iteration_and_insert(ql, torch, reps)}}
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "vmap_keep_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
