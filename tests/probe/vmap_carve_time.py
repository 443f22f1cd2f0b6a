"""Time of the voxel map's visibility carving (qtr_voxel_map_carve_keyframes) against the route it replaces — fetch the map's
sections, decide on the host with the numpy restatement, clear and restore — the two alternating inside every repetition of
ONE run on one handle (--reps repetitions, at least 10; every figure as median, min and max with its count n, wall milliseconds; the host route with 64
keyframes in the first three repetitions only):
  maps:      the eight-scan map of the quality test (tests/vmap_carve_cases.moving_box_scans without vegetation, raw sweeps
             with their ground, 0.5 m voxels, about 20 k voxels) and a map of 50 000 voxels in an annulus of 3 .. 60 m, both
             in default-capacity tables (2^21 slots).  Before every timed call the map is cleared and restored from its saved
             sections (not timed).
  scans:     1, 8 and 64 keyframes (the keyframes of those eight raw sweeps at the front end's defaults, cycled, under the
             scene's own poses), default image (64 x 1024), window 2, min_votes 1 / 2 / 8.  The host route is given the keyframes' clouds, fetched once
             and not timed: it pays for the map's sections, the restatement and the restore only.
  parts:     of the device call, from events on the slot's stream around it; and the same call again, which carves nothing.
Not measured here: the mark pass over a compacted list of live slots instead of the whole table; images other than the
default; the composite benchmark (bench.py), whose kernels this code does not touch.
--composite-parent X1,X2,... --composite-this Y1,Y2,... copy into the output the benchmark's composite figures (registrations/s)
of the parent commit and of this one, every run of each: the probe does not measure them, the caller does, alternating the
two in the session that runs the probe (bench.py --gpus 1 --steps 40 --warmup 5).
Prints one JSON line and writes it to profiles/vmap_carve_time.json (--out PATH: elsewhere)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def main():
    import torch
    from quatro_amd import lib as ql
    import vmap_carve_cases as CC
    import vmap_carve_restate as CR
    import vmap_restate as M
    reps = max(_arg("--reps", 10), 10)
    h = ql.Handle(0)
    st = torch.cuda.ExternalStream(h.stream_ptr(0))
    raw, poses, _ = CC.moving_box_scans(False)
    fp = ql.default_frontend_params(seed=0)
    kfs = [h.keyframe(s, fp) for s in raw]
    clouds = [k.fetch(ql.KF_VOX) for k in kfs]

    def saved(fill):
        m = h.voxel_map(0.5, 1 << 20)
        fill(m)
        sec = {k: m.fetch(k) for k in (M.COORDS, M.COUNT, M.SUMS)}
        return m, sec

    def eight_scan(m):
        up = np.zeros((max(s.shape[0] for s in raw), 4), np.float32)
        up[:, 2] = 1.0
        for s, P in zip(raw, poses):
            m.insert(s, up[:s.shape[0]], P)

    def annulus(m):
        m.insert(*CC.random_map_cloud(50000, 0.5, seed=50, r_hi=60.0))

    composite = {k: [float(x) for x in _arg("--composite-" + k, "", str).split(",") if x] for k in ("parent", "this")}
    out = {"reps": reps, "composite_registrations_per_s": composite, "keyframe_voxels": [int(c.shape[0]) for c in clouds]}
    for name, fill in (("eight_scan_map", eight_scan), ("map_50k", annulus)):
        m, sec = saved(fill)
        res = {"n_voxels": int(sec[M.COUNT].shape[0])}
        for B, votes in ((1, 1), (8, 2), (64, 8)):
            idx = [b % 8 for b in range(B)]
            kk, PP, cc = [kfs[i] for i in idx], poses[idx], [clouds[i] for i in idx]
            p = CR.Params(min_votes=votes)
            prm = p.to_lib()
            acc = {x: [] for x in ("device_wall_ms", "device_event_ms", "device_nothing_wall_ms", "host_route_wall_ms",
                                   "host_fetch_ms", "host_decide_ms", "host_restore_ms")}
            info = None
            for rep in range(reps + 1):  # (the first repetition is the warm-up: images, staging, code objects)
                m.clear()
                m.restore(sec[M.COORDS], sec[M.COUNT], sec[M.SUMS])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                t0 = time.perf_counter()
                info = m.carve_keyframes(kk, PP, prm)
                t1 = time.perf_counter()
                e1.record(st)
                e1.synchronize()
                t2 = time.perf_counter()
                again = m.carve_keyframes(kk, PP, prm)
                t3 = time.perf_counter()
                assert again["n_carved"] == 0
                if rep:
                    acc["device_wall_ms"].append((t1 - t0) * 1e3)
                    acc["device_nothing_wall_ms"].append((t3 - t2) * 1e3)
                    acc["device_event_ms"].append(float(e0.elapsed_time(e1)))
                if B == 64 and rep > 3:  # (the restatement of 64 scans takes seconds: three timed repetitions of the host route)
                    continue
                m.clear()
                m.restore(sec[M.COORDS], sec[M.COUNT], sec[M.SUMS])
                t4 = time.perf_counter()
                f = {k: m.fetch(k) for k in (M.COORDS, M.COUNT, M.SUMS, M.RECORDS)}
                t5 = time.perf_counter()
                c = CR.cfg_make(p, B, 0.5)
                v = CR.carve_votes(c, cc, PP, f[M.RECORDS][:, :3])
                gone = (v == CR.SEEN_THROUGH).sum(axis=1) >= c.min_votes
                t6 = time.perf_counter()
                if gone.any():
                    m.clear()
                    m.restore(f[M.COORDS][~gone], f[M.COUNT][~gone], f[M.SUMS][~gone])
                t7 = time.perf_counter()
                assert int(gone.sum()) == info["n_carved"] and len(m) == info["n_kept"]
                if rep:
                    for key, x in (("host_route_wall_ms", t7 - t4), ("host_fetch_ms", t5 - t4), ("host_decide_ms", t6 - t5),
                                   ("host_restore_ms", t7 - t6)):
                        acc[key].append(x * 1e3)
            res[f"keyframes_{B}"] = {"min_votes": votes, **info, **{k: _stats(x) for k, x in acc.items()}}
        out[name] = res
        m.destroy()
    for k in kfs:
        k.close()
    h.close()
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "vmap_carve_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
