"""Time of sweep deskew (qtr_deskew / qtr_keyframe_create_deskewed) on one raw KITTI-64-shaped sweep (kitti64_raw_scan(0),
115 200 points, skewed by a metre and 0.04 rad per sweep), the compared variants alternating inside every repetition of ONE
run on one handle (--reps repetitions, at least 10; every figure as median, min and max):
  deskew:    qtr_deskew from device memory into device memory at K = 2 and K = 50 knots (wall, and events on the slot's
             stream around the call), and from host memory to host memory at K = 2 (wall: two copies up, one down).
  keyframe:  qtr_keyframe_create on the sweep as it is (the parent commit's call), qtr_keyframe_create_deskewed at K = 2 and
             K = 50, and the route they replace — the deskew in numpy on the host (deskew_restate.model_deskew, vectorised
             float64) followed by qtr_keyframe_create — all from host memory (wall); the first two from device memory too.
Prints one JSON line and writes it to profiles/deskew_time.json (--out PATH: elsewhere)."""
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


def main():
    import torch
    import deskew_cases as K
    import deskew_restate as D
    from quatro_amd import lib as ql
    from quatro_amd import synth
    reps = max(_arg("--reps", 10), 10)
    scan, _ = synth.kitti64_raw_scan(0)
    M = K.pose(K.rot([0.1, -0.2, 1.0], 0.04), (1.0, 0.05, -0.02))
    kt2, kp2 = K.two_knots(M)
    kt50 = np.linspace(0.0, K.PERIOD, 50)
    kp50 = np.stack([D.model_pose_at(kt2, kp2, t) for t in kt50])  # the same motion sampled at 50 knots
    sweep, times = K.skew(scan, kt2, kp2)
    h = ql.Handle(0)
    fp = ql.default_frontend_params(seed=0)
    st = torch.cuda.ExternalStream(h.stream_ptr(0))
    d_sweep, d_times = torch.from_numpy(sweep).cuda(), torch.from_numpy(times).cuda()
    d_out = torch.empty_like(d_sweep)

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e3

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        out, w = wall(fn)
        e1.record(st)
        e1.synchronize()
        return out, w, float(e0.elapsed_time(e1))

    def numpy_route():
        q = sweep.copy()
        q[:, :3] = D.model_deskew(sweep, times, kt2, kp2, 0.0).astype(np.float32)
        return h.keyframe(q, fp)

    def kf(**kw):
        return lambda: h.keyframe(sweep, fp, **kw)

    def kf_dev(**kw):
        return lambda: h.keyframe(d_sweep, fp, **kw)
    names = ("deskew_device_K2", "deskew_device_K50", "deskew_host_K2", "keyframe_plain_host", "keyframe_deskewed_host_K2",
             "keyframe_deskewed_host_K50", "numpy_deskew_then_keyframe_host", "keyframe_plain_device", "keyframe_deskewed_device_K2")
    acc = {n + "_wall_ms": [] for n in names}
    acc.update({"deskew_device_K2_event_ms": [], "deskew_device_K50_event_ms": []})
    voxels = {}
    for rep in range(reps + 1):  # (the first repetition is the warm-up: staging, code objects)
        row = {}
        (_, i2), row["deskew_device_K2_wall_ms"], row["deskew_device_K2_event_ms"] = timed(
            lambda: h.deskew(d_sweep, d_times, kt2, kp2, 0.0, out=d_out))
        (_, i50), row["deskew_device_K50_wall_ms"], row["deskew_device_K50_event_ms"] = timed(
            lambda: h.deskew(d_sweep, d_times, kt50, kp50, 0.0, out=d_out))
        _, row["deskew_host_K2_wall_ms"] = wall(lambda: h.deskew(sweep, times, kt2, kp2, 0.0))
        assert i2["n_points"] == i50["n_points"] == sweep.shape[0] and i2["n_skipped"] == 0
        for name, fn in (("keyframe_plain_host", kf()),
                         ("keyframe_deskewed_host_K2", kf(times=times, knot_times=kt2, knot_poses=kp2)),
                         ("keyframe_deskewed_host_K50", kf(times=times, knot_times=kt50, knot_poses=kp50)),
                         ("numpy_deskew_then_keyframe_host", numpy_route),
                         ("keyframe_plain_device", kf_dev()),
                         ("keyframe_deskewed_device_K2", kf_dev(times=d_times, knot_times=kt2, knot_poses=kp2))):
            k, row[name + "_wall_ms"] = wall(fn)
            voxels[name] = int(k.info["n_voxels"])
            k.close()
        if rep:
            for key, x in row.items():
                acc[key].append(x)
    h.close()
    out = {"points": int(sweep.shape[0]), "keyframe_voxels": voxels, **{k: _stats(v) for k, v in acc.items()}}
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "deskew_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
