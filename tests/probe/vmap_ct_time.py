"""Device time of the continuous-time registration beside the rigid map registration at the same n, the two alternating
inside every repetition of ONE run on one handle (--reps repetitions, at least 10; every figure as median, min and max):
a sweep of kitti64_trajectory(0) with one revolution of azimuth times, sampled at the odometry's leaf (api.sample_sweep at
fp.voxel_size) with the normals of Handle.fpfh, against a map of the scan before it; both from the same guess.
  iteration: a fixed-count run of 30 updates (both epsilons 0), hipEvent based: QTR_DBG_ICP_TIMES[1] / iterations of
             VoxelMap.register_ct (k_vmap_iter_ct) and of VoxelMap.register (k_vmap_iter), and QTR_DBG_ICP_TIMES[0], what
             precedes the loop (for register_ct the census launch is inside);
  call:      the wall time of the whole call with the default stopping rules, device-resident inputs.
Prints one JSON line and writes it to profiles/vmap_ct_time.json (--out PATH: elsewhere)."""
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
    import deskew_cases as DC
    from quatro_amd import api, synth
    from quatro_amd import lib as ql
    reps = max(_arg("--reps", 10), 10)
    h = ql.Handle(0)
    scans, poses = synth.kitti64_trajectory(0, n_scans=3)
    fp = ql.default_frontend_params(seed=0)
    kf = h.keyframe(scans[0], fp)
    vm = h.voxel_map(1.0, 1 << 16)
    vm.insert_keyframe(kf)
    period = DC.PERIOD
    # scan 1 as a sweep: it begins at the scan's own pose and the sensor moves on to the next scan's pose while it turns
    begin = np.linalg.inv(poses[0]) @ poses[1]
    motion = np.linalg.inv(poses[1]) @ poses[2]
    raw, times = DC.skew(scans[1], *DC.two_knots(motion, period), period)
    pts, ts = api.sample_sweep(raw, times, fp.voxel_size)
    nrm, _ = h.fpfh(pts, fp.normal_radius, fp.fpfh_radius)
    guess = begin @ begin  # (the constant-velocity end: the motion of the step before, once more)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pts, nrm, ts)]

    def prm(fixed):
        kw = dict(max_iterations=30, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0) if fixed else {}
        return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)

    variants = (("register_ct", lambda p: vm.register_ct(d[0], d[1], d[2], 0.0, period, begin, guess, p)),
                ("register", lambda p: vm.register(d[0], d[1], guess, p)))
    for _, run in variants:  # (warm-up: arenas, code objects)
        run(prm(True))
        run(prm(False))
    acc = {name: {"per": [], "before": [], "wall": []} for name, _ in variants}
    last = {}
    for _ in range(reps):
        for name, run in variants:
            g = run(prm(True))
            tm = h.debug_fetch(ql.DBG_ICP_TIMES, np.float32)
            acc[name]["per"].append(float(tm[1]) / max(g["iterations"], 1) * 1e3)
            acc[name]["before"].append(float(tm[0]) * 1e3)
            t0 = time.perf_counter()
            last[name] = run(prm(False))
            acc[name]["wall"].append((time.perf_counter() - t0) * 1e3)
    out = {"n_sweep": int(scans[1].shape[0]), "n_src": int(pts.shape[0]), "leaf": float(fp.voxel_size), "map_voxels": len(vm)}
    for name, _ in variants:
        g = last[name]
        out[name] = {"per_iteration_us": _stats(acc[name]["per"]), "before_the_loop_us": _stats(acc[name]["before"]),
                     "call_wall_ms": _stats(acc[name]["wall"]), "iterations": g["iterations"], "n_corr": g["n_corr"],
                     "stop_reason": g["stop_reason"]}
    out["register_ct"]["info"] = last["register_ct"]["info"]
    for name, T in (("guess", guess), ("register_ct", last["register_ct"]["T"])):  # against the sweep's true end pose
        dT = np.linalg.inv(begin @ motion) @ T
        out["end_pose_error_" + name] = {"m": float(np.linalg.norm(dT[:3, 3])),
                                         "deg": float(np.degrees(np.arccos(np.clip((np.trace(dT[:3, :3]) - 1) / 2, -1, 1))))}
    out["iteration_ratio"] = out["register_ct"]["per_iteration_us"]["median"] / out["register"]["per_iteration_us"]["median"]
    out["call_ratio"] = out["register_ct"]["call_wall_ms"]["median"] / out["register"]["call_wall_ms"]["median"]
    vm.destroy()
    kf.close()
    h.close()
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "vmap_ct_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
