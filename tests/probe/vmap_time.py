"""Device time of the voxel map beside the routes that existed before it, the compared variants alternating inside every
repetition of ONE run on one handle (--reps repetitions, at least 10; every figure as median, min and max):
  iteration: kitti64_pair_16k(0), target tilted by roll 1.5 deg / pitch -1.0 deg, from the registration's result: one
             iteration of a fixed-count run of 30 updates (hipEvent based, QTR_DBG_ICP_TIMES[1] / iterations) of
             qtr_voxel_map_register against a map of the target (hash lookup) and of qtr_gicp method 3 on the same clouds
             (dense cell table), plus what precedes the loop in each (QTR_DBG_ICP_TIMES[0]: for method 3 the box, the
             read-back, the counting sort and the voxel records; for the map only the state's initialisation);
  insert:    qtr_voxel_map_insert_keyframe of that pair's ~16 k-voxel target keyframe into an empty map and into a map that
             already holds every voxel it touches: events on the slot's stream around the call (the call's one host wait
             between its two launch groups is inside) and the call's wall time;
  build_map: api.build_map over kitti64_trajectory(0)'s 11 scans under the scene's own poses, against
             Handle.merge_keyframes of the same members (the only route before), and a registration of the revisit scan
             against each: VoxelMap.register_keyframe and qtr_gicp method 3 against the merged keyframe's voxels.
Prints one JSON line and writes it to profiles/vmap_time.json (--out PATH: elsewhere)."""
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


def _vg(ql, **kw):
    return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)


def iteration_and_insert(ql, torch, reps):
    import icp_restate as R
    from quatro_amd import synth
    h = ql.Handle(0)
    s, t, Tgt = synth.kitti64_pair_16k(0)
    tilt = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
    t, Tgt = R.apply(tilt, t), tilt @ Tgt
    fp = ql.default_frontend_params(seed=0)
    r = h.register_pair(s, t, fp)
    ks, kt = h.keyframe(s, fp), h.keyframe(t, fp)
    vs, ns, vt, nt = ks.fetch(ql.KF_VOX), ks.fetch(ql.KF_NORMALS), kt.fetch(ql.KF_VOX), kt.fetch(ql.KF_NORMALS)
    d = [torch.from_numpy(x).cuda() for x in (vs, ns, vt, nt)]
    vm = h.voxel_map(1.0, 1 << 16)
    vm.insert_keyframe(kt)
    fixed = _vg(ql, max_iterations=30, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0)
    variants = (("map_register", lambda: vm.register(d[0], d[1], r["T"], fixed)),
                ("method_3", lambda: h.gicp(d[0], d[2], d[1], d[3], r["T"], fixed)))
    for _, run in variants:  # (warm-up: arenas, code objects)
        run()
    acc = {name: {"per": [], "before": []} for name, _ in variants}
    last = {}
    for _ in range(reps):
        for name, run in variants:
            g = run()
            tm = h.debug_fetch(ql.DBG_ICP_TIMES, np.float32)
            acc[name]["per"].append(float(tm[1]) / max(g["iterations"], 1) * 1e3)
            acc[name]["before"].append(float(tm[0]) * 1e3)
            last[name] = g
    out = {"n_src": int(vs.shape[0]), "n_tgt": int(vt.shape[0]), "map_voxels": len(vm)}
    for name, _ in variants:
        g = last[name]
        out[name] = {"per_iteration_us": _stats(acc[name]["per"]), "before_the_loop_us": _stats(acc[name]["before"]),
                     "iterations": g["iterations"], "n_corr": g["n_corr"], "rot_err_deg": R.rot_err_deg(g["T"], Tgt)}
    # insert: events on the slot's own stream around the call
    st = torch.cuda.ExternalStream(h.stream_ptr(0))
    fresh, again = h.voxel_map(1.0, 1 << 16), vm
    ins = {"into_empty_map": {"event_ms": [], "wall_ms": []}, "into_existing_voxels": {"event_ms": [], "wall_ms": []}}
    info = {}
    for rep in range(reps + 1):  # (the first repetition is the warm-up: the map's insert scratch)
        for name, m in (("into_empty_map", fresh), ("into_existing_voxels", again)):
            if name == "into_empty_map":
                m.clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            t0 = time.perf_counter()
            info[name] = m.insert_keyframe(kt)
            wall = (time.perf_counter() - t0) * 1e3
            e1.record(st)
            e1.synchronize()
            if rep:
                ins[name]["event_ms"].append(float(e0.elapsed_time(e1)))
                ins[name]["wall_ms"].append(wall)
    out["insert"] = {name: {"event_ms": _stats(v["event_ms"]), "wall_ms": _stats(v["wall_ms"]), **info[name]}
                     for name, v in ins.items()}
    for m in (fresh, vm):
        m.destroy()
    for k in (ks, kt):
        k.close()
    h.close()
    return out


def build_map(ql, reps):
    from quatro_amd import api, synth
    h = ql.Handle(0)
    scans, poses = synth.kitti64_trajectory(0)
    fp = ql.default_frontend_params(seed=0)
    kfs = [h.keyframe(s, fp) for s in scans]
    members, query = kfs[:11], kfs[11]
    rel = np.stack([np.linalg.inv(poses[0]) @ p for p in poses])
    guess = rel[11]
    qv, qn = query.fetch(ql.KF_VOX), query.fetch(ql.KF_NORMALS)
    out = {"members": 11, "member_voxels": [int(k.info["n_voxels"]) for k in members]}
    acc = {"build_map_ms": [], "merge_keyframes_ms": [], "map_register_ms": [], "merged_method_3_ms": []}
    last = {}
    for rep in range(reps + 1):  # (the first repetition is the warm-up)
        t0 = time.perf_counter()
        vm = api.build_map(h, members, rel[:11], 1.0)
        t1 = time.perf_counter()
        a = vm.register_keyframe(query, guess)
        t2 = time.perf_counter()
        merged = h.merge_keyframes(members, rel[:11], fp)
        t3 = time.perf_counter()
        mv, mn = merged.fetch(ql.KF_VOX), merged.fetch(ql.KF_NORMALS)
        t4 = time.perf_counter()
        b = h.gicp(qv, mv, qn, mn, guess, _vg(ql))
        t5 = time.perf_counter()
        if rep:
            for k, v in (("build_map_ms", t1 - t0), ("map_register_ms", t2 - t1), ("merge_keyframes_ms", t3 - t2),
                         ("merged_method_3_ms", t5 - t4)):
                acc[k].append(v * 1e3)
        last = {"map_voxels": len(vm), "map_members": vm.info()["n_members"], "merged_voxels": int(merged.info["n_voxels"]),
                "map_register": {k: a[k] for k in ("iterations", "n_corr", "stop_reason")},
                "merged_method_3": {k: b[k] for k in ("iterations", "n_corr", "stop_reason")},
                "T_difference_max": float(np.abs(a["T"] - b["T"]).max())}
        vm.destroy()
        merged.close()
    out.update(last)
    out.update({k: _stats(v) for k, v in acc.items()})
    for k in kfs:
        k.close()
    h.close()
    return out


def main():
    import torch
    from quatro_amd import lib as ql
    reps = max(_arg("--reps", 10), 10)
    out = {"iteration": iteration_and_insert(ql, torch, reps), "build_map": build_map(ql, reps)}
    print(json.dumps(out))
    default = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "vmap_time.json"))
    path = _arg("--out", default, str)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
