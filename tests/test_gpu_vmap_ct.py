"""The continuous-time registration on the MI355X (qtr_voxel_map_register_ct, libquatro_ext.so): the device equal to the host
restatement (tests/vmap_ct_ref/vmap_ct_ref.cpp) as raw records at the chunk edges, from host and device memory; the anchor —
all times at t_end IS VoxelMap.register, bit for bit —; skipped and extrapolated points, the stops, two slots at once; every
refusal with its code; the accuracy scenes of tests/test_vmap_ct_cpu.py as equal records; the C++ demo.  Everything goes
through the C ABI (quatro_amd.lib)."""
import os
import subprocess
import threading

import numpy as np
import pytest

import icp_restate as R
import vmap_ct_cases as K
import vmap_ct_restate as CT
import vmap_restate as M

pytestmark = pytest.mark.gpu

ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same_icp(a, b, what=""):
    assert a.get("status", 0) == b.get("status", 0), what
    assert np.array_equal(_bits(a["T"]), _bits(b["T"])), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _vg(**kw):
    from quatro_amd import lib as ql
    return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)


def _debug(hip, slot=0):
    from quatro_amd import lib as ql
    return (hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64, slot).reshape(-1, 18), hip.debug_fetch(ql.DBG_ICP_CORR, np.int32, slot))


def _both(hip, vm, ref, s, sn, t, begin, guess, iters, what="", device=False, t_begin=K.T_BEGIN, t_end=K.T_END):
    """register_ct of `iters` iterations (both epsilons 0) on the device and in the restatement: the final record, the trace
    of every update, the last correspondence flags and the counts, bit for bit.  Returns the device result."""
    args = (s, sn, t)
    if device:
        import torch
        args = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in args)
    g = vm.register_ct(*args, t_begin, t_end, begin, guess,
                       _vg(max_iterations=iters, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0))
    trace, corr = _debug(hip)
    o = CT.register_ct(ref, s, sn, t, t_begin, t_end, begin, guess, teps=0.0, feps=0.0, max_iter=iters)
    _same_icp(g, o, what)
    assert g["info"] == o["info"], (what, g["info"], o["info"])
    assert trace.shape == o["trace"].shape and np.array_equal(_bits(trace), _bits(o["trace"])), what
    assert np.array_equal(corr, o["corr"]), what
    return g


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


@pytest.fixture(scope="module")
def maps(hip):
    pts, nrm, pose = K.small_map()
    vm, ref = hip.voxel_map(K.SIDE, 1 << 14), M.RefMap(K.SIDE, 1 << 14)
    assert vm.insert(pts, nrm, pose) == ref.insert(pts, nrm, pose)
    assert 100 < len(ref) < 1000
    yield vm, ref
    vm.destroy()


@pytest.mark.parametrize("n", K.SIZES)
def test_the_device_equals_the_restatement_as_raw_records(hip, maps, n):
    from quatro_amd import lib as ql
    vm, ref = maps
    s, sn, t, n_skip, n_extra = K.edge_cloud(n)
    if n == 0:  # (an empty cloud is not an error; an empty device tensor has no pointer to give, so host memory only)
        g = _both(hip, vm, ref, s, sn, t, K.BEGIN, K.GUESS_END, 6, "n = 0")
        assert not g["valid"] and g["stop_reason"] == ql.ICP_STOP_TOO_FEW and np.array_equal(g["T"], K.GUESS_END)
        assert g["info"] == {"n_points": 0, "n_skipped": 0, "n_extrapolated": 0}
        return
    for device in (False, True):
        g = _both(hip, vm, ref, s, sn, t, K.BEGIN, K.GUESS_END, 6, f"n = {n}, device memory {device}", device)
        assert g["info"] == {"n_points": n, "n_skipped": n_skip, "n_extrapolated": n_extra}
    if n >= 255:
        assert g["valid"] and g["iterations"] == 6
        # every iteration's record: the loop cut after k updates (max_iterations = 1 among them)
        for k in (1, 2, 3):
            assert _both(hip, vm, ref, s, sn, t, K.BEGIN, K.GUESS_END, k, f"n = {n}, {k} iterations")["iterations"] == k
    # guess_end = None is begin_pose
    a = vm.register_ct(s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, None, _vg(max_iterations=3))
    b = vm.register_ct(s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.BEGIN, _vg(max_iterations=3))
    _same_icp(a, b, "guess_end = None")
    # the default stopping rules too
    g = vm.register_ct(s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END)
    trace, corr = _debug(hip)
    o = CT.register_ct(ref, s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END)
    _same_icp(g, o, f"n = {n}, default epsilons")
    assert np.array_equal(_bits(trace), _bits(o["trace"])) and np.array_equal(corr, o["corr"])


@pytest.mark.parametrize("n", [1, 256, 513])
def test_all_times_at_t_end_is_the_handles_own_rigid_registration(hip, maps, n):
    vm, ref = maps
    s, sn, _, _, _ = K.edge_cloud(n)
    te = np.full(n, np.float32(K.T_END))
    for prm in (_vg(max_iterations=8, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0), _vg()):
        want = vm.register(s, sn, K.GUESS_END, prm)
        trace_w, corr_w = _debug(hip)
        for B in K.ANCHOR_BEGINS:
            got = vm.register_ct(s, sn, te, K.T_BEGIN, K.T_END, B, K.GUESS_END, prm)
            trace_g, corr_g = _debug(hip)
            _same_icp(got, want, f"anchor, n = {n}")
            assert trace_g.shape == trace_w.shape and np.array_equal(_bits(trace_g), _bits(trace_w))
            assert np.array_equal(corr_g, corr_w)
            assert got["info"]["n_extrapolated"] == 0


def test_edges_skips_extrapolations_stops_and_two_slots(hip, maps):
    from quatro_amd import lib as ql
    vm, ref = maps
    s, sn, t, n_skip, n_extra = K.edge_cloud(513)
    g = _both(hip, vm, ref, s, sn, t, K.BEGIN, K.GUESS_END, 6, "edges")
    _, corr = _debug(hip)
    named = K.named_times()
    for i, (tt, sk, ex) in enumerate(named):
        assert corr[i] == (-1 if sk else 0), (i, tt)  # NaN / inf time: skipped; outside the sweep: counted and still matched
    k = len(named)
    assert (corr[k:k + 4] == -1).all()  # NaN point, infinite point, zero normal, NaN normal
    assert g["info"] == {"n_points": 513, "n_skipped": n_skip, "n_extrapolated": n_extra} and (n_skip, n_extra) == (6, 5)
    # all points without a voxel
    away = s.copy()
    away[:, :3] += np.float32(500.0)
    e = _both(hip, vm, ref, away, sn, t, K.BEGIN, K.GUESS_END, 6, "no voxel anywhere")
    assert e["stop_reason"] == ql.ICP_STOP_TOO_FEW and not e["valid"] and e["n_corr"] == 0 and np.array_equal(e["T"], K.GUESS_END)
    assert (_debug(hip)[1] == -1).all()
    one = _both(hip, vm, ref, s, sn, t, K.BEGIN, K.GUESS_END, 1, "max_iterations = 1")
    assert one["iterations"] == 1 and one["stop_reason"] == ql.ICP_STOP_MAX_ITERATIONS
    # two slots against one map at once: each the single result
    s2, sn2, t2, _, _ = K.edge_cloud(257, seed=1)
    prm = _vg(max_iterations=6, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0)
    single = [vm.register_ct(s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, prm, slot=0),
              vm.register_ct(s2, sn2, t2, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, prm, slot=1)]
    out = [None, None]

    def run(j, args):
        out[j] = vm.register_ct(*args, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, prm, slot=j)

    for _ in range(3):
        th = [threading.Thread(target=run, args=(0, (s, sn, t))), threading.Thread(target=run, args=(1, (s2, sn2, t2)))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        for j in range(2):
            _same_icp(out[j], single[j], f"slot {j} beside the other")
            assert out[j]["info"] == single[j]["info"]
    o2 = CT.register_ct(ref, s2, sn2, t2, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, teps=0.0, feps=0.0, max_iter=6)
    _same_icp(single[1], o2, "slot 1")
    assert np.array_equal(_bits(_debug(hip, 1)[0]), _bits(o2["trace"]))


def test_refusals_leave_the_map_and_the_slot_usable(hip, maps):
    from quatro_amd import lib as ql
    vm, ref = maps
    s, sn, t, _, _ = K.edge_cloud(257)
    args = dict(cloud=s, normals=sn, times=t, t_begin=K.T_BEGIN, t_end=K.T_END, begin_pose=K.BEGIN, guess_end=K.GUESS_END)
    before = {k: vm.fetch(k) for k in (M.COORDS, M.COUNT, M.SUMS)}
    want = vm.register_ct(**args, icp=_vg(max_iterations=4))

    def refused(code, word, **kw):
        with pytest.raises(ql.QuatroHipError) as ei:
            vm.register_ct(**{**args, **kw})
        assert ei.value.code == code and word in str(ei.value), (kw.keys(), str(ei.value))

    other = ql.Handle(0)
    foreign = other.voxel_map(1.0, 64)
    try:
        stolen = ql.VoxelMap(hip, foreign._m.value)  # the other handle's map through this handle
        with pytest.raises(ql.QuatroHipError) as ei:
            stolen.register_ct(**args)
        assert ei.value.code == ql.QTR_ERR_BAD_ARG and "another handle" in str(ei.value)
        stolen._m = None  # (not this wrapper's to destroy)
    finally:
        foreign.destroy()
        other.close()
    for mth in (0, 1, 2):
        refused(ql.QTR_ERR_BAD_ARG, "QTR_ICP_VOXEL_PLANE_TO_PLANE", icp=ql.default_icp_params(method=mth))
    big = np.zeros((hip.limits.max_points + 1, 4), np.float32)
    refused(ql.QTR_ERR_CAPACITY, "max_points", cloud=big, normals=big, times=np.zeros(big.shape[0], np.float32))
    refused(ql.QTR_ERR_BAD_ARG, "normals", normals=None)
    for name, word in (("begin_pose", "begin pose"), ("guess_end", "guess")):
        for v in (np.nan, np.inf):
            bad = np.array(args[name])
            bad[1, 3] = v
            refused(ql.QTR_ERR_BAD_ARG, "non-finite", **{name: bad})
            assert word in hip.last_error()
    refused(ql.QTR_ERR_BAD_ARG, "begin_pose is NULL", begin_pose=None)
    for tb, te in ((K.T_END, K.T_BEGIN), (K.T_END, K.T_END), (np.nan, K.T_END), (K.T_BEGIN, np.inf), (-1e308, 1e308)):
        refused(ql.QTR_ERR_BAD_ARG, "t_begin", t_begin=tb, t_end=te)
    refused(ql.QTR_ERR_BAD_ARG, "pi / 2", guess_end=K.BEGIN @ R.rigid(R.rot(0.0, 0.0, np.radians(100.0)), [0.0, 0.0, 0.0]))
    # the C ABI itself: NULL arrays with n > 0, a negative n, NULL times, an unknown mem
    lib3, res, prm = ql.load_ext(), ql.IcpResult(), _vg()
    import ctypes as C
    B, G = np.ascontiguousarray(K.BEGIN.reshape(16)), np.ascontiguousarray(K.GUESS_END.reshape(16))

    def raw(pp, n, pn, pt, mem=ql.MEM_HOST):
        return lib3.qtr_voxel_map_register_ct(hip._h, 0, vm._m, pp, n, pn, pt, K.T_BEGIN, K.T_END, B.ctypes.data, G.ctypes.data,
                                              C.byref(prm), C.byref(res), mem, None)

    assert raw(None, 257, sn.ctypes.data, t.ctypes.data) == ql.QTR_ERR_BAD_ARG and res.status == ql.QTR_ERR_BAD_ARG
    assert raw(s.ctypes.data, -1, sn.ctypes.data, t.ctypes.data) == ql.QTR_ERR_BAD_ARG
    assert raw(s.ctypes.data, 257, sn.ctypes.data, None) == ql.QTR_ERR_BAD_ARG and "times" in hip.last_error()
    assert raw(s.ctypes.data, 257, sn.ctypes.data, t.ctypes.data, mem=7) == ql.QTR_ERR_BAD_ARG
    assert lib3.qtr_voxel_map_register_ct(hip._h, 9, vm._m, s.ctypes.data, 257, sn.ctypes.data, t.ctypes.data, K.T_BEGIN, K.T_END,
                                          B.ctypes.data, G.ctypes.data, C.byref(prm), C.byref(res), ql.MEM_HOST, None) == ql.QTR_ERR_BAD_ARG
    assert raw(s.ctypes.data, 257, sn.ctypes.data, t.ctypes.data) == ql.QTR_OK  # info may be NULL
    # the map is what it was and the slot registers as before
    after = {k: vm.fetch(k) for k in before}
    assert all(np.array_equal(_bits(before[k]), _bits(after[k])) for k in before)
    _same_icp(vm.register_ct(**args, icp=_vg(max_iterations=4)), want, "after the refusals")
    _same_icp(vm.register(s, sn, K.GUESS_END, _vg(max_iterations=4)), ref.register(s, sn, K.GUESS_END, max_iter=4), "rigid, after")


@pytest.mark.parametrize("case", K.ACC_CASES, ids=[c[0] for c in K.ACC_CASES])
def test_the_accuracy_scene_gives_the_restatements_record(hip, case):
    """The device record equals the restatement's, so the assertion of tests/test_vmap_ct_cpu.py on the end-pose errors carries
    over to the device."""
    sc = K.accuracy_scene(case)
    vm, ref = hip.voxel_map(1.0, 1 << 16), M.RefMap(1.0, 1 << 16)
    try:
        assert vm.insert(sc["world"], sc["world_normals"], None) == ref.insert(sc["world"], sc["world_normals"], None)
        B = sc["begin"]
        guess, want = B @ sc["guess_motion"], B @ sc["true_motion"]
        g = vm.register_ct(sc["raw"], sc["normals"], sc["times"], 0.0, K.PERIOD, B, guess)
        trace, corr = _debug(hip)
        o = CT.register_ct(ref, sc["raw"], sc["normals"], sc["times"], 0.0, K.PERIOD, B, guess)
        _same_icp(g, o, sc["name"])
        assert g["info"] == o["info"] and np.array_equal(_bits(trace), _bits(o["trace"])) and np.array_equal(corr, o["corr"])
        err, err0 = K.pose_error(g["T"], want), K.pose_error(guess, want)
        print(f"{sc['name']}: end-pose error {err[0]:.4f} m / {err[1]:.3f} deg from {err0[0]:.4f} m / {err0[1]:.3f} deg, "
              f"{g['iterations']} iterations, {g['n_corr']} correspondences")
        assert g["valid"] and g["converged"]
    finally:
        vm.destroy()


def test_continuous_time_odometry_runs_on_the_device_and_leaves_the_old_path_alone(hip):
    """scan_to_map_odometry(continuous_time=True) on four sweeps of kitti64_trajectory(0), each skewed with the scene's own
    motion (1 m per sweep): the chain B_k = E_{k-1} from E_0 = I, one insert per sweep, finite poses.  Only the structure is
    asserted; the errors against the scene's poses are printed beside those of the constant-velocity deskew (DESIGN.md
    section 22 says why the first sweep's motion stays in them: sweep 0 is taken as unmoved and every begin pose is fixed).
    continuous_time=False is the call without the argument, bit for bit."""
    import deskew_cases as DC
    from quatro_amd import api, synth
    from quatro_amd import lib as ql
    scans, gt = synth.kitti64_trajectory(0, n_scans=5)
    raw, times = [], []
    for k in range(4):
        s, t = DC.skew(scans[k], *DC.two_knots(np.linalg.inv(gt[k]) @ gt[k + 1]))
        raw.append(s)
        times.append(t)
    truth = [np.linalg.inv(gt[0]) @ g for g in gt[:4]]
    fp = ql.default_frontend_params()
    maps = []
    try:
        ct, vm = api.scan_to_map_odometry(hip, raw, fp, voxel_size=1.0, capacity=1 << 16, times=times, sweep_period=DC.PERIOD,
                                          continuous_time=True)
        maps.append(vm)
        assert ct.shape == (4, 4, 4) and np.isfinite(ct).all() and vm.info()["n_inserts"] == 4
        assert np.array_equal(ct[0], np.eye(4)) and np.array_equal(ct[1], np.eye(4))  # B_0 = I, B_1 = E_0 = I
        cv, vm1 = api.scan_to_map_odometry(hip, raw, fp, voxel_size=1.0, capacity=1 << 16, times=times, sweep_period=DC.PERIOD)
        maps.append(vm1)
        cv0, vm0 = api.scan_to_map_odometry(hip, raw, fp, voxel_size=1.0, capacity=1 << 16, times=times, sweep_period=DC.PERIOD,
                                            continuous_time=False)
        maps.append(vm0)
        assert np.array_equal(_bits(cv), _bits(cv0))
        for name, poses in (("continuous time", ct), ("constant-velocity deskew", cv)):
            steps = [float(np.linalg.norm((np.linalg.inv(poses[k]) @ poses[k + 1])[:3, 3])) for k in range(3)]
            errs = [float(np.linalg.norm(p[:3, 3] - t[:3, 3])) for p, t in zip(poses, truth)]
            print(f"odometry on skewed sweeps, {name}: start-pose error {['%.4f' % e for e in errs]} m, step lengths "
                  f"{['%.4f' % s for s in steps]} m (the scene's: 1 m)")
        with pytest.raises(ValueError):
            api.scan_to_map_odometry(hip, raw, fp, continuous_time=True)
    finally:
        for m in maps:
            m.destroy()


def test_cpp_voxelmap_ct_demo_prints_what_the_python_calls_return(hip, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "voxelmap_ct_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "voxelmap_ct_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    pts, nrm, pose = K.small_map()
    s, sn, t, _, _ = K.edge_cloud(200)
    t[:3] = [np.float32(K.T_END + 0.01), np.float32(K.T_BEGIN), np.float32(K.T_END)]
    t4 = np.zeros((200, 4), np.float32)
    t4[:, 0] = t
    args = [repr(K.SIDE)]
    for name, a in (("a", pts), ("an", nrm), ("pa", pose), ("q", s), ("qn", sn), ("qt", t4), ("tb", K.T_BEGIN), ("te", K.T_END),
                    ("b", K.BEGIN), ("g", K.GUESS_END)):
        if isinstance(a, float):
            args.append(repr(a))
            continue
        path = str(tmp_path / name)
        if a.shape == (4, 4):
            np.savetxt(path, a, fmt="%.17g")
        else:
            synth.save_kitti_bin(path, a)
        args.append(path)
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    vm = hip.voxel_map(K.SIDE, 1 << 16)
    try:
        i = vm.insert(pts, nrm, pose)
        r = vm.register_ct(s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END)
        assert out[0] == f"insert: points {i['n_points']} members {i['n_members']} new {i['n_new_voxels']} touched {i['n_touched_voxels']}", out[0]
        assert out[1] == f"sweep: points 200 skipped {r['info']['n_skipped']} extrapolated {r['info']['n_extrapolated']}", out[1]
        assert r["info"]["n_extrapolated"] == 1
        assert out[2] == f"iterations {r['iterations']} stop {r['stop_reason']} corr {r['n_corr']} valid {int(r['valid'])}", out[2]
        words = np.array([int(x, 16) for ln in out[3:12] for x in ln.split()], dtype=np.uint64).view(np.float64)
        assert np.array_equal(_bits(words[:16]), _bits(r["T"].reshape(16)))
        assert _f64bits(words[16]) == _f64bits(r["fitness"]) and _f64bits(words[17]) == _f64bits(r["rmse"])
        mid = ql.ct_pose_at(K.T_BEGIN, K.T_END, K.BEGIN, r["T"], 0.5 * (K.T_BEGIN + K.T_END))
        assert np.array_equal(_bits(words[18:34]), _bits(mid.reshape(16)))
        assert r["valid"] and r["iterations"] >= 2
    finally:
        vm.destroy()
