"""Sweep deskew on the MI355X (qtr_deskew / qtr_keyframe_create_deskewed, libquatro_ext.so): bit-parity of the output and
the counts with the host restatement (tests/deskew_ref/deskew_ref.cpp) across the workgroup and knot-table sizes, on the
edge times and skipped points of the CPU test, from host and device memory, in place; the keyframe of a raw sweep against
the keyframe of its deskewed cloud; the refusals; deskewing scan-to-map odometry against the composition of the
restatements; what deskewing does to the odometry's error; and the C++ demo.  Everything goes through the C ABI
(quatro_amd.lib)."""
import os
import subprocess

import numpy as np
import pytest

import deskew_cases as K
import deskew_restate as D
import vmap_restate as M

pytestmark = pytest.mark.gpu

SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _same_map(vm, ref, what=""):
    fa, fb = {k: vm.fetch(k) for k in SECTIONS}, ref.fetch_all()
    for k in SECTIONS:
        _same(fa[k], fb[k], (what, k))
    ia, ib = vm.info(), ref.info()
    assert all(ia[k] == ib[k] for k in ("n_voxels", "n_inserts", "n_members")), (what, ia, ib)


def _same_keyframe(a, b, what=""):
    from quatro_amd import lib as ql
    for item in (ql.KF_VOX, ql.KF_NORMALS, ql.KF_FPFH, ql.KF_MEAN):
        _same(a.fetch(item), b.fetch(item), (what, item))
    assert a.info == b.info, (what, a.info, b.info)


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


@pytest.mark.parametrize("Kn", [2, 3, 256])
def test_bit_equal_to_the_restatement_across_block_and_table_sizes(hip, Kn):
    """P around the 256-point workgroup, K = 2 (one interval), 3 and 256 (the whole LDS table); times in no order, some of
    them outside the knots; t_ref inside an interval."""
    kt, kp = K.smooth_knots(Kn, seed=Kn, max_angle=1.2 if Kn == 3 else 0.05)
    t_ref = float(kt[0] + 0.3 * (kt[-1] - kt[0]))
    for P in (1, 255, 256, 257, 1000):
        cloud = K.random_cloud(P, seed=P)
        times = np.random.default_rng(P + Kn).uniform(2 * kt[0] - kt[1], 2 * kt[-1] - kt[-2], P).astype(np.float32)
        want, winfo = D.deskew(cloud, times, kt, kp, t_ref)
        got, info = hip.deskew(cloud, times, kt, kp, t_ref)
        assert info == winfo and info["n_points"] == P, (P, info, winfo)
        _same(got, want, (Kn, P))
    assert winfo["n_extrapolated"] > 0


def test_edge_times_skipped_points_and_identity_knots(hip):
    kt, kp = K.smooth_knots(5, 4)
    edges = K.edge_times(kt)
    cloud = K.random_cloud(len(edges), 6)
    times = np.array([t for t, _, _ in edges], np.float32)
    want, winfo = D.deskew(cloud, times, kt, kp, float(kt[0]))
    got, info = hip.deskew(cloud, times, kt, kp, float(kt[0]))
    assert info == winfo == {"n_points": len(edges), "n_skipped": 0, "n_extrapolated": sum(e for _, _, e in edges)}
    _same(got, want, "edge times")
    cloud, times, n_skip = K.skipped_cloud()
    kt3, kp3 = K.smooth_knots(3, 7)
    want, winfo = D.deskew(cloud, times, kt3, kp3, 0.0)
    got, info = hip.deskew(cloud, times, kt3, kp3, 0.0)
    assert info == winfo and info["n_skipped"] == n_skip
    _same(got, want, "skipped points")
    bad = ~(np.isfinite(cloud[:, :3]).all(axis=1) & np.isfinite(times))
    _same(got[bad], cloud[bad], "a skipped point keeps its bits")
    cloud = K.random_cloud(700, 8)
    got, info = hip.deskew(cloud, np.random.default_rng(0).uniform(-0.05, 0.15, 700).astype(np.float32), *K.identity_knots(7),
                           t_ref=0.04)
    assert np.array_equal(got, cloud) and info["n_extrapolated"] > 0


def test_host_and_device_memory_in_place_empty_and_twice(hip):
    import torch
    kt, kp = K.smooth_knots(17, 2, max_angle=0.3)
    cloud, times = K.random_cloud(1000, 3), K.random_times(1000, kt, 3)
    want, winfo = D.deskew(cloud, times, kt, kp, 0.02)
    got, info = hip.deskew(cloud, times, kt, kp, 0.02)
    again, info2 = hip.deskew(cloud, times, kt, kp, 0.02, slot=1)
    assert info == info2 == winfo
    _same(got, want, "host")
    _same(again, got, "the same bits twice")
    d_cloud, d_times = torch.from_numpy(cloud).cuda(), torch.from_numpy(times).cuda()
    d_out, info = hip.deskew(d_cloud, d_times, kt, kp, 0.02)
    assert info == winfo and d_out.data_ptr() != d_cloud.data_ptr()
    _same(d_out.cpu().numpy(), want, "device")
    _same(d_cloud.cpu().numpy(), cloud, "the input is only read")
    same, info = hip.deskew(d_cloud, d_times, kt, kp, 0.02, out=d_cloud)  # in place on device memory
    assert info == winfo and same.data_ptr() == d_cloud.data_ptr()
    _same(d_cloud.cpu().numpy(), want, "in place")
    with pytest.raises(ValueError):
        hip.deskew(d_cloud, times, kt, kp, 0.02)  # a device cloud with host times
    got, info = hip.deskew(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), kt, kp, 0.02)
    assert got.shape == (0, 4) and info == {"n_points": 0, "n_skipped": 0, "n_extrapolated": 0}


@pytest.fixture(scope="module")
def skewed_scan():
    """One kitti64_pair scan as a sensor records it that moves a metre and turns 0.04 rad during the sweep."""
    from quatro_amd import synth
    scan = synth.kitti64_pair(0)[0]
    kt, kp = K.two_knots(K.pose(K.rot([0.1, -0.2, 1.0], 0.04), (1.0, 0.05, -0.02)))
    skewed, times = K.skew(scan, kt, kp)
    for a in (skewed, times, kt, kp):
        a.setflags(write=False)
    return skewed, times, kt, kp


def test_keyframe_of_a_raw_sweep_is_the_keyframe_of_its_deskewed_cloud(hip, skewed_scan):
    import torch
    from quatro_amd import lib as ql
    skewed, times, kt, kp = skewed_scan
    fp = ql.default_frontend_params()
    out, info = hip.deskew(skewed, times, kt, kp, 0.0)
    _same(out, D.deskew(skewed, times, kt, kp, 0.0)[0], "the deskewed sweep")
    with hip.keyframe(out, fp) as want, hip.keyframe(skewed, fp) as raw, \
            hip.keyframe(skewed, fp, times=times, knot_times=kt, knot_poses=kp, t_ref=0.0) as got, \
            hip.keyframe(torch.tensor(skewed).cuda(), fp, slot=1, times=torch.tensor(times).cuda(), knot_times=kt,
                         knot_poses=kp) as got_dev:
        _same_keyframe(got, want, "host sweep")
        _same_keyframe(got_dev, want, "device sweep")
        assert got.deskew == got_dev.deskew == info == {"n_points": skewed.shape[0], "n_skipped": 0, "n_extrapolated": 0}
        assert not np.array_equal(raw.fetch(ql.KF_VOX), want.fetch(ql.KF_VOX))  # (the deskew is not a no-op here)


def test_refusals_leave_the_slot_usable(hip, skewed_scan):
    import ctypes as C
    from quatro_amd import lib as ql
    skewed, times, kt, kp = skewed_scan
    fp = ql.default_frontend_params()
    with hip.keyframe(skewed, fp) as kf:
        before = {i: kf.fetch(i) for i in (ql.KF_VOX, ql.KF_NORMALS, ql.KF_FPFH, ql.KF_MEAN)}
    cloud, t4 = K.random_cloud(4), np.zeros(4, np.float32)
    I3 = np.stack([np.eye(4)] * 3)
    over = K.pose(K.rot([1, 2, 3], 0.3) @ K.rot([0.3, -1, 0.5], K.ROTATION_LIMIT * (1 + 1e-9)))
    under = K.pose(K.rot([1, 2, 3], 0.3) @ K.rot([0.3, -1, 0.5], K.ROTATION_LIMIT * (1 - 1e-9)))
    base = K.pose(K.rot([1, 2, 3], 0.3))
    cases = [
        ((np.array([0.0]), np.eye(4)[None], 0.0), "knots"),
        (K.identity_knots(257) + (0.0,), "knots"),
        ((np.array([0.0, np.nan, 0.2]), I3, 0.0), "knot times"),
        ((np.array([0.0, 0.1, 0.1]), I3, 0.0), "knot times"),
        ((np.array([0.0, 0.2, 0.1]), I3, 0.0), "knot times"),
        ((np.array([0.0, 0.1]), np.stack([np.eye(4), K.pose(c=(0, np.inf, 0))]), 0.0), "non-finite"),
        ((np.array([0.0, 0.1]), np.stack([base, over]), 0.0), "rotation"),
        ((np.array([0.0, 0.1]), np.stack([np.eye(4), K.pose(K.rot([0, 0, 1], np.pi))]), 0.0), "rotation"),
        (K.identity_knots(2) + (np.nan,), "t_ref"),
        (K.identity_knots(2) + (-np.inf,), "t_ref"),
    ]
    for (bkt, bkp, t_ref), word in cases:
        for call in (lambda: hip.deskew(cloud, t4, bkt, bkp, t_ref),
                     lambda: hip.keyframe(skewed, fp, times=times, knot_times=bkt, knot_poses=bkp, t_ref=t_ref)):
            with pytest.raises(ql.QuatroHipError) as ei:
                call()
            assert ei.value.code == ql.QTR_ERR_BAD_ARG and word in str(ei.value), (word, str(ei.value))
    got, _ = hip.deskew(cloud, t4, np.array([0.0, 0.1]), np.stack([base, under]), 0.0)  # just under the limit: admitted
    _same(got, D.deskew(cloud, t4, np.array([0.0, 0.1]), np.stack([base, under]), 0.0)[0], "just under the limit")
    # NULL arrays with P > 0, P < 0, and P > max_points: through the C ABI itself
    dlib, out4, info = ql.load_ext(), np.zeros((4, 4), np.float32), ql.DeskewInfo()
    gkt, gkp = ql._knots(kt, kp)
    kfp = C.c_void_p()

    def raw_deskew(pc, pt, P, po):
        return dlib.qtr_deskew(hip._h, 0, pc, pt, P, gkt.ctypes.data, gkp.ctypes.data, 2, 0.0, po, ql.MEM_HOST, C.byref(info))

    def raw_keyframe(pc, pt, P):
        return dlib.qtr_keyframe_create_deskewed(hip._h, 0, pc, pt, P, gkt.ctypes.data, gkp.ctypes.data, 2, 0.0, C.byref(fp),
                                                 ql.MEM_HOST, C.byref(kfp), C.byref(info))
    assert raw_deskew(None, t4.ctypes.data, 4, out4.ctypes.data) == ql.QTR_ERR_BAD_ARG
    assert raw_deskew(cloud.ctypes.data, None, 4, out4.ctypes.data) == ql.QTR_ERR_BAD_ARG
    assert raw_deskew(cloud.ctypes.data, t4.ctypes.data, 4, None) == ql.QTR_ERR_BAD_ARG
    assert raw_deskew(cloud.ctypes.data, t4.ctypes.data, -1, out4.ctypes.data) == ql.QTR_ERR_BAD_ARG
    assert raw_deskew(cloud.ctypes.data, t4.ctypes.data, 262145, out4.ctypes.data) == ql.QTR_ERR_CAPACITY  # (never read)
    assert raw_keyframe(None, t4.ctypes.data, 4) == ql.QTR_ERR_BAD_ARG and not kfp.value
    assert raw_keyframe(cloud.ctypes.data, None, 4) == ql.QTR_ERR_BAD_ARG and not kfp.value
    assert raw_keyframe(cloud.ctypes.data, t4.ctypes.data, -1) == ql.QTR_ERR_BAD_ARG and not kfp.value
    assert raw_keyframe(cloud.ctypes.data, t4.ctypes.data, 262145) == ql.QTR_ERR_CAPACITY and not kfp.value
    assert raw_keyframe(cloud.ctypes.data, t4.ctypes.data, 0) == ql.QTR_ERR_BAD_ARG and not kfp.value  # (as qtr_keyframe_create)
    with hip.keyframe(skewed, fp) as kf:  # the slot's plain keyframe afterwards: its usual bits
        for i, a in before.items():
            _same(kf.fetch(i), a, ("after the refusals", i))


# ---- odometry ---------------------------------------------------------------------------------------------------------
def _cv_knots(T2, T1, period):
    """quatro_amd.api.constant_velocity_knots restated: ([0, period], [I, T2^-1 T1]), rigid inverse, fixed order."""
    A = [[float(x) for x in r] for r in np.asarray(T2, np.float64).reshape(4, 4)]
    B = [[float(x) for x in r] for r in np.asarray(T1, np.float64).reshape(4, 4)]
    inv = [[A[c][r] for c in range(3)] + [-((A[0][r] * A[0][3] + A[1][r] * A[1][3]) + A[2][r] * A[2][3])] for r in range(3)]
    inv.append([0.0, 0.0, 0.0, 1.0])
    Mo = [[((inv[r][0] * B[0][c] + inv[r][1] * B[1][c]) + inv[r][2] * B[2][c]) + inv[r][3] * B[3][c] for c in range(4)]
          for r in range(4)]
    Mo[3] = [0.0, 0.0, 0.0, 1.0]
    return np.array([0.0, float(period)]), np.stack([np.eye(4), np.array(Mo, np.float64)])


@pytest.fixture(scope="module")
def skewed_trajectory():
    """kitti64_trajectory(0, n_scans=6): its six path scans, each skewed with the scene's own motion — the sensor moves from
    its pose to the next pose of the path during the sweep (the last scan: as during the sweep before).  Returns (skewed
    scans, times, true knots per scan, true poses relative to the first)."""
    from quatro_amd import synth
    scans, gt = synth.kitti64_trajectory(0, n_scans=6)
    scans, gt = scans[:6], gt[:6]
    raw, times, knots = [], [], []
    for k in range(6):
        a, b = (k, k + 1) if k < 5 else (4, 5)
        kt, kp = K.two_knots(np.linalg.inv(gt[a]) @ gt[b])
        s, t = K.skew(scans[k], kt, kp)
        raw.append(s)
        times.append(t)
        knots.append((kt, kp))
    return raw, times, knots, [np.linalg.inv(gt[0]) @ g for g in gt]


def test_deskewing_odometry_is_the_composition_of_the_restatements(hip, skewed_trajectory):
    """scan_to_map_odometry(times=) against, scan by scan: the restated deskew of the raw scan under the knots the poses so
    far give, the device keyframe's fetched cloud and normals of that, and the voxel map's restatement; times=None against
    the unchanged restatement on the raw scans."""
    from quatro_amd import api
    from quatro_amd import lib as ql
    raw, times, _, _ = skewed_trajectory
    fp = ql.default_frontend_params()
    ref, poses, results = M.RefMap(1.0, 1 << 16), [], []
    for k in range(6):
        kt, kp = _cv_knots(poses[-2], poses[-1], K.PERIOD) if k >= 2 else K.identity_knots(2)
        desk, info = D.deskew(raw[k], times[k], kt, kp, 0.0)
        assert info["n_skipped"] == 0 and info["n_extrapolated"] == 0
        with hip.keyframe(desk, fp) as kf:
            c, n = kf.fetch(ql.KF_VOX), kf.fetch(ql.KF_NORMALS)
        if k == 0:
            T = np.eye(4)
        else:
            guess = poses[-1] if k == 1 else M.constant_velocity_guess(poses[-2], poses[-1])
            r = ref.register(c, n, guess)
            results.append(r)
            T = r["T"].copy() if r["valid"] else np.array(guess, np.float64)
        ref.insert(c, n, T)
        poses.append(T)
    assert all(r["valid"] for r in results)
    maps = []
    try:
        got, vm = api.scan_to_map_odometry(hip, raw, fp, voxel_size=1.0, capacity=1 << 16, times=times, sweep_period=K.PERIOD)
        maps.append(vm)
        _same(got, np.stack(poses), "deskewing odometry")
        _same_map(vm, ref, "deskewing odometry's map")
        # times=None: what it is today
        kfs = [hip.keyframe(s, fp) for s in raw]
        try:
            want0, ref0, results0 = M.odometry([k.fetch(ql.KF_VOX) for k in kfs], [k.fetch(ql.KF_NORMALS) for k in kfs], 1.0, 1 << 16)
        finally:
            for k in kfs:
                k.close()
        got0, vm0 = api.scan_to_map_odometry(hip, raw, fp, voxel_size=1.0, capacity=1 << 16, times=None)
        maps.append(vm0)
        _same(got0, want0, "times=None")
        _same_map(vm0, ref0, "times=None")
        assert not np.array_equal(got, got0)
        with pytest.raises(ValueError):
            api.scan_to_map_odometry(hip, raw, fp, times=times)  # times without sweep_period
    finally:
        for m in maps:
            m.destroy()


def test_deskewing_with_the_true_motion_brings_the_odometry_closer_to_the_scene(hip, skewed_trajectory):
    """The physical check: keyframes of the skewed scans made with the TRUE motion as knots, fed to scan_to_map_odometry, end
    closer to the scene's last pose than the same run on the skewed scans as they are.  Only that inequality is asserted; the
    errors, and those of the constant-velocity variant, are printed.

    Measured on an MI355X, translation error of the last pose: 0.0122 m with the true motion, 0.1915 m without deskew,
    0.3335 m with constant-velocity knots (why that is worse here: DESIGN.md section 17)."""
    from quatro_amd import api
    from quatro_amd import lib as ql
    raw, times, knots, truth = skewed_trajectory
    fp = ql.default_frontend_params()

    def run(scans, **kw):
        poses, vm = api.scan_to_map_odometry(hip, scans, fp, voxel_size=1.0, capacity=1 << 16, **kw)
        vm.destroy()
        return [float(np.linalg.norm(p[:3, 3] - t[:3, 3])) for p, t in zip(poses, truth)]
    kfs = [hip.keyframe(s, fp, times=t, knot_times=kt, knot_poses=kp, t_ref=0.0) for s, t, (kt, kp) in zip(raw, times, knots)]
    try:
        e_true = run(kfs)
    finally:
        for k in kfs:
            k.close()
    e_none = run(raw)
    e_cv = run(raw, times=times, sweep_period=K.PERIOD)
    for name, e in (("true-motion knots", e_true), ("no deskew", e_none), ("constant-velocity knots", e_cv)):
        print(f"odometry on skewed scans, {name}: translation error per scan {['%.4f' % x for x in e]} m")
    assert e_true[-1] < e_none[-1], (e_true, e_none)


def test_cpp_deskew_demo_prints_what_the_python_calls_return(hip, skewed_scan, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    skewed, times, kt, kp = skewed_scan
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "deskew_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "deskew_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath),
                           "-Wl,-rpath,/opt/rocm/lib"])
    sweep, tfile, kfile = str(tmp_path / "sweep.bin"), str(tmp_path / "times.f32"), str(tmp_path / "knots.txt")
    synth.save_kitti_bin(sweep, skewed)
    np.asarray(times, np.float32).tofile(tfile)
    np.savetxt(kfile, np.concatenate([kt[:, None], kp.reshape(-1, 16)], axis=1), fmt="%.17g")
    out = subprocess.run([exe, sweep, tfile, kfile, "0.0", "0.025"], capture_output=True, text=True, check=True,
                         timeout=180).stdout.split("\n")
    got, info = hip.deskew(skewed, times, kt, kp, 0.0)

    def xor(a):
        return int(np.bitwise_xor.reduce(_bits(a).reshape(-1)))
    assert out[0] == (f"deskew: points {info['n_points']} skipped {info['n_skipped']} extrapolated {info['n_extrapolated']} "
                      f"records {xor(got):08x}"), out[0]
    with hip.keyframe(got, ql.default_frontend_params()) as kf:
        assert out[1] == (f"keyframe: points {kf.info['n_points']} voxels {kf.info['n_voxels']} skipped 0 "
                          f"voxels {xor(kf.fetch(ql.KF_VOX)):08x}"), out[1]
    T = np.array([float(x) for x in out[2].split()[1:]]).reshape(4, 4)
    _same(T, ql.deskew_pose_at(kt, kp, 0.025), "pose_at")
