"""The persistent Gaussian voxel map on the MI355X (qtr_voxel_map_*): bit-parity with the host restatement
(tests/vmap_ref/vmap_ref.cpp) of the records after every insert and of every iteration of a registration, a crowded table
whose probe chains wrap, the capacity refusal, the equality with the merged method 3 on positive-octant targets, the
single-call loops in blocks (QTR_ICP_BLOCK) against the unblocked ones, the path equalities, scan-to-map odometry and build_map, the refusals, the C++ demo and the two libraries' symbol tables.  Everything
goes through the C ABI (quatro_amd.lib; the map's entry points are libquatro_ext.so's, include/quatro_voxelmap.h)."""
import os
import subprocess

import numpy as np
import pytest

import icp_restate as R
import vgicp_restate as V
import vmap_cases as K
import vmap_restate as M

pytestmark = pytest.mark.gpu

ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")
SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)


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


def _sections(m):
    return m.fetch_all() if isinstance(m, M.RefMap) else {k: m.fetch(k) for k in SECTIONS}


def _same_map(a, b, what=""):
    fa, fb = _sections(a), _sections(b)
    for k in SECTIONS:
        assert fa[k].shape == fb[k].shape and np.array_equal(_bits(fa[k]), _bits(fb[k])), (what, k)
    ia, ib = a.info(), b.info()
    assert all(ia[k] == ib[k] for k in ("n_voxels", "n_inserts", "n_members")), (what, ia, ib)


def _vg(**kw):
    from quatro_amd import lib as ql
    return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)


def _register_both(hip, vm, ref, s, sn, guess, iters, what=""):
    """A registration of `iters` iterations (both epsilons 0) on the device and in the restatement: final record, the trace
    of every update and the last correspondence flags, bit for bit.  Returns the device result."""
    from quatro_amd import lib as ql
    g = vm.register(s, sn, guess, _vg(max_iterations=iters, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0))
    trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    corr = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
    o = ref.register(s, sn, guess, teps=0.0, feps=0.0, max_iter=iters)
    _same_icp(g, o, what)
    assert np.array_equal(_bits(trace), _bits(o["trace"])) and np.array_equal(corr, o["corr"]), what
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
def hand():
    return K.hand_built()


@pytest.fixture(scope="module")
def vox_pair(hip):
    """kitti64_pair(2)'s voxel clouds with both normal sets from qtr_fpfh."""
    from quatro_amd import synth
    s, t, Tgt = synth.kitti64_pair(2)
    vs, vt = hip.voxelize(s, 0.3), hip.voxelize(t, 0.3)
    ns, _ = hip.fpfh(vs, 0.5, 0.5)
    nt, _ = hip.fpfh(vt, 0.5, 0.5)
    return vs, vt, ns, nt, Tgt


def test_hand_built_case_is_bit_equal_to_the_restatement(hip, hand):
    inserts, s, sn = hand
    vm, ref = hip.voxel_map(K.SIDE, 4096), M.RefMap(K.SIDE, 4096)
    try:
        for j, (p, n, pose) in enumerate(inserts):
            assert vm.insert(p, n, pose) == ref.insert(p, n, pose), j
            _same_map(vm, ref, f"after insert {j}")
        by = {tuple(c): int(n) for c, n in zip(vm.fetch(M.COORDS), vm.fetch(M.COUNT))}
        print(f"hand-built: {len(by)} voxels, {vm.info()['n_members']} members; sizes {sorted(by.values())[-4:]}")
        assert (by[K.V1], by[K.V65], by[K.V300], by[K.VALL]) == (1, 65, 300, 21)
        assert by[(K.LO, 0, 0)] == 1 and by[(0, K.HI, 0)] == 1
        _register_both(hip, vm, ref, s, sn, np.eye(4), 1, "identity, one iteration")
        for k in range(1, 9):  # every iteration's T, n_corr, stop reason, fitness and rmse: the loop cut after k updates
            g = _register_both(hip, vm, ref, s, sn, K.GUESS, k, f"{k} iterations")
            assert g["valid"] and g["iterations"] == k
    finally:
        vm.destroy()


def test_crowded_table_and_the_capacity_refusal(hip):
    from quatro_amd import lib as ql
    coords, extra = K.crowded(64, 62)
    S = M.table_slots(64)
    assert S == 128 and all(M.hash_slot(M.key(*c), S) >= S - 6 for c in np.concatenate([coords, extra]))
    pts, nrm = K.cloud_of_voxels(coords, 1.0)
    vm, ref = hip.voxel_map(1.0, 64), M.RefMap(1.0, 64)
    try:
        assert vm.insert(pts, nrm) == ref.insert(pts, nrm)
        _same_map(vm, ref, "62 voxels on six home slots")
        s, sn = K.cloud_of_voxels(np.concatenate([coords[::2], extra]), 1.0, per_voxel=(3,), seed=8)
        _register_both(hip, vm, ref, s, sn, R.rigid(R.rot(0.002, 0.001, -0.002), [0.01, 0.02, -0.01]), 4, "crowded")
        before = _sections(vm)
        more, more_n = K.cloud_of_voxels(np.concatenate([coords[:5], extra[:3]]), 1.0, seed=5)  # 3 new voxels: 65 > 64
        with pytest.raises(ql.QuatroHipError) as ei:
            vm.insert(more, more_n)
        assert ei.value.code == ql.QTR_ERR_CAPACITY and "capacity=64" in str(ei.value) and "62" in str(ei.value), str(ei.value)
        with pytest.raises(M.CapacityError):
            ref.insert(more, more_n)
        after = _sections(vm)
        assert all(np.array_equal(_bits(before[k]), _bits(after[k])) for k in SECTIONS)
        _same_map(vm, ref, "after the refusal")
        fit, fit_n = K.cloud_of_voxels(np.concatenate([coords[:5], extra[:2]]), 1.0, seed=5)  # 2 new: exactly 64 of 64
        assert vm.insert(fit, fit_n) == ref.insert(fit, fit_n)
        _same_map(vm, ref, "64 of 64 voxels")
        one, one_n = K.cloud_of_voxels(extra[2:3], 1.0, seed=6)  # the 65th voxel
        with pytest.raises(ql.QuatroHipError) as ei:
            vm.insert(one, one_n)
        assert ei.value.code == ql.QTR_ERR_CAPACITY and "capacity=64" in str(ei.value), str(ei.value)
        _same_map(vm, ref, "after the second refusal")
        again, again_n = K.cloud_of_voxels(coords[10:40], 1.0, seed=7)  # existing voxels only: fits
        assert vm.insert(again, again_n) == ref.insert(again, again_n)
        _same_map(vm, ref, "a fitting insert after the refusals")
        _register_both(hip, vm, ref, s, sn, np.eye(4), 3, "full table")
    finally:
        vm.destroy()


def _against_method_3(hip, s, sn, t, tn, guess, iters, what):
    """qtr_voxel_map_register on a map of t under pose = NULL against qtr_gicp method 3 at max_correspondence_distance =
    voxel_size = 1: first the two restatements on the CPU, then the two device paths, every iteration."""
    from quatro_amd import lib as ql
    ref = M.RefMap(1.0, 1 << 16)
    ref.insert(t, tn, None)
    a = ref.register(s, sn, guess, teps=0.0, feps=0.0, max_iter=iters)
    b = V.run(s, sn, t, tn, guess, max_d=1.0, teps=0.0, feps=0.0, max_iter=iters)
    assert np.array_equal(b["grid"][:3], [0, 0, 0]), what
    assert a["iterations"] == b["iterations"] and a["iterations"] >= min(iters, 3), what
    assert np.array_equal(_bits(a["trace"]), _bits(b["trace"])), what + ": the restatements differ"
    prm = _vg(max_iterations=iters, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0, max_correspondence_distance=1.0)
    vm = hip.voxel_map(1.0, 1 << 16)
    try:
        vm.insert(t, tn, None)
        g3 = hip.gicp(s, t, sn, tn, guess, prm)
        trace3 = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
        corr3 = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
        gm = vm.register(s, sn, guess, prm)
        trace_m = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
        corr_m = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
        _same_icp(gm, g3, what + ": map against method 3")
        assert np.array_equal(_bits(trace_m), _bits(trace3)) and trace_m.shape[0] == g3["iterations"], what
        assert np.array_equal(corr_m == 0, corr3 >= 0) and np.array_equal(corr_m == -1, corr3 == -1), what
        _same_icp(gm, a, what + ": map against its restatement")
        print(f"{what}: {gm['iterations']} iterations, {gm['n_corr']} correspondences, {len(vm)} voxels")
    finally:
        vm.destroy()


def test_map_registration_equals_method_3_bit_for_bit(hip, vox_pair):
    s, sn, t, tn = K.octant_hand_built()
    _against_method_3(hip, s, sn, t, tn, np.eye(4), 1, "hand-built, identity")
    _against_method_3(hip, s, sn, t, tn, K.GUESS, 10, "hand-built")
    vs, vt, ns, nt, Tgt = vox_pair
    s2, t2 = K.into_octant(vs, vt)
    tn2 = np.concatenate([nt, np.array([[0.0, 0.0, 1.0, 0.0]], np.float32)])
    shift = (t2[0, :3] - vt[0, :3]).astype(np.float64)
    G0 = R.rigid(np.eye(3), shift) @ Tgt @ R.rigid(R.rot(0.012, -0.009, 0.015), [0.25, -0.3, 0.08]) @ R.rigid(np.eye(3), -shift)
    _against_method_3(hip, s2, ns, t2, tn2, G0, 12, "kitti64_pair(2) in the positive octant")


def _handle(n_slots, **env):
    """A handle created under these environment variables (the handle reads them once, when it is made)."""
    from quatro_amd import lib as ql
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ql.Handle(0, n_slots=n_slots)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_single_call_loops_in_blocks_equal_the_unblocked_loops(hip):
    """QTR_ICP_BLOCK=4 against all launches at once, through both single-call entries of the one host loop: qtr_gicp method 3
    and VoxelMap.register on a map of the targets under no pose (300 sources: two workgroups per launch, so the last-arriver
    path is live).  10 fixed updates are the blocks 4 + 4 + 2, the last one short; with transformation_epsilon = 1e-2 both
    restatements stop after 6 updates (reason 2) on this input, inside the second block, so the host leaves the loop at its
    second read-back."""
    from quatro_amd import lib as ql
    s, sn, t, tn = K.octant_hand_built()
    assert s.shape[0] == 300 and t.shape[0] == 500
    blocked = _handle(1, QTR_ICP_BLOCK="4")
    maps = []
    try:
        for h in (hip, blocked):
            maps.append(h.voxel_map(1.0, 1 << 16))
            maps[-1].insert(t, tn, None)
        for kw, iters in ((dict(max_iterations=10, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0), 10),
                          (dict(max_iterations=30, transformation_epsilon=1e-2, euclidean_fitness_epsilon=0.0), 6)):
            prm = _vg(max_correspondence_distance=1.0, **kw)
            for what in ("qtr_gicp method 3", "VoxelMap.register"):
                got = []
                for h, vm in zip((hip, blocked), maps):
                    g = h.gicp(s, t, sn, tn, K.GUESS, prm) if what.startswith("qtr_gicp") else vm.register(s, sn, K.GUESS, prm)
                    got.append((g, h.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18), h.debug_fetch(ql.DBG_ICP_CORR, np.int32)))
                (g0, trace0, corr0), (g1, trace1, corr1) = got
                print(f"{what}, {kw}: {g0['iterations']} / {g1['iterations']} iterations, stop {g0['stop_reason']} / {g1['stop_reason']}")
                assert g0["iterations"] == iters and g0["valid"], (what, kw, g0)
                _same_icp(g1, g0, f"{what}, {kw}: blocked against unblocked")
                assert trace1.shape == trace0.shape == (iters, 18) and np.array_equal(_bits(trace1), _bits(trace0)), (what, kw)
                assert np.array_equal(corr1, corr0), (what, kw)
    finally:
        for m in maps:
            m.destroy()
        blocked.close()


def test_path_equalities(hip, vox_pair):
    import torch
    from quatro_amd import lib as ql
    from quatro_amd import synth
    vs, vt, ns, nt, Tgt = vox_pair
    pose = R.rigid(R.rot(0.01, -0.02, 0.3), [1.5, -2.0, 0.25])
    G0 = pose @ Tgt @ R.rigid(R.rot(0.012, -0.009, 0.015), [0.25, -0.3, 0.08])
    prm = _vg(max_iterations=10)
    made = []

    def new_map(side=1.0, cap=1 << 15):
        made.append(hip.voxel_map(side, cap))
        return made[-1]

    try:
        base = new_map()
        base.insert(vt, nt, pose)
        want = base.register(vs, ns, G0, prm)
        assert want["valid"] and want["iterations"] >= 3
        # the same result twice in a row, and from a second map built the same way: slot placement does not show
        _same_icp(base.register(vs, ns, G0, prm), want, "twice")
        twin = new_map()
        twin.insert(vt, nt, pose)
        _same_map(twin, base, "a second map")
        _same_icp(twin.register(vs, ns, G0, prm, slot=1), want, "a second map, the other slot")
        # whole = halves
        halves = new_map()
        h = vt.shape[0] // 2 + 17
        halves.insert(vt[:h], nt[:h], pose)
        halves.insert(vt[h:], nt[h:], pose)
        for k in (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD):
            assert np.array_equal(_bits(halves.fetch(k)), _bits(base.fetch(k))), k
        # device memory = host memory
        d = [torch.from_numpy(x).cuda() for x in (vs, ns, vt, nt)]
        dev = new_map()
        dev.insert(d[2], d[3], pose)
        _same_map(dev, base, "device-resident insert")
        _same_icp(base.register(d[0], d[1], G0, prm), want, "device-resident source")
        # clear then re-insert = a fresh map; the other map on the handle is not disturbed
        twin.clear()
        assert len(twin) == 0 and twin.fetch(M.CLOUD).shape == (0, 4) and twin.info()["n_inserts"] == 0
        e = twin.register(vs, ns, G0, prm)
        assert not e["valid"] and e["n_corr"] == 0 and e["stop_reason"] == ql.ICP_STOP_TOO_FEW and np.array_equal(e["T"], G0)
        twin.insert(vt, nt, pose)
        _same_map(twin, base, "clear, then the same insert")
        other = new_map(0.7, 1 << 15)
        other.insert(vs, ns, None)
        _same_icp(base.register(vs, ns, G0, prm), want, "with another map alive")
        _same_map(twin, base, "with another map alive")
        # keyframe entries = the cloud entries on the keyframe's fetched sections
        kf = hip.keyframe(synth.kitti64_pair(2)[1])
        try:
            kv, kn = kf.fetch(ql.KF_VOX), kf.fetch(ql.KF_NORMALS)
            a, b = new_map(), new_map()
            assert a.insert_keyframe(kf, pose) == b.insert(kv, kn, pose)
            _same_map(a, b, "insert_keyframe")
            _same_icp(a.register_keyframe(kf, pose), a.register(kv, kn, pose), "register_keyframe")
        finally:
            kf.close()
        # methods 0 - 3 on the slot give the same bits before and after a map registration on it
        def four():
            out = [hip.icp(vs, vt, nt, Tgt, ql.default_icp_params(method=mth, max_iterations=6)) for mth in (0, 1)]
            return out + [hip.gicp(vs, vt, ns, nt, Tgt, ql.default_icp_params(method=mth, max_iterations=6)) for mth in (2, 3)]
        before = four()
        _same_icp(base.register(vs, ns, G0, prm), want, "between the method runs")
        for mth, (x, y) in enumerate(zip(before, four())):
            _same_icp(x, y, f"method {mth}")
    finally:
        for m in made:
            m.destroy()


def test_scan_to_map_odometry_and_build_map(hip):
    from quatro_amd import api, synth
    from quatro_amd import lib as ql
    scans, gt = synth.kitti64_trajectory(0, n_scans=6)
    scans, gt = scans[:6], gt[:6]
    fp = ql.default_frontend_params()
    kfs = [hip.keyframe(s, fp) for s in scans]
    vm = bm = None
    try:
        poses, vm = api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, capacity=1 << 16)
        clouds, normals = [k.fetch(ql.KF_VOX) for k in kfs], [k.fetch(ql.KF_NORMALS) for k in kfs]
        want, ref, results = M.odometry(clouds, normals, 1.0, 1 << 16)
        assert np.array_equal(_bits(poses), _bits(want))
        _same_map(vm, ref, "the odometry's map")
        bm = api.build_map(hip, kfs, poses, 1.0, 1 << 16)
        _same_map(bm, vm, "build_map under the odometry's poses")
        _same_icp(api.localize(hip, bm, kfs[3], poses[3]), ref.register(clouds[3], normals[3], poses[3]), "localize")
        # what the restatement shows: every registration valid, and the drift against the scene's
        # own poses
        rel = [np.linalg.inv(gt[0]) @ g for g in gt]
        terr = [float(np.linalg.norm(p[:3, 3] - r[:3, 3])) for p, r in zip(want, rel)]
        rerr = [R.rot_err_deg(p, r) for p, r in zip(want, rel)]
        print(f"odometry (restatement): {len(ref)} voxels; translation error per scan {['%.3f' % e for e in terr]} m, "
              f"rotation {['%.3f' % e for e in rerr]} deg; iterations {[r['iterations'] for r in results]}")
        assert all(r["valid"] for r in results)
    finally:
        for m in (vm, bm):
            if m is not None:
                m.destroy()
        for k in kfs:
            k.close()


def test_refusals(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    for kw, word in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=-1.0), "voxel_size"),
                     (dict(voxel_size=float("nan")), "voxel_size"), (dict(capacity=0), "capacity"), (dict(capacity=-5), "capacity")):
        with pytest.raises(ql.QuatroHipError) as ei:
            hip.voxel_map(**kw)
        assert ei.value.code == ql.QTR_ERR_BAD_ARG and word in str(ei.value), (kw, str(ei.value))
    vm = hip.voxel_map(1.0, 1 << 15)
    other = ql.Handle(0)
    kf = foreign_kf = foreign_map = None
    try:
        vm.insert(vt, nt)
        want = _sections(vm)

        def refused(code, word, fn, *a, **k):
            with pytest.raises(ql.QuatroHipError) as ei:
                fn(*a, **k)
            assert ei.value.code == code and word in str(ei.value), (word, str(ei.value))

        for mth in (0, 1, 2):
            refused(ql.QTR_ERR_BAD_ARG, "QTR_ICP_VOXEL_PLANE_TO_PLANE", vm.register, vs, ns, Tgt, ql.default_icp_params(method=mth))
        refused(ql.QTR_ERR_BAD_ARG, "normals", vm.register, vs, None, Tgt)
        refused(ql.QTR_ERR_BAD_ARG, "normals", vm.insert, vs, None)
        bad = np.eye(4)
        bad[1, 3] = np.nan
        refused(ql.QTR_ERR_BAD_ARG, "non-finite", vm.insert, vs, ns, bad)
        refused(ql.QTR_ERR_BAD_ARG, "non-finite", vm.register, vs, ns, bad)
        bad[1, 3] = np.inf
        refused(ql.QTR_ERR_BAD_ARG, "non-finite", vm.insert, vs, ns, bad)
        big = np.zeros((hip.limits.max_points + 1, 4), np.float32)
        refused(ql.QTR_ERR_CAPACITY, "max_points", vm.insert, big, big)
        refused(ql.QTR_ERR_CAPACITY, "max_points", vm.register, big, big)
        foreign_kf = other.keyframe(np.concatenate([vs, vt]))
        kf = hip.keyframe(np.concatenate([vs, vt]))
        foreign_map = other.voxel_map(1.0, 64)
        refused(ql.QTR_ERR_BAD_ARG, "another handle", vm.insert_keyframe, foreign_kf)
        refused(ql.QTR_ERR_BAD_ARG, "another handle", vm.register_keyframe, foreign_kf)
        stolen = ql.VoxelMap(hip, foreign_map._m.value)  # the other handle's map through this handle
        refused(ql.QTR_ERR_BAD_ARG, "another handle", stolen.insert, vs, ns)
        refused(ql.QTR_ERR_BAD_ARG, "another handle", stolen.register, vs, ns)
        refused(ql.QTR_ERR_BAD_ARG, "another handle", stolen.insert_keyframe, kf)
        refused(ql.QTR_ERR_BAD_ARG, "another handle", stolen.clear)
        with pytest.raises(ql.QuatroHipError):
            stolen.fetch(M.CLOUD)
        stolen._m = None  # (not this wrapper's to destroy)
        got = _sections(vm)
        assert all(np.array_equal(_bits(want[k]), _bits(got[k])) for k in SECTIONS) and vm.info()["n_inserts"] == 1
        # an empty cloud is not an error
        assert vm.insert(vs[:0], ns[:0])["n_points"] == 0
        e = vm.register(vs[:0], ns[:0], Tgt)
        assert not e["valid"] and e["stop_reason"] == ql.ICP_STOP_TOO_FEW and np.array_equal(e["T"], Tgt)
    finally:
        for k in (kf, foreign_kf):
            if k is not None:
                k.close()
        if foreign_map is not None:
            foreign_map.destroy()
        vm.destroy()
        other.close()


def test_cpp_voxelmap_demo_prints_what_the_python_calls_return(hip, vox_pair, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "voxelmap_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "voxelmap_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    vs, vt, ns, nt, Tgt = vox_pair
    pose_a, pose_b = R.rigid(R.rot(0.0, 0.0, 0.2), [1.0, 2.0, 0.0]), None
    pose_b = pose_a @ np.linalg.inv(Tgt)  # the source cloud under the pose that lays it over the target
    guess = pose_a @ Tgt @ R.rigid(R.rot(0.01, -0.01, 0.01), [0.1, -0.1, 0.05])
    args = ["1.0"]
    for name, a in (("a", vt), ("an", nt), ("pa", pose_a), ("b", vs), ("bn", ns), ("pb", pose_b), ("q", vs), ("qn", ns), ("g", guess)):
        path = str(tmp_path / name)
        if a.shape == (4, 4):
            np.savetxt(path, a, fmt="%.17g")
        else:
            synth.save_kitti_bin(path, a)
        args.append(path)
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    vm = hip.voxel_map(1.0, 1 << 16)
    try:
        ia, ib = vm.insert(vt, nt, pose_a), vm.insert(vs, ns, pose_b)
        r = vm.register(vs, ns, guess)
        for k, i in enumerate((ia, ib)):
            assert out[k] == (f"insert {k}: points {i['n_points']} members {i['n_members']} new {i['n_new_voxels']} "
                              f"touched {i['n_touched_voxels']}"), out[k]
        info = vm.info()
        assert out[2] == f"map: voxels {info['n_voxels']} members {info['n_members']} inserts 2 cloud {info['n_voxels']}", out[2]
        assert out[3] == f"iterations {r['iterations']} stop {r['stop_reason']} corr {r['n_corr']} valid {int(r['valid'])}", out[3]
        words = np.array([int(x, 16) for ln in out[4:9] for x in ln.split()], dtype=np.uint64).view(np.float64)
        assert np.array_equal(_bits(words[:16]), _bits(r["T"].reshape(16)))
        assert _f64bits(words[16]) == _f64bits(r["fitness"]) and _f64bits(words[17]) == _f64bits(r["rmse"])
        assert r["valid"] and r["iterations"] >= 2
    finally:
        vm.destroy()
