"""Submap keyframes on the MI355X (qtr_keyframe_merge): the merged keyframe bit-equal to qtr_keyframe_create on the
host-built concatenation (tests/submap_restate.py), registrations against it bit-equal to the raw-scan entries, the place
index, the contract's edges, and api.close_loop with submaps end to end.  Every comparison is bit-exact against a path that
existed before the merge did.  Everything goes through the C ABI binding."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import place_restate as pr
import submap_restate as sr

pytestmark = pytest.mark.gpu

ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")
REG_INT_KEYS = ("status", "valid", "gnc_iters", "max_core", "n_edges", "n_card", "n_src", "n_tgt", "L", "n_rot_inliers",
                "n_clique", "n_final")
N_SCANS, MID, QUERY = 17, 8, 17


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same_reg(a, b, what=""):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert _f64bits(a["cost"]) == _f64bits(b["cost"]), what
    for k in REG_INT_KEYS:
        if k in a and k in b:
            assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("clique", "final_inliers"):
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), (what, k)


def _same_icp(a, b, what=""):
    assert a["status"] == b["status"], what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _same_keyframe(a, b, what=""):
    from quatro_amd import lib as ql
    assert a.info == b.info, (what, a.info, b.info)
    for item in (ql.KF_VOX, ql.KF_NORMALS, ql.KF_FPFH, ql.KF_MEAN):
        assert np.array_equal(_bits(a.fetch(item)), _bits(b.fetch(item))), (what, item)


@pytest.fixture(scope="module")
def h4():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=4)
    yield h
    h.close()


@pytest.fixture(scope="module")
def traj(h4):
    """kitti64_trajectory(0): seventeen scans 1 m apart and the revisit of the middle one, their keyframes, the keyframes'
    voxels on the host."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    scans, poses = synth.kitti64_trajectory(0, N_SCANS, 1.0)
    kfs = [h4.keyframe(s, slot=i % 4) for i, s in enumerate(scans)]
    vox = [kf.fetch(ql.KF_VOX) for kf in kfs]
    yield scans, poses, kfs, vox
    for kf in kfs:
        kf.close()


def _window(poses, vox, centre, hw, lo=0, hi=N_SCANS):
    """(member ids, relative poses, the concatenation built on the host) of the submap around `centre`"""
    ids = list(range(max(centre - hw, lo), min(centre + hw + 1, hi)))
    rel = np.stack([np.linalg.inv(poses[centre]) @ poses[i] for i in ids])
    return ids, rel, sr.merge([vox[i] for i in ids], rel)


# ---- the merged keyframe is qtr_keyframe_create's --------------------------------------------------------------------------
@pytest.mark.parametrize("fp_kw", [{}, {"voxel_size": 0.45}], ids=["members' fp", "coarser leaf"])
@pytest.mark.parametrize("hw", [0, 1, 3, 8], ids=["K=1", "K=3", "K=7", "K=17"])
def test_merge_is_bit_identical_to_keyframe_create_on_the_host_built_cloud(h4, traj, hw, fp_kw):
    from quatro_amd import lib as ql
    _, poses, kfs, vox = traj
    fp = ql.default_frontend_params(**fp_kw)
    ids, rel, cat = _window(poses, vox, MID, hw)
    assert len(ids) == 2 * hw + 1
    with h4.merge_keyframes([kfs[i] for i in ids], rel, fp) as got, h4.keyframe(cat, fp) as want:
        print(f"K = {len(ids)}, {fp_kw}: {cat.shape[0]} voxels in, {got.info['n_voxels']} out, {got.info['device_bytes']} bytes")
        assert got.info["n_points"] == cat.shape[0] == sum(v.shape[0] for v in (vox[i] for i in ids))
        assert got.info["voxel_size"] == np.float32(fp.voxel_size) and got.info["passed_through"] == 0
        _same_keyframe(got, want, f"K {len(ids)} {fp_kw}")
        if hw:  # (not vacuous: the members were moved, and the grid fused what they share)
            assert not np.array_equal(sr.transform(rel[0], vox[ids[0]]), vox[ids[0]])
            assert got.info["n_voxels"] < cat.shape[0]
    if hw == 0:  # no poses = identities: a re-voxelisation of the member's own voxels
        with h4.merge_keyframes([kfs[MID]], None, fp, slot=1) as got, h4.keyframe(vox[MID], fp) as want:
            _same_keyframe(got, want, "identity")
            if not fp_kw:
                assert np.array_equal(_bits(got.fetch(ql.KF_VOX)), _bits(vox[MID]))


def test_repeated_member_and_other_slot(h4, traj):
    _, poses, kfs, vox = traj
    rel = np.stack([np.eye(4), np.linalg.inv(poses[MID]) @ poses[MID + 1], np.eye(4)])
    cat = sr.merge([vox[MID], vox[MID + 1], vox[MID]], rel)
    with h4.merge_keyframes([kfs[MID], kfs[MID + 1], kfs[MID]], rel, slot=2) as got, h4.keyframe(cat, slot=3) as want:
        assert got.info["n_points"] == 2 * vox[MID].shape[0] + vox[MID + 1].shape[0]
        _same_keyframe(got, want, "member twice")


# ---- registrations against a submap -------------------------------------------------------------------------------------
def test_registration_against_a_submap_equals_register_pair_on_the_host_built_cloud(h4, traj):
    from quatro_amd import lib as ql
    scans, poses, kfs, vox = traj
    ids, rel, cat = _window(poses, vox, MID, 2)
    with h4.merge_keyframes([kfs[i] for i in ids], rel) as sub:
        for seed, fp_kw in ((0, {}), (3, {"use_crosscheck": 0})):
            fp = ql.default_frontend_params(seed=seed, **fp_kw)
            a = h4.register_pair(scans[QUERY], cat, fp)
            ca = h4.debug_fetch(ql.DBG_CORR, np.int32)
            ra = [h4.refine_pair(None, ql.default_icp_params(method=m)) for m in (0, 1, 2)]
            b = h4.register_keyframes(kfs[QUERY], sub, fp)
            cb = h4.debug_fetch(ql.DBG_CORR, np.int32)
            rb = [h4.refine_pair(None, ql.default_icp_params(method=m)) for m in (0, 1, 2)]
            _same_reg(b, a, f"seed {seed} {fp_kw}")
            assert np.array_equal(ca, cb), seed
            for m in range(3):
                _same_icp(rb[m], ra[m], f"seed {seed} method {m}")
            assert a["status"] == ql.QTR_OK and a["valid"] and a["n_tgt"] == sub.info["n_voxels"], seed


def test_one_to_many_job_against_five_submaps_equals_the_single_calls(h4, traj):
    from quatro_amd import api
    from quatro_amd import lib as ql
    _, poses, kfs, vox = traj
    fp, icp = ql.default_frontend_params(seed=2), ql.default_icp_params()
    subs = []
    try:
        for n, c in enumerate((4, 6, 8, 10, 12)):
            subs.append(api.make_submap(h4, kfs, poses, c, 2, fp, slot=n % 4))
        single, single_ref = [], []
        for s in subs:
            single.append(h4.register_keyframes(kfs[QUERY], s, fp))
            single_ref.append(h4.refine_pair(None, icp))
        recs, best = api.register_one_to_many(h4, kfs[QUERY], subs, fp)
        recs2, refined, best2 = api.register_one_to_many(h4, kfs[QUERY], subs, fp, icp=icp)
    finally:
        for s in subs:
            s.close()
    for k in range(5):
        _same_reg(recs[k], single[k], f"submap {k}")
        _same_reg(recs2[k], single[k], f"submap {k} (refining job)")
        _same_icp(refined[k], single_ref[k], f"submap {k}")
    print("final inliers against the submaps around 4, 6, 8, 10, 12:", [len(r["final_inliers"]) for r in single], "best", best)
    assert best == best2 == api.best_candidate(single) and single[2]["valid"]


def test_place_index_takes_a_submap(h4, traj):
    from quatro_amd import lib as ql
    _, poses, kfs, vox = traj
    ids, rel, _ = _window(poses, vox, MID, 3)
    with h4.merge_keyframes([kfs[i] for i in ids], rel) as sub, h4.place_index(4) as ix:
        assert ix.add(sub) == 0
        want = h4.place_describe(sub.fetch(ql.KF_VOX), slot=1)
        assert np.array_equal(_bits(ix.fetch(0)), _bits(want)) and np.array_equal(_bits(want), _bits(pr.describe(sub.fetch(ql.KF_VOX))))
        assert [m["id"] for m in ix.query(kfs[MID], 3)] == [0] and [m["id"] for m in ix.query(sub, 1)] == [0]


# ---- the contract's edges -----------------------------------------------------------------------------------------------
def _merge_rc(h, members, poses, K, fp, slot=0):
    arr = (C.c_void_p * max(len(members), 1))(*members)
    out = C.c_void_p(77)
    p = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64).ctypes.data
    rc = h._lib.qtr_keyframe_merge(h._h, slot, arr, p, K, None if fp is None else C.byref(fp), C.byref(out))
    return rc, out.value


def test_capacity_error_leaves_the_slot_usable():
    """Members whose voxels add up beyond max_points: QTR_ERR_CAPACITY naming both numbers, nothing enqueued — a registration
    on the slot afterwards is bit-identical to one made before.  (A handle of its own, sized so that two members overflow.)"""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, _ = synth.kitti64_pair(1)
    cap = (max(s.shape[0], t.shape[0]) + 1023) // 1024 * 1024
    h = ql.Handle(0, max_points=cap, max_voxels=cap)
    try:
        fp = ql.default_frontend_params(seed=1)
        before = h.register_pair(s, t, fp)
        ks, kt = h.keyframe(s), h.keyframe(t)
        n = ks.info["n_voxels"]
        K = h.limits.max_points // n + 1
        assert 2 <= K <= 64
        with h.merge_keyframes([ks] * (K - 1)) as ok:  # (just below the limit still merges)
            assert ok.info["n_points"] == (K - 1) * n
        with pytest.raises(ql.QuatroHipError) as e:
            h.merge_keyframes([ks] * K)
        assert e.value.code == ql.QTR_ERR_CAPACITY and str(K * n) in str(e.value) and str(h.limits.max_points) in str(e.value)
        rc, out = _merge_rc(h, [ks._kf.value] * K, None, K, fp)
        assert rc == ql.QTR_ERR_CAPACITY and out is None
        _same_reg(h.register_pair(s, t, fp), before, "register_pair after the refused merge")
        _same_reg(h.register_keyframes(ks, kt, fp), before, "register_keyframes after the refused merge")
    finally:
        h.close()


def test_bad_arguments_are_refused_before_anything_runs(h4, traj):
    from quatro_amd import lib as ql
    _, poses, kfs, vox = traj
    fp, bad = ql.default_frontend_params(), ql.QTR_ERR_BAD_ARG
    m = [kfs[0]._kf.value, kfs[1]._kf.value]
    eye2 = np.stack([np.eye(4)] * 2)
    assert _merge_rc(h4, m, eye2, 0, fp) == (bad, None)
    assert _merge_rc(h4, m, eye2, -3, fp) == (bad, None)
    assert _merge_rc(h4, [m[0]] * 65, None, 65, fp) == (bad, None)
    assert _merge_rc(h4, m, eye2, 2, None) == (bad, None)
    assert _merge_rc(h4, [m[0], None], eye2, 2, fp) == (bad, None)
    assert _merge_rc(h4, m, eye2, 2, fp, slot=9) == (bad, None)
    arr = (C.c_void_p * 2)(*m)
    assert h4._lib.qtr_keyframe_merge(h4._h, 0, arr, None, 2, C.byref(fp), None) == bad
    for k in range(12):
        for v in (np.nan, np.inf):
            p = eye2.copy()
            p[1].reshape(16)[k] = v
            assert _merge_rc(h4, m, p, 2, fp) == (bad, None), (k, v)
            assert "non-finite" in h4.last_error()
    p = eye2.copy()
    p[1][3] = [np.nan, np.inf, -np.inf, np.nan]  # row 3 is ignored
    with h4.merge_keyframes([kfs[0], kfs[1]], p) as a, h4.merge_keyframes([kfs[0], kfs[1]], eye2) as b:
        _same_keyframe(a, b, "row 3")
    other = ql.Handle(0)
    try:
        with other.keyframe(vox[0]) as foreign:
            assert _merge_rc(h4, [m[0], foreign._kf.value], eye2, 2, fp) == (bad, None)
            assert "another handle" in h4.last_error()
            assert _merge_rc(other, m, eye2, 2, fp) == (bad, None)
    finally:
        other.close()
    # the front end's own refusals are qtr_keyframe_create's
    with pytest.raises(ql.QuatroHipError) as e:
        h4.merge_keyframes([kfs[0]], None, ql.default_frontend_params(normal_radius=0.9))
    assert e.value.code == bad and "fpfh_radius" in str(e.value)
    with pytest.raises(ql.QuatroHipError) as e:  # 1 mm leaf: pcl::VoxelGrid's pass-through, and the cloud is within max_voxels
        h4.merge_keyframes([kfs[i] for i in range(8)], None, ql.default_frontend_params(voxel_size=0.001))
    assert e.value.code == ql.QTR_ERR_CAPACITY and "max_voxels" in str(e.value)
    # the slot is as usable as before
    with h4.merge_keyframes([kfs[0], kfs[1]], eye2) as a, h4.keyframe(sr.merge([vox[0], vox[1]])) as b:
        _same_keyframe(a, b, "after the refused calls")


def test_member_destroyed_and_recreated_between_merges(h4, traj):
    scans, poses, kfs, vox = traj
    rel = np.stack([np.eye(4), np.linalg.inv(poses[2]) @ poses[3]])
    tmp = h4.keyframe(scans[3])
    a = h4.merge_keyframes([kfs[2], tmp], rel)
    tmp.close()
    tmp = h4.keyframe(scans[3], slot=1)  # (very likely another allocation)
    b = h4.merge_keyframes([kfs[2], tmp], rel)
    tmp.close()
    try:
        _same_keyframe(a, b, "recreated member")
        with h4.keyframe(sr.merge([vox[2], vox[3]], rel)) as want:
            _same_keyframe(a, want, "the merge outlives its members")
    finally:
        a.close()
        b.close()


def test_two_threads_merge_from_the_same_members(h4, traj):
    _, poses, kfs, vox = traj
    wins = [_window(poses, vox, MID, 2), _window(poses, vox, MID + 1, 3)]
    single = [h4.merge_keyframes([kfs[i] for i in ids], rel) for ids, rel, _ in wins]
    out = [[None] * 4, [None] * 4]

    def work(t):
        ids, rel, _ = wins[t]
        for r in range(4):
            out[t][r] = h4.merge_keyframes([kfs[i] for i in ids], rel, None, 1 + t)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    try:
        for t in range(2):
            for r in range(4):
                _same_keyframe(out[t][r], single[t], f"thread {t} round {r}")
    finally:
        for k in single + out[0] + out[1]:
            if k is not None:
                k.close()


def test_device_memory_returns_when_submaps_are_destroyed(h4, traj):
    import torch
    _, poses, kfs, vox = traj
    ids, rel, _ = _window(poses, vox, MID, 2)
    members = [kfs[i] for i in ids]
    h4.merge_keyframes(members, rel).close()
    h4.merge_keyframes(members, rel, slot=1).close()  # (first use of both slots: their merge scratch is there before the measurement)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    made = [h4.merge_keyframes(members, rel, slot=i % 2) for i in range(30)]
    held = sum(k.info["device_bytes"] for k in made)
    free1, _ = torch.cuda.mem_get_info()
    for k in made:
        k.close()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    print(f"30 submaps hold {held} bytes; free memory {free0} -> {free1} -> {free2}")
    assert held > 30 * 176 * 12000 and free0 - free1 >= held // 2
    assert free2 >= free0 - (2 << 20), (free0, free1, free2)  # back to its level (the allocator works in 2 MiB pages)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _yaw(T):
    return float(np.arctan2(T[1, 0], T[0, 0]))


def _wrap(a):
    return float(np.arctan2(np.sin(a), np.cos(a)))


def test_close_loop_with_submaps_finds_the_revisited_keyframe(h4, qo, traj):
    """close_loop(k = 3, submap_half_width = 2) on the trajectory's revisit: the winner is the revisited keyframe (8, the
    middle of the path: the only one within 0.4 m of the query), its record equals the CPU oracle's register_pair on (the
    query's voxels, the host-merged cloud) under the project's bit-exact rule — sizes, clique, final inliers and every bit of
    T — and its distance from the ground truth inv(poses[8]) @ poses[17] is held against the oracle's own on the same input,
    times 1.5.  The margin covers nothing on the device (its T is the oracle's); it keeps the assertion meaningful should the
    scene be regenerated.  The oracle on kitti64_trajectory(0, 17, 1.0): 394 final inliers against the submap around 8 (369
    around 7, 386 around 9), translation error 0.0065 m, yaw error 1.96e-4 rad."""
    from quatro_amd import api
    from quatro_amd import lib as ql
    _, poses, kfs, vox = traj
    fp = ql.default_frontend_params(seed=0)
    with h4.place_index(N_SCANS) as ix:
        for kf in kfs[:N_SCANS]:
            ix.add(kf)
        made = []
        merge = h4.merge_keyframes
        try:
            h4.merge_keyframes = lambda *a, **kw: made.append(merge(*a, **kw)) or made[-1]  # (to see what becomes of the temporaries)
            r = api.close_loop(h4, ix, kfs, kfs[QUERY], 3, fp=fp, poses=poses, submap_half_width=2)
        finally:
            del h4.merge_keyframes
        plain = api.close_loop(h4, ix, kfs, kfs[QUERY], 3, fp=fp)
    ids = [m["id"] for m in r["matches"]]
    assert len(made) == 3 and all(not k._kf for k in made)  # destroyed after the job
    assert ids == [m["id"] for m in plain["matches"]] and len(r["records"]) == 3
    for c, rec in zip(ids, r["records"]):
        _, _, cat = _window(poses, vox, c, 2)
        o = qo.register_pair(vox[QUERY], cat, seed=0)
        Tgt = np.linalg.inv(poses[c]) @ poses[QUERY]
        err = (abs(_wrap(_yaw(rec["T"]) - _yaw(Tgt))), float(np.linalg.norm(rec["T"][:3, 3] - Tgt[:3, 3])))
        err_o = (abs(_wrap(_yaw(o["T"]) - _yaw(Tgt))), float(np.linalg.norm(o["T"][:3, 3] - Tgt[:3, 3])))
        print(f"candidate {c}: final inliers {len(rec['final_inliers'])} (oracle {o['final_inliers'].size}), yaw error "
              f"{err[0]:.3e} rad (oracle {err_o[0]:.3e}), translation error {err[1]:.4f} m (oracle {err_o[1]:.4f})")
        assert (rec["n_src"], rec["n_tgt"], rec["L"]) == (o["n_src"], o["n_tgt"], o["L"]), c
        assert rec["valid"] == o["valid"] and np.array_equal(rec["clique"], o["clique"]), c
        assert np.array_equal(rec["final_inliers"], o["final_inliers"]) and np.array_equal(rec["T"], o["T"]), c
        assert err[0] <= 1.5 * err_o[0] and err[1] <= 1.5 * err_o[1], (c, err, err_o)
    assert r["best_id"] == MID and ids[r["best"]] == MID, (ids, [len(x["final_inliers"]) for x in r["records"]])


def test_cpp_submap_demo_prints_the_python_paths_transform(h4, traj, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    scans, poses, _, _ = traj
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "submap_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "submap_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    ids = [MID - 1, MID, MID + 1]
    rel = np.stack([np.linalg.inv(poses[MID]) @ poses[i] for i in ids])
    pose_file = str(tmp_path / "poses.bin")
    rel.astype(np.float64).tofile(pose_file)
    files = []
    for i in [QUERY] + ids:
        files.append(str(tmp_path / f"{i}.bin"))
        synth.save_kitti_bin(files[-1], scans[i])
    out = subprocess.run([exe, pose_file] + files, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    loaded = [h4.keyframe(ql.read_kitti_bin(f)) for f in files]
    try:
        with h4.merge_keyframes(loaded[1:], rel) as sub:
            r = h4.register_keyframes(loaded[0], sub, ql.default_frontend_params())
            assert out[0] == f"submap members 3 n_points {sub.info['n_points']} n_voxels {sub.info['n_voxels']}", out
        assert out[1] == f"valid {int(r['valid'])} n_src {r['n_src']} n_tgt {r['n_tgt']} L {r['L']}", out
        T = np.array([int(w, 16) for ln in out[2:6] for w in ln.split()], dtype=np.uint64)
        assert np.array_equal(T.view(np.float64).reshape(4, 4), r["T"]) and r["valid"], out
    finally:
        for kf in loaded:
            kf.close()
