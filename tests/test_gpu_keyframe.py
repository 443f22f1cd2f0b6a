"""Keyframes on the MI355X (qtr_keyframe_create / qtr_register_keyframes / qtr_submit_batch_keyframes): every record
bit-equal to the raw-scan entry's — single pairs, cross pairs, the three refinements, batches with and without ICP, a
one-to-many job, an odometry chain — plus the edge cases of the contract.  Everything goes through the C ABI binding."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import icp_restate as R

pytestmark = pytest.mark.gpu

TILT = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")
REG_INT_KEYS = ("status", "valid", "gnc_iters", "max_core", "n_edges", "n_card", "n_src", "n_tgt", "L", "n_rot_inliers")


def _tilted(pair):
    s, t, Tgt = pair
    return s, R.apply(TILT, t), TILT @ Tgt


@pytest.fixture(scope="module")
def pairs():
    """The ten pairs of tests/test_gpu_icp_batch.py: kitti64_pair(0..4) and kitti64_pair_16k(0..4), every other one with
    its target tilted; (source, target, seed)."""
    from quatro_amd import synth
    out = []
    for k in range(5):
        for big in (False, True):
            p = (synth.kitti64_pair_16k if big else synth.kitti64_pair)(k)
            if (k + big) % 2 == 0:
                p = _tilted(p)
            out.append((p[0], p[1], 10 * k + big))
    return out


CROSS = [(i, (i + 3) % 10) for i in range(10)]  # source of pair i against the target of pair j, i != j


@pytest.fixture(scope="module")
def h2():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


@pytest.fixture(scope="module")
def kfs(h2, pairs):
    """(source keyframe, target keyframe) of every pair, each scan's front end run once."""
    out = [(h2.keyframe(s), h2.keyframe(t)) for s, t, _ in pairs]
    yield out
    for a, b in out:
        a.close()
        b.close()


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _call(fn, *a, **kw):
    """a registration's dict, or {"status": code} when the binding raised (capacity, bad argument)"""
    from quatro_amd import lib as ql
    try:
        return fn(*a, **kw)
    except ql.QuatroHipError as e:
        return {"status": e.code}


def _same_reg(a, b, what=""):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    if "T" not in a and "T" not in b:
        return
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _slot_state(h, slot=0):
    from quatro_amd import lib as ql
    return (h.debug_fetch(ql.DBG_CORR, np.int32, slot), h.debug_fetch(ql.DBG_VOX_SRC, np.float32, slot),
            h.debug_fetch(ql.DBG_VOX_TGT, np.float32, slot))


VARIANTS = [({}, "demo"), ({"use_tuple_test": 0}, "demo"), ({"use_crosscheck": 0}, "demo"), ({}, "default")]


@pytest.mark.parametrize("fp_kw,prm_name", VARIANTS)
def test_single_pair_is_bit_identical_to_register_pair(h2, pairs, kfs, fp_kw, prm_name):
    from quatro_amd import lib as ql
    prm = ql.demo_params() if prm_name == "demo" else ql.default_params()
    n_ok = 0
    for i, ((s, t, seed), (ks, kt)) in enumerate(zip(pairs, kfs)):
        fp = ql.default_frontend_params(seed=seed, **fp_kw)
        a = _call(h2.register_pair, s, t, fp, prm)
        sa = _slot_state(h2)
        b = _call(h2.register_keyframes, ks, kt, fp, prm)
        sb = _slot_state(h2)
        _same_reg(b, a, f"pair {i} {fp_kw} {prm_name}")
        for x, y, name in zip(sa, sb, ("corr", "vox_src", "vox_tgt")):
            assert np.array_equal(_bits(x), _bits(y)), (i, name)
        assert np.array_equal(_bits(sb[1]), _bits(ks.fetch(ql.KF_VOX)).reshape(-1)), i
        assert np.array_equal(_bits(sb[2]), _bits(kt.fetch(ql.KF_VOX)).reshape(-1)), i
        n_ok += a["status"] == ql.QTR_OK and bool(a.get("valid"))
        st = h2.stage_times()
        assert st["voxelize"] == 0 and st["fpfh"] == 0 and st["match"] > 0, st
    print(f"{fp_kw} {prm_name}: {n_ok} of 10 raw-scan registrations valid")
    if not fp_kw and prm_name == "demo":
        assert n_ok >= 8  # (the fixture's condition, on the raw-scan side)


def test_stored_normals_and_descriptors_are_qtr_fpfh_of_the_stored_voxels(h2, pairs, kfs):
    """The relation tests/test_gpu_gicp.py relies on for the normals (the FPFH stage of the whole path equals qtr_fpfh on
    the voxel cloud), here for what a keyframe stores; the sequential mean within the rounding bound of a float sum."""
    from quatro_amd import lib as ql
    for i, (ks, kt) in enumerate(kfs):
        for kf in (ks, kt):
            vox = kf.fetch(ql.KF_VOX)
            fp = ql.default_frontend_params()
            nrm, desc = h2.fpfh(vox, fp.normal_radius, fp.fpfh_radius, slot=1)
            same_n = np.array_equal(_bits(nrm), _bits(kf.fetch(ql.KF_NORMALS)))
            same_d = np.array_equal(_bits(desc), _bits(kf.fetch(ql.KF_FPFH)))
            print(f"pair {i}: {vox.shape[0]} voxels, normals equal {same_n}, descriptors equal {same_d}")
            assert same_n and same_d, i
            info = kf.info
            assert info["n_voxels"] == vox.shape[0] and info["passed_through"] == 0
            assert info["device_bytes"] <= 256 * info["n_voxels"] + 4096, info
            m = kf.fetch(ql.KF_MEAN)
            # a float accumulator over the points in order: its error is at most n * 2^-24 * max|x| (sequential summation)
            exact = vox[:, :3].astype(np.float64).mean(axis=0)
            bound = vox.shape[0] * 2.0 ** -24 * np.abs(vox[:, :3]).max()
            assert np.abs(m[:3] - exact).max() <= bound, (i, m, exact, bound)


def test_cross_pairs_are_bit_identical(h2, pairs, kfs):
    from quatro_amd import lib as ql
    st = []
    for i, j in CROSS:
        fp = ql.default_frontend_params(seed=100 + i)
        a = _call(h2.register_pair, pairs[i][0], pairs[j][1], fp)
        ca = _slot_state(h2)[0]
        b = _call(h2.register_keyframes, kfs[i][0], kfs[j][1], fp)
        _same_reg(b, a, f"cross {i}x{j}")
        assert np.array_equal(ca, _slot_state(h2)[0]), (i, j)
        st.append((a["status"], bool(a.get("valid"))))
    print("cross pairs (status, valid):", st)


@pytest.mark.parametrize("method", [0, 1, 2])
def test_refine_pair_after_register_keyframes(h2, pairs, kfs, method):
    from quatro_amd import lib as ql
    icp = ql.default_icp_params(method=method)
    for i in (0, 1, 2, 3, 5):
        s, t, seed = pairs[i]
        fp = ql.default_frontend_params(seed=seed)
        h2.register_pair(s, t, fp)
        a = h2.refine_pair(None, icp)
        h2.register_keyframes(kfs[i][0], kfs[i][1], fp)
        b = h2.refine_pair(None, icp)
        _same_icp(b, a, f"pair {i} method {method}")


@pytest.mark.parametrize("n_slots,icp_kw", [(16, None), (16, {}), (4, None), (4, {"max_iterations": 4})])
def test_batched_keyframes_are_bit_identical_to_the_raw_scan_batch(pairs, n_slots, icp_kw):
    from quatro_amd import lib as ql
    raw = list(pairs) + [(pairs[i][0], pairs[j][1], 100 + i) for i, j in CROSS]
    hb = ql.Handle(0, n_slots=n_slots)
    try:
        src = [hb.keyframe(s, slot=i % n_slots) for i, (s, _, _) in enumerate(pairs)]
        tgt = [hb.keyframe(t, slot=(i + 1) % n_slots) for i, (_, t, _) in enumerate(pairs)]
        kp = [(src[i], tgt[i], pairs[i][2]) for i in range(10)] + [(src[i], tgt[j], 100 + i) for i, j in CROSS]
        if icp_kw is None:
            want = hb.register_batch(raw)
            got = hb.register_batch_keyframes(kp)
            again = hb.register_batch_keyframes(kp)
        else:
            icp = ql.default_icp_params(**icp_kw)
            want, want_ref = hb.register_batch_refine(raw, icp=icp)
            got, got_ref = hb.register_batch_keyframes(kp, icp=icp)
            for i, (a, b) in enumerate(zip(got_ref, want_ref)):
                _same_icp(a, b, f"refined {i}")
            again = got
            with pytest.raises(ql.QuatroHipError) as e:  # (as after qtr_submit_batch)
                hb.refine_pair(None, icp)
            assert e.value.code == ql.QTR_ERR_BAD_ARG
    finally:
        hb.close()
    assert len(got) == 20
    for i, (a, b, c) in enumerate(zip(got, want, again)):
        _same_reg(a, b, f"record {i}")
        _same_reg(c, b, f"record {i}, second job")
    assert sum(r["status"] == ql.QTR_OK and r["valid"] for r in want[:10]) >= 8


def test_one_to_many_job_equals_five_register_pair_calls():
    from quatro_amd import api, synth
    from quatro_amd import lib as ql
    P = [synth.kitti64_pair_16k(k) for k in range(5)]
    query = P[2][0]
    fp = ql.default_frontend_params(seed=5)
    hb = ql.Handle(0, n_slots=4)
    try:
        raw = [hb.register_pair(query, P[k][1], fp) for k in range(5)]
        with hb.keyframe(query) as kq:
            cands = [hb.keyframe(P[k][1], slot=k % 4) for k in range(5)]
            recs, best = api.register_one_to_many(hb, kq, cands, fp)
            recs2, refined, best2 = api.register_one_to_many(hb, kq, cands, fp, icp=ql.default_icp_params())
            for c in cands:
                c.close()
    finally:
        hb.close()
    for k in range(5):
        _same_reg(recs[k], raw[k], f"candidate {k}")
        _same_reg(recs2[k], raw[k], f"candidate {k} (refining job)")
    n_final = [len(r["final_inliers"]) if r["valid"] else -1 for r in raw]
    print("one-to-many: n_final of the raw-scan records", n_final, "best", best)
    assert raw[2]["valid"] and best == best2 == int(np.argmax(n_final)) and max(n_final) >= 0
    assert refined[best]["status"] == ql.QTR_OK


def test_odometry_chain_runs_each_front_end_once(h2):
    from quatro_amd import synth
    from quatro_amd import lib as ql
    step = R.rigid(R.rot(0.0, 0.0, 0.04), [0.8, 0.1, 0.0])
    scans = [synth.kitti64_pair_16k(1)[0]]
    for _ in range(4):
        scans.append(R.apply(step, scans[-1]))
    chain = [h2.keyframe(s) for s in scans]
    try:
        for kf in chain:
            assert kf.info["device_bytes"] <= 256 * kf.info["n_voxels"] + 4096 and kf.info["n_points"] == scans[0].shape[0]
        for k in range(4):
            fp = ql.default_frontend_params(seed=k)
            a = _call(h2.register_pair, scans[k], scans[k + 1], fp)
            b = _call(h2.register_keyframes, chain[k], chain[k + 1], fp)
            _same_reg(b, a, f"step {k}")
            assert a["status"] == ql.QTR_OK and a["valid"], k
    finally:
        for kf in chain:
            kf.close()


def test_bad_arguments_and_failing_scans(h2, pairs, kfs):
    from quatro_amd import lib as ql
    ks, kt = kfs[1]
    for kw in ({"voxel_size": 0.31}, {"normal_radius": 0.45}, {"fpfh_radius": 0.8}):
        with pytest.raises(ql.QuatroHipError) as e:
            h2.register_keyframes(ks, kt, ql.default_frontend_params(**kw))
        assert e.value.code == ql.QTR_ERR_BAD_ARG, kw
        with pytest.raises(ql.QuatroHipError) as e:
            h2.register_batch_keyframes([(ks, kt, 1)], ql.default_frontend_params(**kw))
        assert e.value.code == ql.QTR_ERR_BAD_ARG, kw
    other = ql.Handle(0)
    try:
        for fn in (other.register_keyframes, lambda a, b: other.register_batch_keyframes([(a, b, 1)])):
            with pytest.raises(ql.QuatroHipError) as e:  # a keyframe of another handle
                fn(ks, kt)
            assert e.value.code == ql.QTR_ERR_BAD_ARG
        assert other._lib.qtr_keyframe_fetch(other._h, ks._kf, ql.KF_VOX, None, 0) < 0
        assert other._lib.qtr_wait(other._h) == ql.QTR_OK  # (nothing was enqueued)
    finally:
        other.close()
    # refined goes with icp; a job is refused whole
    fp, prm, icp = ql.default_frontend_params(), ql.demo_params(), ql.default_icp_params()
    descs = (ql.KfPairDesc * 1)(ql.KfPairDesc(ks._kf, kt._kf, 1, None, None, 0))
    res, ref = (ql.Result * 1)(), (ql.IcpResult * 1)()
    lib = h2._lib
    assert lib.qtr_submit_batch_keyframes(h2._h, descs, 1, C.byref(fp), C.byref(prm), None, res, ref) == ql.QTR_ERR_BAD_ARG
    assert lib.qtr_submit_batch_keyframes(h2._h, descs, 1, C.byref(fp), C.byref(prm), C.byref(icp), res, None) == ql.QTR_ERR_BAD_ARG
    descs[0].tgt = None
    assert lib.qtr_submit_batch_keyframes(h2._h, descs, 1, C.byref(fp), C.byref(prm), None, res, None) == ql.QTR_ERR_BAD_ARG
    assert lib.qtr_wait(h2._h) == ql.QTR_OK
    # scans that front_device refuses fail at creation with its codes
    with pytest.raises(ql.QuatroHipError) as e:
        h2.keyframe(np.zeros((0, 4), dtype=np.float32))
    assert e.value.code == ql.QTR_ERR_BAD_ARG and "empty point cloud" in str(e.value)
    big = np.zeros((100000, 4), dtype=np.float32)  # ~10^5 voxels at 0.3 m: over max_voxels = 65536
    big[:, :3] = np.random.default_rng(5).uniform(-100, 100, (100000, 3))
    with pytest.raises(ql.QuatroHipError) as e:
        h2.keyframe(big)
    assert e.value.code == ql.QTR_ERR_CAPACITY and "max_voxels" in str(e.value)
    with pytest.raises(ql.QuatroHipError) as e:
        h2.keyframe(np.zeros((300000, 4), dtype=np.float32))
    assert e.value.code == ql.QTR_ERR_CAPACITY and "max_points" in str(e.value)
    with pytest.raises(ql.QuatroHipError) as e:
        h2.keyframe(pairs[0][0], ql.default_frontend_params(normal_radius=0.9))
    assert e.value.code == ql.QTR_ERR_BAD_ARG
    # the handle is as usable as before
    s, t, seed = pairs[1]
    fp = ql.default_frontend_params(seed=seed)
    _same_reg(h2.register_keyframes(ks, kt, fp), h2.register_pair(s, t, fp), "after the refused calls")


def test_same_keyframe_on_both_sides_and_recreation(h2, pairs):
    from quatro_amd import lib as ql
    s = pairs[3][0]
    fp = ql.default_frontend_params(seed=9)
    want = h2.register_pair(s, s, fp)
    kf = h2.keyframe(s)
    got = h2.register_keyframes(kf, kf, fp)
    _same_reg(got, want, "kf_src == kf_tgt")
    assert got["valid"] and np.abs(got["T"] - np.eye(4)).max() < 1e-6
    kf.close()
    kf.close()  # (idempotent in the binding)
    with h2.keyframe(s, slot=1) as again:  # destroyed, another one created — from the other slot
        _same_reg(h2.register_keyframes(again, again, fp, slot=1), want, "recreated")


def test_two_threads_register_against_the_same_target_keyframe(h2, pairs, kfs):
    from quatro_amd import lib as ql
    kt = kfs[5][1]
    fps = [ql.default_frontend_params(seed=31), ql.default_frontend_params(seed=32)]
    srcs = [kfs[5][0], kfs[7][0]]
    single = [_call(h2.register_keyframes, srcs[k], kt, fps[k]) for k in range(2)]
    out = [[None] * 6, [None] * 6]

    def work(k):
        for r in range(6):
            out[k][r] = _call(h2.register_keyframes, srcs[k], kt, fps[k], None, k)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for k in range(2):
        for r in range(6):
            _same_reg(out[k][r], single[k], f"thread {k} round {r}")


def test_no_state_crosses_between_the_two_paths(h2, pairs, kfs):
    from quatro_amd import lib as ql
    s, t, seed = pairs[9]
    fp = ql.default_frontend_params(seed=seed)
    fresh = ql.Handle(0)
    try:
        want = fresh.register_pair(s, t, fp)
        want_corr = fresh.debug_fetch(ql.DBG_CORR, np.int32)
    finally:
        fresh.close()
    h2.register_keyframes(kfs[2][0], kfs[4][1], ql.default_frontend_params(seed=1, use_crosscheck=0))
    got = h2.register_pair(s, t, fp)
    _same_reg(got, want, "register_pair after register_keyframes")
    assert np.array_equal(want_corr, h2.debug_fetch(ql.DBG_CORR, np.int32))


def test_device_memory_returns_when_keyframes_are_destroyed(h2, pairs):
    import torch
    s = pairs[1][0]
    h2.keyframe(s).close()  # (first use: whatever the runtime keeps for itself is there before the measurement)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    made = [h2.keyframe(s, slot=i % 2) for i in range(40)]
    held = sum(k.info["device_bytes"] for k in made)
    free1, _ = torch.cuda.mem_get_info()
    for k in made:
        k.close()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    print(f"40 keyframes hold {held} bytes; free memory {free0} -> {free1} -> {free2}")
    assert held > 40 * 176 * 8000 and free0 - free1 >= held // 2
    assert free2 >= free0 - (2 << 20), (free0, free1, free2)  # back to its level (the allocator works in 2 MiB pages)


def test_destroying_the_handle_frees_forgotten_keyframes(pairs):
    import torch
    from quatro_amd import lib as ql
    torch.cuda.synchronize()
    h = ql.Handle(0)
    h.close()
    free0, _ = torch.cuda.mem_get_info()
    h = ql.Handle(0)
    made = [h.keyframe(pairs[1][0]) for _ in range(20)]
    assert len(made) == 20
    h.close()  # (the keyframes were never closed)
    free1, _ = torch.cuda.mem_get_info()
    assert free1 >= free0 - (2 << 20), (free0, free1)


def test_cpp_keyframe_demo_prints_the_python_paths_transforms(h2, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "keyframe_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "keyframe_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    step = R.rigid(R.rot(0.0, 0.0, 0.04), [0.8, 0.1, 0.0])
    scans = [synth.kitti64_pair(1)[0]]
    for _ in range(2):
        scans.append(R.apply(step, scans[-1]))
    files = []
    for k, sc in enumerate(scans):
        files.append(str(tmp_path / f"{k}.bin"))
        synth.save_kitti_bin(files[-1], sc)
    out = subprocess.run([exe] + files, capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    loaded = [ql.read_kitti_bin(f) for f in files]
    chain = [h2.keyframe(sc) for sc in loaded]
    try:
        for k in range(2):
            r = h2.register_keyframes(chain[k], chain[k + 1], ql.default_frontend_params(seed=k))
            T = np.array([int(w, 16) for ln in out[5 * k + 1:5 * k + 5] for w in ln.split()], dtype=np.uint64)
            assert np.array_equal(T.view(np.float64).reshape(4, 4), r["T"]), (k, out)
    finally:
        for kf in chain:
            kf.close()
