"""ICP refinement on the MI355X (qtr_icp / qtr_refine_pair): bit-parity with the host restatement of the loop
(tests/icp_ref/icp_ref.cpp), the end-to-end gain over Quatro's 4-DoF result on tilted scans, the edge cases and the
documented statuses, device memory, two slots from two threads, and no side effect on the registration path."""
import threading

import numpy as np
import pytest

import icp_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vox_pair(hip):
    from quatro_amd import synth
    s, t, Tgt = synth.kitti64_pair(2)
    vs, vt = hip.voxelize(s, 0.3), hip.voxelize(t, 0.3)
    nrm, _ = hip.fpfh(vt, 0.5, 0.5)
    return vs, vt, nrm, Tgt


def _perturbed(Tgt):
    return Tgt @ R.rigid(R.rot(0.012, -0.009, 0.015), [0.25, -0.3, 0.08])


@pytest.mark.parametrize("method", [0, 1])
def test_icp_is_bit_equal_to_the_restatement_every_iteration(hip, vox_pair, method):
    from quatro_amd import lib as ql
    vs, vt, nrm, Tgt = vox_pair
    G = _perturbed(Tgt)
    prm = ql.default_icp_params(method=method, max_iterations=40)
    g = hip.icp(vs, vt, nrm, G, prm)
    trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    corr_last = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
    o = R.run(vs, vt, nrm, G, max_iter=40, method=method)
    assert g["valid"] and g["iterations"] >= 3
    assert (g["iterations"], g["stop_reason"], g["n_corr"]) == (o["iterations"], o["stop_reason"], o["n_corr"])
    assert np.array_equal(g["T"], o["T"]) and g["fitness"] == o["fitness"] and g["rmse"] == o["rmse"]
    assert np.array_equal(trace, o["trace"])
    assert np.array_equal(corr_last, o["corr"])
    # every iteration's correspondence set: the loop cut after k updates leaves iteration k's set behind
    for k in range(1, g["iterations"]):
        gk = hip.icp(vs, vt, nrm, G, ql.default_icp_params(method=method, max_iterations=k))
        ok = R.run(vs, vt, nrm, G, max_iter=k, method=method, corr_iter=k - 1)
        assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_CORR, np.int32), ok["corr"]), k
        assert np.array_equal(gk["T"], o["trace"][k - 1, :16].reshape(4, 4)), k
    # a second run gives the same bits
    g2 = hip.icp(vs, vt, nrm, G, prm)
    assert np.array_equal(g2["T"], g["T"]) and np.array_equal(hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18),
                                                             trace)


def test_icp_normals_computed_on_the_device_match_the_fpfh_stage(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, nrm, Tgt = vox_pair
    prm = ql.default_icp_params(normal_radius=0.5)
    a = hip.icp(vs, vt, nrm, _perturbed(Tgt), prm)
    b = hip.icp(vs, vt, None, _perturbed(Tgt), prm)
    assert np.array_equal(a["T"], b["T"]) and a["iterations"] == b["iterations"]


@pytest.mark.parametrize("pair_id", [0, 1])
def test_refine_pair_recovers_roll_and_pitch_after_quatro(hip, pair_id):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, Tgt = synth.kitti64_pair_16k(pair_id)
    tilt = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
    t = R.apply(tilt, t)
    Tgt = tilt @ Tgt
    r = hip.register_pair(s, t, ql.default_frontend_params(seed=pair_id))
    e0 = R.rot_err_deg(r["T"], Tgt)
    assert e0 >= 1.5, e0
    g = hip.refine_pair(None, ql.default_icp_params())
    e1 = R.rot_err_deg(g["T"], Tgt)
    print(f"pair {pair_id}: quatro {e0:.3f} deg -> icp {e1:.3f} deg, {np.linalg.norm(g['T'][:3, 3] - Tgt[:3, 3]):.3f} m, "
          f"{g['iterations']} iterations, stop {g['stop_reason']}")
    # (measured: 1.805 -> 0.094 deg / 3.9 cm and 1.875 -> 0.076 deg / 3.2 cm; the bounds keep a factor ~2.5)
    assert g["valid"] and e1 <= 0.25 and e1 <= e0 / 3
    assert np.linalg.norm(g["T"][:3, 3] - Tgt[:3, 3]) <= 0.08
    # the slot's clouds are the caller's source and target: the same loop through qtr_icp on the fetched voxel clouds
    vs = hip.debug_fetch(ql.DBG_VOX_SRC, np.float32).reshape(-1, 4)
    vt = hip.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
    p = hip.refine_pair(None, ql.default_icp_params(method=ql.ICP_POINT_TO_POINT))
    q = hip.icp(vs, vt, None, r["T"], ql.default_icp_params(method=ql.ICP_POINT_TO_POINT))
    assert np.array_equal(p["T"], q["T"])


def test_refine_pair_leaves_the_registration_path_untouched(hip):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, _ = synth.kitti64_pair(1)
    fp = ql.default_frontend_params(seed=1)
    a = hip.register_pair(s, t, fp)
    hip.refine_pair(None, ql.default_icp_params())
    b = hip.register_pair(s, t, fp)
    for k in ("T", "clique", "final_inliers"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["cost"], a["n_src"], a["n_tgt"], a["L"]) == (b["cost"], b["n_src"], b["n_tgt"], b["L"])


def test_icp_edge_cases_and_statuses(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, nrm, Tgt = vox_pair
    # a single plane: degenerate, valid = 0, T finite
    rng = np.random.default_rng(3)
    plane = R.f4(np.c_[rng.random((3000, 2)) * 20, np.zeros(3000)])
    g = hip.icp(plane, plane, None, R.rigid(np.eye(3), [0.1, 0.1, 0.05]))
    assert g["stop_reason"] == ql.ICP_STOP_DEGENERATE and not g["valid"] and np.isfinite(g["T"]).all()
    # kilometres off: too few correspondences, T == guess
    far = R.rigid(np.eye(3), [3000.0, -2000.0, 0.0])
    g = hip.icp(vs, vt, nrm, far)
    assert g["stop_reason"] == ql.ICP_STOP_TOO_FEW and not g["valid"] and np.array_equal(g["T"], far)
    # NaN points in either cloud are ignored
    G = _perturbed(Tgt)
    base = hip.icp(vs, vt, nrm, G)
    vs2, vt2, n2 = vs.copy(), vt.copy(), nrm.copy()
    vs2[::97, :3] = np.nan
    vt2[5::89, 0] = np.nan
    g = hip.icp(vs2, vt2, n2, G)
    o = R.run(vs2, vt2, n2, G)
    assert g["valid"] and np.array_equal(g["T"], o["T"]) and np.abs(g["T"] - base["T"]).max() < 0.05
    # empty clouds: QTR_OK, valid = 0, T = guess
    e = hip.icp(vs[:0], vt, nrm, G)
    assert not e["valid"] and np.array_equal(e["T"], G)
    e = hip.icp(vs, vt[:0], nrm[:0], G)
    assert not e["valid"] and np.array_equal(e["T"], G)
    # bad arguments and capacity
    for kw in ({"max_correspondence_distance": 0.0}, {"max_correspondence_distance": float("nan")},
               {"max_iterations": 0}, {"method": 7}, {"transformation_epsilon": -1.0}, {"min_correspondences": -1}):
        with pytest.raises(ql.QuatroHipError) as ei:
            hip.icp(vs, vt, nrm, G, ql.default_icp_params(**kw))
        assert ei.value.code == ql.QTR_ERR_BAD_ARG, kw
    bad = G.copy()
    bad[0, 3] = np.inf
    with pytest.raises(ql.QuatroHipError) as ei:
        hip.icp(vs, vt, nrm, bad)
    assert ei.value.code == ql.QTR_ERR_BAD_ARG
    res = ql.IcpResult()
    prm = ql.default_icp_params()
    assert hip._lib.qtr_icp(hip._h, 0, None, 5, vt.ctypes.data, vt.shape[0], None, None, prm, res, 0) == ql.QTR_ERR_BAD_ARG
    assert hip._lib.qtr_icp(hip._h, 0, vs.ctypes.data, -1, vt.ctypes.data, vt.shape[0], None, None, prm, res,
                            0) == ql.QTR_ERR_BAD_ARG
    assert hip._lib.qtr_icp(hip._h, 9, vs.ctypes.data, 10, vt.ctypes.data, 10, None, None, prm, res, 0) == ql.QTR_ERR_BAD_ARG
    small = ql.Handle(0, max_points=8192, max_voxels=4096, max_corr=1024)
    try:
        with pytest.raises(ql.QuatroHipError) as ei:
            small.icp(vs[:5000], vt[:100], None, G)
        assert ei.value.code == ql.QTR_ERR_CAPACITY
    finally:
        small.close()
    # refine_pair on a slot whose last call was not a registration
    with pytest.raises(ql.QuatroHipError) as ei:
        hip.refine_pair(None, prm)
    assert ei.value.code == ql.QTR_ERR_BAD_ARG


def test_icp_device_memory_matches_host_memory(hip, vox_pair):
    import torch
    from quatro_amd import lib as ql
    vs, vt, nrm, Tgt = vox_pair
    G = _perturbed(Tgt)
    for method in (0, 1):
        prm = ql.default_icp_params(method=method)
        a = hip.icp(vs, vt, nrm, G, prm)
        d = hip.icp(torch.from_numpy(vs).cuda(), torch.from_numpy(vt).cuda(), torch.from_numpy(nrm).cuda(), G, prm)
        assert np.array_equal(a["T"], d["T"]) and a["iterations"] == d["iterations"]
    a = hip.icp(vs, vt, None, G)
    d = hip.icp(torch.from_numpy(vs).cuda(), torch.from_numpy(vt).cuda(), None, G)
    assert np.array_equal(a["T"], d["T"])


def test_icp_two_slots_from_two_threads_match_sequential_calls(vox_pair):
    from quatro_amd import lib as ql
    vs, vt, nrm, Tgt = vox_pair
    h = ql.Handle(0, n_slots=2)
    try:
        guesses = [_perturbed(Tgt), Tgt @ R.rigid(R.rot(-0.01, 0.01, -0.02), [-0.2, 0.3, -0.05])]
        seq = [h.icp(vs, vt, nrm, guesses[k], ql.default_icp_params(method=k), slot=k)["T"] for k in (0, 1)]
        out = [None, None]

        def work(k):
            for _ in range(3):
                out[k] = h.icp(vs, vt, nrm, guesses[k], ql.default_icp_params(method=k), slot=k)["T"]

        th = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert np.array_equal(out[0], seq[0]) and np.array_equal(out[1], seq[1])
    finally:
        h.close()


def test_icp_python_class_over_the_handle(hip, vox_pair):
    from quatro_amd import api
    vs, vt, nrm, Tgt = vox_pair
    icp = api.IterativeClosestPoint(handle=hip)
    icp.setInputSource(vs)
    icp.setInputTarget(vt)
    icp.setMaxCorrespondenceDistance(1.0)
    icp.setMaximumIterations(30)
    icp.setTransformationEpsilon(1e-7)
    icp.setEuclideanFitnessEpsilon(1e-6)
    out = icp.align(_perturbed(Tgt))
    assert icp.hasConverged() and out.shape == vs.shape and icp.getFitnessScore() < 0.5
    assert np.array_equal(icp.getFinalTransformation(), hip.icp(vs, vt, None, _perturbed(Tgt))["T"])


@pytest.mark.parametrize("method", ["point_to_plane", "point_to_point"])
def test_cpp_icp_demo_gives_the_python_paths_bits(hip, vox_pair, tmp_path, method):
    import os
    import subprocess
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "icp_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "icp_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    vs, vt, _, Tgt = vox_pair
    G = _perturbed(Tgt)
    vs.tofile(str(tmp_path / "s.bin"))
    vt.tofile(str(tmp_path / "t.bin"))
    (tmp_path / "g.txt").write_text(" ".join(repr(float(x)) for x in G.reshape(-1)))
    out = subprocess.run([exe, str(tmp_path / "s.bin"), str(tmp_path / "t.bin"), str(tmp_path / "g.txt"), method],
                         capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    T = np.array([int(w, 16) for ln in out[1:5] for w in ln.split()], dtype=np.uint64).view(np.float64).reshape(4, 4)
    m = ql.ICP_POINT_TO_PLANE if method == "point_to_plane" else ql.ICP_POINT_TO_POINT
    g = hip.icp(vs, vt, None, G, ql.default_icp_params(method=m))
    assert np.array_equal(T, g["T"]), (out, g["T"])
