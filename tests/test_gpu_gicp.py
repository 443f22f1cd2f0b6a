"""Plane-to-plane (Generalized ICP) refinement on the MI355X, method QTR_ICP_PLANE_TO_PLANE through qtr_gicp / qtr_icp /
qtr_refine_pair / qtr_submit_batch_refine: bit-parity with the host restatement of the loop (tests/gicp_ref/gicp_ref.cpp)
at every iteration, the slot's own normals against explicit ones, the batched path against register + refine, device
memory, the statuses, the C++ wrapper, and the rotation error on tilted scans."""
import os
import subprocess

import numpy as np
import pytest

import gicp_restate as G
import icp_restate as R

pytestmark = pytest.mark.gpu

TILT = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same_icp(a, b, what=""):
    assert a.get("status", 0) == b.get("status", 0), what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _same_reg(a, b, what=""):
    assert a["status"] == b["status"], what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert _f64bits(a["cost"]) == _f64bits(b["cost"]), what
    assert (a["n_src"], a["n_tgt"], a["L"]) == (b["n_src"], b["n_tgt"], b["L"]), what


def _tilted(pair):
    s, t, Tgt = pair
    return s, R.apply(TILT, t), TILT @ Tgt


def _perturbed(Tgt):
    return Tgt @ R.rigid(R.rot(0.012, -0.009, 0.015), [0.25, -0.3, 0.08])


def _gicp_params(**kw):
    from quatro_amd import lib as ql
    return ql.default_icp_params(method=ql.ICP_PLANE_TO_PLANE, **kw)


def _handle(n_slots, **env):
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


@pytest.fixture(scope="module")
def vox_pair(hip):
    """kitti64_pair(2)'s voxel clouds with both normal sets from qtr_fpfh."""
    from quatro_amd import synth
    s, t, Tgt = synth.kitti64_pair(2)
    vs, vt = hip.voxelize(s, 0.3), hip.voxelize(t, 0.3)
    ns, _ = hip.fpfh(vs, 0.5, 0.5)
    nt, _ = hip.fpfh(vt, 0.5, 0.5)
    return vs, vt, ns, nt, Tgt


@pytest.fixture(scope="module")
def pairs():
    """The ten pairs of tests/test_gpu_icp_batch.py: kitti64_pair(0..4) and kitti64_pair_16k(0..4), every other one with
    its target tilted."""
    from quatro_amd import synth
    out = []
    for k in range(5):
        for big in (False, True):
            p = (synth.kitti64_pair_16k if big else synth.kitti64_pair)(k)
            if (k + big) % 2 == 0:
                p = _tilted(p)
            out.append((p[0], p[1], 10 * k + big))
    return out


def test_gicp_is_bit_equal_to_the_restatement_every_iteration(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    assert np.isnan(ns[:, :3]).any(1).sum() < ns.shape[0] // 2  # (most points have a normal; those without are skipped)
    G0 = _perturbed(Tgt)
    prm = _gicp_params(max_iterations=40)
    g = hip.gicp(vs, vt, ns, nt, G0, prm)
    trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    corr_last = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
    o = G.run(vs, ns, vt, nt, G0, max_iter=40)
    print(f"gicp: {g['iterations']} iterations, stop {g['stop_reason']}, {g['n_corr']} correspondences, "
          f"rot err {R.rot_err_deg(G0, Tgt):.4f} -> {R.rot_err_deg(g['T'], Tgt):.4f} deg")
    assert g["valid"] and g["iterations"] >= 3
    assert (g["iterations"], g["stop_reason"], g["n_corr"]) == (o["iterations"], o["stop_reason"], o["n_corr"])
    assert np.array_equal(g["T"], o["T"]) and g["fitness"] == o["fitness"] and g["rmse"] == o["rmse"]
    assert np.array_equal(trace, o["trace"])
    assert np.array_equal(corr_last, o["corr"])
    # every iteration's correspondence set: the loop cut after k updates leaves iteration k's set behind
    for k in range(1, g["iterations"]):
        gk = hip.gicp(vs, vt, ns, nt, G0, _gicp_params(max_iterations=k))
        ok = G.run(vs, ns, vt, nt, G0, max_iter=k, corr_iter=k - 1)
        assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_CORR, np.int32), ok["corr"]), k
        assert np.array_equal(gk["T"], o["trace"][k - 1, :16].reshape(4, 4)), k
    # a second run gives the same bits
    g2 = hip.gicp(vs, vt, ns, nt, G0, prm)
    assert np.array_equal(g2["T"], g["T"])
    assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18), trace)


def test_unusable_normals_are_skipped_like_the_restatement_skips_them(hip, vox_pair):
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    ns2, nt2 = ns.copy(), nt.copy()
    ns2[::7, :3] = 0.0
    ns2[3::11, 1] = np.inf
    nt2[::5, :3] = 0.0
    nt2[2::13, 0] = np.nan
    g = hip.gicp(vs, vt, ns2, nt2, G0, _gicp_params(max_iterations=6))
    o = G.run(vs, ns2, vt, nt2, G0, max_iter=6)
    _same_icp(g, o)
    # no usable source normal at all: too few correspondences, T = guess
    g = hip.gicp(vs, vt, np.zeros_like(ns), nt, G0, _gicp_params())
    assert g["stop_reason"] == 4 and not g["valid"] and g["n_corr"] == 0 and np.array_equal(g["T"], G0)


def test_refine_pair_uses_the_normals_the_registration_left_in_the_slot(hip):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, Tgt = _tilted(synth.kitti64_pair_16k(1))
    fp = ql.default_frontend_params(seed=1)
    r = hip.register_pair(s, t, fp)
    p = hip.refine_pair(None, _gicp_params())
    vs = hip.debug_fetch(ql.DBG_VOX_SRC, np.float32).reshape(-1, 4)
    vt = hip.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
    ns, _ = hip.fpfh(vs, fp.normal_radius, fp.fpfh_radius)
    nt, _ = hip.fpfh(vt, fp.normal_radius, fp.fpfh_radius)
    q = hip.gicp(vs, vt, ns, nt, r["T"], _gicp_params())
    assert p["valid"] and p["iterations"] >= 2
    _same_icp(p, q, "refine_pair vs qtr_gicp on the slot's clouds")


def test_normals_computed_on_the_device_match_explicit_ones(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    prm = _gicp_params(normal_radius=0.5)
    a = hip.gicp(vs, vt, ns, nt, G0, prm)
    for got, what in ((hip.icp(vs, vt, None, G0, prm), "qtr_icp, no normals"),
                      (hip.icp(vs, vt, nt, G0, prm), "qtr_icp, target normals"),
                      (hip.gicp(vs, vt, None, None, G0, prm), "qtr_gicp, no normals"),
                      (hip.gicp(vs, vt, ns, None, G0, prm), "qtr_gicp, source normals"),
                      (hip.gicp(vs, vt, None, nt, G0, prm), "qtr_gicp, target normals")):
        _same_icp(a, got, what)
    assert a["valid"] and a["iterations"] >= 3


CASES = [  # (batch slots, ICP parameters, environment of the batch handle)
    (16, {}, {}),                               # two lanes of 8, the defaults
    (4, {"max_iterations": 4}, {}),             # slots reused chunk after chunk; a short loop
    (4, {}, {"QTR_ICP_BLOCK": "5"}),            # blocks of 5 launches
]


@pytest.mark.parametrize("n_slots,icp_kw,env", CASES)
def test_batch_refine_is_bit_equal_to_the_single_pair_path(pairs, n_slots, icp_kw, env):
    from quatro_amd import lib as ql
    icp = _gicp_params(**icp_kw)
    h1 = _handle(1)
    hb = _handle(n_slots, **env)
    hp = _handle(n_slots)
    try:
        ref = []
        for s, t, seed in pairs:
            r = h1.register_pair(s, t, ql.default_frontend_params(seed=seed))
            ref.append((r, h1.refine_pair(None, icp)))
        plain = hp.register_batch(pairs)
        res, refined = hb.register_batch_refine(pairs, icp=icp)
    finally:
        h1.close()
        hb.close()
        hp.close()
    for i, ((r1, g1), p, r, g) in enumerate(zip(ref, plain, res, refined)):
        assert r["status"] == ql.QTR_OK and g["status"] == ql.QTR_OK and g["valid"], i
        _same_reg(r, p, f"result {i}")
        _same_reg(r, r1, f"result {i} vs register_pair")
        _same_icp(g, g1, f"refined {i}")
    print(f"{n_slots} slots {icp_kw}: iterations {sorted({g['iterations'] for g in refined})}, "
          f"stop reasons {sorted({g['stop_reason'] for g in refined})}")


def test_mixed_batch_leaves_a_correspondence_only_pair_unrefined():
    from quatro_amd import lib as ql
    from quatro_amd import synth
    a = _tilted(synth.kitti64_pair_16k(0))
    b = synth.kitti64_pair(1)
    cs, ct, _, _ = synth.correspondences(L=2000, inlier_frac=0.2, seed=3)
    mixed = [(a[0], a[1], 1), (None, None, 2, cs, ct), (b[0], b[1], 3)]
    hb = _handle(4)
    h1 = _handle(1)
    try:
        res, refined = hb.register_batch_refine(mixed, icp=_gicp_params())
        single = []
        for i in (0, 2):
            h1.register_pair(mixed[i][0], mixed[i][1], ql.default_frontend_params(seed=mixed[i][2]))
            single.append(h1.refine_pair(None, _gicp_params()))
    finally:
        hb.close()
        h1.close()
    assert [r["status"] for r in res] == [ql.QTR_OK] * 3
    assert [g["status"] for g in refined] == [ql.QTR_OK, ql.QTR_ERR_NOT_RUN, ql.QTR_OK]
    assert not refined[1]["valid"] and np.array_equal(refined[1]["T"], res[1]["T"])
    _same_icp(refined[0], single[0], "pair 0")
    _same_icp(refined[2], single[1], "pair 2")


def test_only_plane_to_plane_goes_through_qtr_gicp(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    for method in (ql.ICP_POINT_TO_PLANE, ql.ICP_POINT_TO_POINT, 7):
        with pytest.raises(ql.QuatroHipError) as ei:
            hip.gicp(vs, vt, ns, nt, Tgt, ql.default_icp_params(method=method))
        assert ei.value.code == ql.QTR_ERR_BAD_ARG, method
    # the arguments are checked as qtr_icp checks them; empty clouds: QTR_OK, valid = 0, T = guess
    res, prm = ql.IcpResult(), _gicp_params()
    lib = hip._lib
    assert lib.qtr_gicp(hip._h, 0, None, 5, None, vt.ctypes.data, vt.shape[0], None, None, prm, res, 0) == ql.QTR_ERR_BAD_ARG
    assert lib.qtr_gicp(hip._h, 9, vs.ctypes.data, 10, None, vt.ctypes.data, 10, None, None, prm, res, 0) == ql.QTR_ERR_BAD_ARG
    e = hip.gicp(vs[:0], vt, ns[:0], nt, Tgt)
    assert not e["valid"] and np.array_equal(e["T"], Tgt)
    small = ql.Handle(0, max_points=8192, max_voxels=4096, max_corr=1024)
    try:
        with pytest.raises(ql.QuatroHipError) as ei:
            small.gicp(vs[:5000], vt[:100], None, None, Tgt)
        assert ei.value.code == ql.QTR_ERR_CAPACITY
    finally:
        small.close()


def test_device_memory_gives_the_host_paths_bits(hip, vox_pair, pairs):
    import torch
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    prm = _gicp_params()
    d = [torch.from_numpy(x).cuda() for x in (vs, vt, ns, nt)]
    a = hip.gicp(vs, vt, ns, nt, G0, prm)
    _same_icp(a, hip.gicp(d[0], d[1], d[2], d[3], G0, prm), "qtr_gicp, both normal sets")
    _same_icp(a, hip.gicp(d[0], d[1], None, None, G0, prm), "qtr_gicp, no normals")
    _same_icp(a, hip.gicp(d[0], d[1], None, d[3], G0, prm), "qtr_gicp, target normals")
    _same_icp(a, hip.icp(d[0], d[1], None, G0, prm), "qtr_icp, no normals")
    _same_icp(a, hip.icp(d[0], d[1], d[3], G0, prm), "qtr_icp, target normals")
    sub = pairs[:4]
    hb = _handle(4)
    try:
        hres, href = hb.register_batch_refine(sub, icp=prm)
        items = [{"src": torch.from_numpy(np.ascontiguousarray(s)).cuda(), "tgt": torch.from_numpy(np.ascontiguousarray(t)).cuda(),
                  "fp": ql.default_frontend_params(seed=seed)} for s, t, seed in sub]
        torch.cuda.synchronize()
        dres, dref = hb.register_batch_dev_refine(items, ql.demo_params(), prm)
    finally:
        hb.close()
    for i in range(len(sub)):
        assert np.array_equal(dres[i]["T"].view(np.uint64), hres[i]["T"].view(np.uint64)), i
        _same_icp(dref[i], href[i], f"batched pair {i}")


def test_no_state_crosses_from_one_method_to_the_next(hip):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, _ = _tilted(synth.kitti64_pair(3))
    fp = ql.default_frontend_params(seed=3)
    hip.register_pair(s, t, fp)
    alone = [hip.refine_pair(None, ql.default_icp_params(method=m)) for m in (0, 1)]
    hip.register_pair(s, t, fp)
    g = hip.refine_pair(None, _gicp_params())
    after = [hip.refine_pair(None, ql.default_icp_params(method=m)) for m in (0, 1)]
    g2 = hip.refine_pair(None, _gicp_params())
    for m in (0, 1):
        _same_icp(alone[m], after[m], f"method {m} after plane-to-plane")
    _same_icp(g, g2, "plane-to-plane after the other two")


def test_python_class_reaches_plane_to_plane(hip, vox_pair):
    from quatro_amd import api
    vs, vt, ns, nt, Tgt = vox_pair
    icp = api.IterativeClosestPoint(handle=hip, method="plane_to_plane")
    icp.setInputSource(vs)
    icp.setInputTarget(vt)
    icp.setSourceNormals(ns)
    icp.setTargetNormals(nt)
    out = icp.align(_perturbed(Tgt))
    assert icp.hasConverged() and out.shape == vs.shape
    assert np.array_equal(icp.getFinalTransformation(), hip.gicp(vs, vt, ns, nt, _perturbed(Tgt))["T"])


@pytest.mark.parametrize("normals", ["computed", "given"])
def test_cpp_gicp_demo_gives_the_python_paths_bits(hip, vox_pair, tmp_path, normals):
    from quatro_amd import build as qbuild
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "gicp_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "gicp_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    for a, name in ((vs, "s.bin"), (vt, "t.bin"), (ns, "ns.bin"), (nt, "nt.bin")):
        a.tofile(str(tmp_path / name))
    (tmp_path / "g.txt").write_text(" ".join(repr(float(x)) for x in G0.reshape(-1)))
    args = [exe, str(tmp_path / "s.bin"), str(tmp_path / "t.bin"), str(tmp_path / "g.txt")]
    if normals == "given":
        args += [str(tmp_path / "ns.bin"), str(tmp_path / "nt.bin")]
    out = subprocess.run(args, capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    T = np.array([int(w, 16) for ln in out[1:5] for w in ln.split()], dtype=np.uint64).view(np.float64).reshape(4, 4)
    g = hip.gicp(vs, vt, ns, nt, G0) if normals == "given" else hip.gicp(vs, vt, None, None, G0)
    assert np.array_equal(T, g["T"]), (out, g["T"])


def test_plane_to_plane_lowers_the_rotation_error_of_tilted_registrations(hip):
    """Rotation / translation error against the generator's truth on the tilted kitti64_pair_16k(0..3): the registration,
    point-to-plane, plane-to-plane (the table of DESIGN.md section 9).  The plane-to-plane result is the host
    restatement's, bit for bit, so the assertion below is one about the arithmetic, not about the device."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    rows = []
    for k in range(4):
        s, t, Tgt = _tilted(synth.kitti64_pair_16k(k))
        fp = ql.default_frontend_params(seed=k)
        r = hip.register_pair(s, t, fp)
        p2pl = hip.refine_pair(None, ql.default_icp_params())
        g = hip.refine_pair(None, _gicp_params())
        vs = hip.debug_fetch(ql.DBG_VOX_SRC, np.float32).reshape(-1, 4)
        vt = hip.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
        ns, _ = hip.fpfh(vs, fp.normal_radius, fp.fpfh_radius)
        nt, _ = hip.fpfh(vt, fp.normal_radius, fp.fpfh_radius)
        o = G.run(vs, ns, vt, nt, r["T"])
        _same_icp({**g, "status": 0}, o, f"pair {k}: device vs restatement")
        e = [R.rot_err_deg(x["T"], Tgt) for x in (r, p2pl, g)]
        d = [float(np.linalg.norm(x["T"][:3, 3] - Tgt[:3, 3])) for x in (r, p2pl, g)]
        print(f"pair {k}: quatro {e[0]:.3f} deg {d[0]:.3f} m | point-to-plane {e[1]:.3f} deg {d[1]:.3f} m, "
              f"{p2pl['iterations']} it, stop {p2pl['stop_reason']} | plane-to-plane {e[2]:.3f} deg {d[2]:.3f} m, "
              f"{g['iterations']} it, stop {g['stop_reason']}, {g['n_corr']} corr")
        rows.append((g["valid"], e[0], e[2]))
    for k, (valid, e0, e2) in enumerate(rows):
        assert valid and e2 < e0, (k, e0, e2)
