"""No-GPU checks of the voxelised plane-to-plane refinement (VGICP), method QTR_ICP_VOXEL_PLANE_TO_PLANE: the binding
against the header, the host restatement of the device loop (tests/vgicp_ref/vgicp_ref.cpp over include/qtr_icp_math.h)
on an exact rigid copy, against an independent numpy implementation, and the contract's rules one by one: the grid, the
members, the summation order, the stops and the cell cap."""
import os
import re

import numpy as np

import icp_restate as R
import vgicp_restate as V
from test_icp_cpu import _exact_pair

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 1e-3  # QTR_ICP_GICP_EPSILON

# The exact rigid copy of test_restatement_recovers_an_exact_rigid_copy.  Unlike the search methods' the truth is not an
# exact fixed point of this one: a source point is compared with its voxel's mean, and in a voxel that holds parts of two
# faces sum d x M d does not vanish.  max |T - truth| over the 3 x 4 block, measured on the CPU and printed by the test:
# 1.2e-3 (rotation entries and metres alike; 14 updates from 0.3) at 1.5 m voxels.  Asserted: ten times that.
EXACT_COPY_MEASURED = 1.2e-3
# Largest |T_restatement - T_numpy| over the 12 iterations of the independent check, measured on the CPU and printed by the
# test: 7.5e-15 (np.linalg.inv and solve against the adjugate and LDL^T, means of covariances against covariances of
# means of n n^T).  Asserted: ten times that.
NUMPY_AGREEMENT_MEASURED = 7.5e-15


def test_voxel_method_is_bound_without_a_new_entry_point():
    from quatro_amd import api
    from quatro_amd import lib as ql
    assert ql.ICP_VOXEL_PLANE_TO_PLANE == 3
    assert len(ql.EXPORTS) == 75
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    assert re.search(r"#define QTR_ICP_VOXEL_PLANE_TO_PLANE 3\b", hdr)
    math = open(os.path.join(ROOT, "include", "qtr_icp_math.h")).read()
    assert re.search(r"#define QTR_ICP_CELL_CAP \(1 << 22\)", math) and re.search(r"#define QTR_ICP_T_W 30\b", math)
    icp = api.IterativeClosestPoint(handle=object(), method="voxel_plane_to_plane")
    assert icp.params_.method == ql.ICP_VOXEL_PLANE_TO_PLANE
    try:
        api.IterativeClosestPoint(handle=object(), method="voxel")
        raise AssertionError("an unknown method was accepted")
    except ValueError as e:
        assert all(m in str(e) for m in ("point_to_plane", "point_to_point", "'plane_to_plane'", "voxel_plane_to_plane"))
    hpp = open(os.path.join(ROOT, "include", "quatro_icp.hpp")).read()
    assert "VOXEL_PLANE_TO_PLANE = QTR_ICP_VOXEL_PLANE_TO_PLANE" in hpp


def test_restatement_recovers_an_exact_rigid_copy():
    s, tgt, nt, T = _exact_pair()
    _, ns = R.box_scene()
    guess = T @ R.rigid(R.rot(0.02, -0.015, 0.03), [0.3, -0.2, 0.1])
    o = V.run(s, ns, tgt, nt, guess, max_d=1.5, max_iter=60, teps=1e-12, feps=0.0)
    err = np.abs(o["T"] - T)[:3].max()
    print(f"exact copy: {o['iterations']} iterations, stop {o['stop_reason']}, {o['n_corr']} of {s.shape[0]} correspondences, "
          f"max |T - truth| {err:.3e} (guess: {np.abs(guess - T)[:3].max():.3e})")
    assert o["valid"] and o["status"] == 0
    assert err <= 10 * EXACT_COPY_MEASURED
    assert o["trace"].shape == (o["iterations"], 18) and np.array_equal(o["trace"][-1, :16].reshape(4, 4), o["T"])
    # rmse is the weighted one, fitness the plain mean of d^2 over the correspondences
    assert o["fitness"] > 0 and o["rmse"] > 0 and o["n_corr"] > s.shape[0] // 2


def _skew(q):
    K = np.zeros(q.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -q[..., 2], q[..., 1]
    K[..., 1, 0], K[..., 1, 2] = q[..., 2], -q[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -q[..., 1], q[..., 0]
    return K


def _cov(n):
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    return np.eye(3) - (1 - EPS) * n[..., :, None] * n[..., None, :]


def _numpy_voxels(tgt, tgt_nrm, side):
    """One Gaussian per voxel with explicit per-point covariances and np.add.at: origin, dims, and per linear cell index
    the count, the mean and the mean covariance."""
    t = tgt[:, :3].astype(np.float64)
    o = t.min(0)
    dims = np.floor((t.max(0) - o) / side).astype(np.int64) + 1
    idx = np.floor((t - o) / side).astype(np.int64)
    lin = idx[:, 0] + dims[0] * (idx[:, 1] + dims[1] * idx[:, 2])
    ncell = int(dims.prod())
    N = np.zeros(ncell)
    mu = np.zeros((ncell, 3))
    C = np.zeros((ncell, 3, 3))
    np.add.at(N, lin, 1.0)
    np.add.at(mu, lin, t)
    np.add.at(C, lin, _cov(tgt_nrm[:, :3].astype(np.float64)))
    has = N > 0
    mu[has] /= N[has, None]
    C[has] /= N[has, None, None]
    return o, dims, N, mu, C


def _numpy_vgicp(src, src_nrm, tgt, tgt_nrm, T, side, iters):
    """Independent float64 VGICP.  Returns every iteration's T, the correspondence counts and the smallest distance of a
    coordinate (target or transformed source) to a voxel face, in voxel sides."""
    o, dims, N, mu, C = _numpy_voxels(tgt, tgt_nrm, side)
    p = src[:, :3].astype(np.float64)
    Ca = _cov(src_nrm[:, :3].astype(np.float64))
    frac = (tgt[:, :3].astype(np.float64) - o) / side
    face = [np.abs(frac - np.round(frac))[frac > 0.5].min()]  # (the origin's own coordinates lie on a face by construction)
    out, counts = [], []
    for _ in range(iters):
        Rm = T[:3, :3]
        q = p @ Rm.T + T[:3, 3]
        f = (q - o) / side
        face.append(np.abs(f - np.round(f)).min())
        idx = np.floor(f).astype(np.int64)
        inside = ((idx >= 0) & (idx < dims)).all(1)
        lin = np.where(inside, idx[:, 0] + dims[0] * (idx[:, 1] + dims[1] * idx[:, 2]), 0)
        ok = inside & (N[lin] > 0)
        lin, q = lin[ok], q[ok]
        d = q - mu[lin]
        M = np.linalg.inv(C[lin] + Rm @ Ca[ok] @ Rm.T)
        J = np.concatenate([-_skew(q), np.broadcast_to(np.eye(3), q.shape[:1] + (3, 3))], axis=2)
        H = np.einsum("n,nai,nab,nbj->ij", N[lin], J, M, J)
        b = -np.einsum("n,nai,nab,nb->i", N[lin], J, M, d)
        x = np.linalg.solve(H, b)
        qq = np.r_[1.0, x[:3] / 2]
        a, bq, c, e = qq / np.linalg.norm(qq)
        dR = np.array([[a * a + bq * bq - c * c - e * e, 2 * (bq * c - a * e), 2 * (bq * e + a * c)],
                       [2 * (bq * c + a * e), a * a - bq * bq + c * c - e * e, 2 * (c * e - a * bq)],
                       [2 * (bq * e - a * c), 2 * (c * e + a * bq), a * a - bq * bq - c * c + e * e]])
        T = R.rigid(dR, x[3:]) @ T
        out.append(T)
        counts.append(int(ok.sum()))
    return out, counts, min(face)


def _noisy_scene():
    rng = np.random.default_rng(7)
    s, n = R.box_scene(seed=5)
    Tt = R.rigid(R.rot(0.03, -0.02, 0.05), [0.4, -0.3, 0.2])
    tgt = R.apply(Tt, s)
    tgt[:, :3] += rng.normal(0, 0.01, (tgt.shape[0], 3)).astype(np.float32)  # sensor noise
    nt = n.copy()
    nt[:, :3] = n[:, :3] @ Tt[:3, :3].T
    return s, n, tgt, nt, Tt


def test_restatement_agrees_with_an_independent_numpy_vgicp():
    s, n, tgt, nt, Tt = _noisy_scene()
    o = V.run(s, n, tgt, nt, np.eye(4), max_d=1.0, max_iter=12, teps=0.0, feps=0.0)
    assert o["iterations"] == 12 and o["stop_reason"] == 1
    Ts, counts, face = _numpy_vgicp(s, n, tgt, nt, np.eye(4), 1.0, 12)
    # no coordinate within 1e-9 voxel sides of a face: the two floor()s cannot disagree
    assert face > 1e-9, face
    assert [int(c) for c in o["trace"][:, 17]] == counts
    err = max(np.abs(o["trace"][k, :16].reshape(4, 4) - Ts[k]).max() for k in range(12))
    print(f"restatement vs numpy over 12 iterations: max |dT| {err:.3e}; smallest distance to a voxel face {face:.3e} sides; "
          f"rot err {R.rot_err_deg(o['T'], Tt):.4f} deg, |dt| {np.abs(o['T'][:3, 3] - Tt[:3, 3]).max():.4f} m")
    assert err <= 10 * NUMPY_AGREEMENT_MEASURED
    # the records themselves: count, mean, covariance of every voxel
    org, dims, N, mu, C = _numpy_voxels(tgt, nt, 1.0)
    assert np.array_equal(o["grid"][:3], org) and np.array_equal(o["grid"][3:6], dims) and o["grid"][6] == dims.prod()
    rec = o["records"][o["records"][:, 0] > 0]
    lin = rec[:, 10].astype(np.int64)
    assert len(lin) == int((N > 0).sum()) and np.array_equal(rec[:, 0], N[lin])
    assert np.abs(rec[:, 1:4] - mu[lin]).max() < 1e-12
    Cr = C[lin]
    assert np.abs(rec[:, 4:10] - np.stack([Cr[:, 0, 0], Cr[:, 0, 1], Cr[:, 0, 2], Cr[:, 1, 1], Cr[:, 1, 2], Cr[:, 2, 2]], 1)).max() < 1e-12


def _cube_targets(side=1.0):
    """Eight voxels of 2 x 2 x 2 with five points each, strictly inside, on a grid whose origin is (0, 0, 0) and whose
    maximum corner is a target at (1.5, 1.5, 1.5); normals along z."""
    rng = np.random.default_rng(2)
    pts = []
    for cz in range(2):
        for cy in range(2):
            for cx in range(2):
                pts.append(np.array([cx, cy, cz]) * side + 0.125 + 0.25 * rng.random((5, 3)))
    pts = np.concatenate(pts)
    pts[0] = 0.0               # the origin (voxel 0)
    pts[-1] = 1.5 * side       # the box's maximum (voxel 7): dims = floor(1.5) + 1 = 2
    t = R.f4(pts)
    n = R.f4(np.tile([0.0, 0.0, 1.0], (len(pts), 1)))
    return t, n


def test_grid_rule_faces_belong_to_the_upper_voxel_and_outside_is_no_correspondence():
    t, n = _cube_targets()
    up, dn = np.nextafter(np.float32(2.0), np.float32(3.0)), np.nextafter(np.float32(0.0), np.float32(-1.0))
    below1, below2 = np.nextafter(np.float32(1.0), np.float32(0.0)), np.nextafter(np.float32(2.0), np.float32(0.0))
    src = R.f4(np.array([
        [1.0, 0.5, 0.5],       # 0: on the face between voxel 0 and voxel 1 -> the upper one (cell 1)
        [below1, 0.5, 0.5],    # 1: one ulp below that face -> cell 0
        [0.5, 1.0, 1.0],       # 2: on two faces -> cell (0, 1, 1) = 6
        [0.0, 0.0, 0.0],       # 3: the origin itself -> cell 0
        [dn, 0.5, 0.5], [0.5, dn, 0.5], [0.5, 0.5, dn],    # 4-6: one ulp outside the three lower faces
        [2.0, 0.5, 0.5], [0.5, 2.0, 0.5], [0.5, 0.5, 2.0],  # 7-9: ON the three upper faces of the grid: already outside
        [np.nan, 0.5, 0.5],    # 10: NaN
        [1e30, 0.5, 0.5],      # 11: huge
        [0.5, -1e30, 0.5],     # 12
        [below2, 0.5, 0.5],    # 13: one ulp inside the grid's upper face -> cell 1
    ], dtype=np.float64))
    # (2.0 is the first value outside: "one ulp outside the upper face" of [0, 2) in exact terms; the next float up too)
    src = np.concatenate([src, R.f4(np.array([[up, 0.5, 0.5], [0.5, up, 0.5], [0.5, 0.5, up]], dtype=np.float64))])
    ns = R.f4(np.tile([0.0, 0.0, 1.0], (len(src), 1)))
    o = V.run(src, ns, t, n, np.eye(4), max_d=1.0, max_iter=1, teps=0.0, feps=0.0)
    assert np.array_equal(o["grid"], [0, 0, 0, 2, 2, 2, 8])
    rep = {int(r[10]): j for j, r in enumerate(o["records"]) if r[0] > 0}  # cell -> representative
    assert sorted(rep) == list(range(8)) and all(rep[c] == 5 * c for c in range(8))
    want = [rep[1], rep[0], rep[6], rep[0]] + [-1] * 9 + [rep[1]] + [-1] * 3
    assert o["corr"].tolist() == want
    assert o["n_corr"] == 5
    # the same through a transform: the cell is the cell of q = T p, not of p
    o2 = V.run(src, ns, t, n, R.rigid(np.eye(3), [0.5, 0, 0]), max_d=1.0, max_iter=1, teps=0.0, feps=0.0)
    assert o2["corr"][:4].tolist() == [rep[1], rep[1], rep[7], rep[0]]
    assert o2["corr"][7] == -1 and o2["corr"][4] == rep[0]  # (dn + 0.5 is inside again)


def test_members_are_the_targets_with_a_usable_normal():
    t, n = _cube_targets()
    src = R.f4(np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.4, 1.4, 1.4]]))
    ns = R.f4(np.tile([0.0, 0.0, 1.0], (4, 1)))
    kw = dict(max_d=1.0, max_iter=1, teps=0.0, feps=0.0, min_corr=1)
    base = V.run(src, ns, t, n, np.eye(4), **kw)
    assert base["corr"].tolist() == [0, 5, 10, 35] and base["records"][0, 0] == 5
    n2 = n.copy()
    n2[0, :3] = 0.0        # voxel 0's lowest index: the representative moves on, the count drops
    n2[2, 0] = np.nan
    n2[5:10, :3] = 0.0     # voxel 1: nobody left -> the voxel does not exist
    n2[12, 2] = np.inf
    o = V.run(src, ns, t, n2, np.eye(4), **kw)
    assert o["corr"].tolist() == [1, -1, 10, 35]
    assert o["records"][1, 0] == 3 and o["records"][0, 0] == 0 and o["records"][10, 0] == 4
    assert not (o["records"][5:10, 0] > 0).any()
    # the mean is the members', not the cell's: voxel 0 without points 0 and 2
    assert np.allclose(o["records"][1, 1:4], t[[1, 3, 4], :3].astype(np.float64).mean(0), atol=1e-15)
    # a non-finite target point takes no part (and not in the box either)
    t3 = t.copy()
    t3[20] = [np.nan, 7.0, 7.0, 0.0]
    t3[21] = [np.inf, 0.5, 0.5, 0.0]
    o = V.run(src, ns, t3, n, np.eye(4), **kw)
    assert np.array_equal(o["grid"], [0, 0, 0, 2, 2, 2, 8]) and o["records"][22, 0] == 3
    # a normal's length does not matter (powers of two: the normalised normals are the same doubles)
    o = V.run(src, ns * np.float32(4.0), t, n * np.float32(0.25), np.eye(4), **kw)
    assert np.array_equal(o["T"], base["T"])


def test_sums_run_in_ascending_target_index_whatever_order_the_members_arrive_in():
    s, n, tgt, nt, _ = _noisy_scene()
    kw = dict(max_d=1.0, max_iter=3, teps=0.0, feps=0.0)
    base = V.run(s, n, tgt, nt, np.eye(4), **kw)
    rng = np.random.default_rng(0)
    for _ in range(3):  # the same cloud, indices preserved, handed over in another order: equal bits
        o = V.run(s, n, tgt, nt, np.eye(4), feed=rng.permutation(tgt.shape[0]), **kw)
        assert np.array_equal(o["records"].view(np.uint64), base["records"].view(np.uint64))
        assert np.array_equal(o["trace"].view(np.uint64), base["trace"].view(np.uint64))
        assert np.array_equal(o["corr"], base["corr"])
    # the storage order permuted inside voxels: the sums run in another order, so bits may move - but only as far as the
    # ascending-index rule says: re-summing the permuted members by hand in ascending NEW index gives the new record
    lin = base["records"][:, 10]
    big = int(lin[np.argmax(base["records"][:, 0])])
    rep = int(np.flatnonzero((base["records"][:, 0] > 0) & (lin == big))[0])
    org = base["grid"][:3]
    cell = np.floor((tgt[:, :3].astype(np.float64) - org) / 1.0)
    members = np.flatnonzero((cell == cell[rep]).all(1))
    assert len(members) == base["records"][rep, 0] >= 8 and members[0] == rep
    perm = np.arange(tgt.shape[0])
    perm[members] = members[::-1]            # reverse the voxel's members in storage
    t2, n2 = tgt[perm], nt[perm]
    o = V.run(s, n, t2, n2, np.eye(4), **kw)
    assert o["records"][rep, 0] == len(members)  # (the lowest index of the voxel is still `rep`: same places, other points)
    acc = np.zeros(3)
    for j in members:                         # ascending new index
        acc = acc + t2[j, :3].astype(np.float64)
    assert np.array_equal(o["records"][rep, 1:4], acc / len(members))
    acc_old = np.zeros(3)
    for j in members:
        acc_old = acc_old + tgt[j, :3].astype(np.float64)
    assert np.array_equal(base["records"][rep, 1:4], acc_old / len(members))
    # every other voxel is untouched
    others = np.setdiff1d(np.flatnonzero(base["records"][:, 0] > 0), [rep])
    assert np.array_equal(o["records"][others].view(np.uint64), base["records"][others].view(np.uint64))
    assert np.abs(o["T"] - base["T"]).max() < 1e-12


def test_fewer_than_four_correspondences_stop_the_loop():
    s, tgt, nt, T = _exact_pair()
    _, ns = R.box_scene()
    guess = T @ R.rigid(R.rot(0.01, -0.01, 0.01), [0.1, -0.1, 0.05])
    full = V.run(s, ns, tgt, nt, guess, max_d=1.5, max_iter=1)
    usable = np.flatnonzero(full["corr"] >= 0)[:3]
    ns3 = np.zeros_like(ns)
    ns3[usable] = ns[usable]  # three usable source normals, all three inside voxels
    o = V.run(s, ns3, tgt, nt, guess, max_d=1.5)
    assert o["stop_reason"] == 4 and not o["valid"] and o["iterations"] == 0 and o["n_corr"] == 3
    assert np.array_equal(o["T"], guess)
    ns4 = ns3.copy()
    nxt = np.flatnonzero(full["corr"] >= 0)[3]
    ns4[nxt] = ns[nxt]        # min_correspondences = 0 means 4
    o = V.run(s, ns4, tgt, nt, guess, max_d=1.5, max_iter=1)
    assert o["n_corr"] == 4 and o["stop_reason"] != 4
    far = R.rigid(np.eye(3), [5000.0, 0, 0])
    o = V.run(s, ns, tgt, nt, far)
    assert o["stop_reason"] == 4 and not o["valid"] and o["n_corr"] == 0 and np.array_equal(o["T"], far)
    # empty clouds, or a target without a finite point: valid = 0, T = guess
    for a, b in ((s[:0], tgt), (s, tgt[:0]), (s, np.full_like(tgt, np.nan))):
        na, nb = ns[:a.shape[0]], nt[:b.shape[0]]
        o = V.run(a, na, b, nb, guess)
        assert o["status"] == 0 and not o["valid"] and o["iterations"] == 0 and np.array_equal(o["T"], guess)


def test_a_grid_past_the_cell_cap_is_refused_not_coarsened():
    """0.01 m voxels on a 10 m box are 1001^3 cells against the cap of 2^22.  The box is the device's to find, so the C ABI
    cannot refuse before it has one: the same refusal through qtr_gicp is tests/test_gpu_vgicp.py's."""
    rng = np.random.default_rng(1)
    t = R.f4(rng.random((500, 3)) * 10.0)
    t[0, :3], t[1, :3] = 0.0, 10.0
    n = R.f4(np.tile([0.0, 0.0, 1.0], (500, 1)))
    o = V.run(t, n, t, n, np.eye(4), max_d=0.01)
    assert o["status"] == V.CAPACITY and not o["valid"] and np.array_equal(o["T"], np.eye(4))
    assert o["grid"][6] == 1001.0 ** 3 > 2 ** 22
    # the largest grid that fits is not refused, and one cell more is
    for side, ok in ((10.0 / 160.5, True), (10.0 / 161.5, False)):  # 161^3 = 4173281 <= 2^22 = 4194304 < 162^3
        o = V.run(t, n, t, n, np.eye(4), max_d=side, max_iter=1)
        assert (o["status"] == 0) == ok and o["grid"][6] == (161.0 if ok else 162.0) ** 3, (side, o["grid"])
