"""No-GPU checks of the plane-to-plane (Generalized ICP) refinement, qtr_gicp / method QTR_ICP_PLANE_TO_PLANE: the binding
against the header, the host restatement of the device loop (tests/gicp_ref/gicp_ref.cpp over include/qtr_icp_math.h) on
exact data, the restatement against an independent scipy cKDTree GICP, the covariance-from-normal identity the design
rests on, and the skip rules."""
import os
import re

import numpy as np
import pytest

import gicp_restate as G
import icp_restate as R
from test_icp_cpu import _exact_pair

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 1e-3  # QTR_ICP_GICP_EPSILON


def test_gicp_method_and_entry_point_are_bound():
    from quatro_amd import lib as ql
    assert ql.ICP_PLANE_TO_PLANE == 2
    lib = ql.load()
    assert "qtr_gicp" in ql.EXPORTS and lib.qtr_gicp.argtypes is not None and len(lib.qtr_gicp.argtypes) == 12
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    assert re.search(r"#define QTR_ICP_PLANE_TO_PLANE 2\b", hdr)
    decl = re.search(r"QTR_API int qtr_gicp\((.*?)\);", hdr, flags=re.S).group(1)
    assert [a.split()[-1].split("[")[0].lstrip("*") for a in decl.split(",")] == [
        "h", "slot", "src4", "n_s", "src_normals4", "tgt4", "n_t", "tgt_normals4", "guess", "prm", "res", "mem"]
    math = open(os.path.join(ROOT, "include", "qtr_icp_math.h")).read()
    assert re.search(r"#define QTR_ICP_GICP_EPSILON 1e-3\b", math)
    assert hasattr(ql.Handle, "gicp")


def test_restatement_recovers_an_exact_rigid_copy():
    # d = 0 at the truth is a fixed point of Gauss-Newton whatever M is: the bound of the other two methods
    s, tgt, nt, T = _exact_pair()
    _, ns = R.box_scene()
    guess = T @ R.rigid(R.rot(0.02, -0.015, 0.03), [0.3, -0.2, 0.1])
    o = G.run(s, ns, tgt, nt, guess, max_d=1.5, max_iter=60, teps=1e-12, feps=0.0)
    assert o["valid"] and o["converged"]
    assert np.abs(o["T"] - T).max() <= 1e-9
    assert o["fitness"] < 1e-20 and o["n_corr"] == s.shape[0]
    assert o["trace"].shape == (o["iterations"], 18) and np.array_equal(o["trace"][-1, :16].reshape(4, 4), o["T"])
    # started at the truth it stays there: every d is exactly zero, so the update is the identity and the loop stops on it
    o = G.run(s, ns, tgt, nt, T, max_d=1.5, max_iter=5, teps=0.0, feps=0.0)
    assert np.array_equal(o["T"], T) and o["iterations"] == 1 and o["stop_reason"] == 2


def _cov(n):
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    return np.eye(3) - (1 - EPS) * n[..., :, None] * n[..., None, :]


def _skew(q):
    K = np.zeros(q.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -q[..., 2], q[..., 1]
    K[..., 1, 0], K[..., 1, 2] = q[..., 2], -q[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -q[..., 1], q[..., 0]
    return K


def _scipy_gicp(src, src_nrm, tgt, tgt_nrm, T, max_d, iters):
    """Independent float64 GICP: cKDTree nearest neighbours, explicit covariances, np.linalg.inv / solve, the same
    left-multiplied increment.  Returns every iteration's T and the smallest gap between the two nearest distances."""
    from scipy.spatial import cKDTree
    tree = cKDTree(tgt[:, :3].astype(np.float64))
    p = src[:, :3].astype(np.float64)
    Ca, Cb = _cov(src_nrm[:, :3].astype(np.float64)), _cov(tgt_nrm[:, :3].astype(np.float64))
    out, ties = [], 0
    for _ in range(iters):
        Rm = T[:3, :3]
        q = p @ Rm.T + T[:3, 3]
        d2, j2 = tree.query(q, k=2)
        ties += int((d2[:, 0] == d2[:, 1]).sum())
        ok = d2[:, 0] <= max_d
        j = j2[ok, 0]
        q, d = q[ok], q[ok] - tgt[j, :3].astype(np.float64)
        M = np.linalg.inv(Cb[j] + Rm @ Ca[ok] @ Rm.T)
        J = np.concatenate([-_skew(q), np.broadcast_to(np.eye(3), q.shape[:1] + (3, 3))], axis=2)
        H = np.einsum("nai,nab,nbj->ij", J, M, J)
        b = -np.einsum("nai,nab,nb->i", J, M, d)
        x = np.linalg.solve(H, b)
        qq = np.r_[1.0, x[:3] / 2]
        a, bq, c, e = qq / np.linalg.norm(qq)
        dR = np.array([[a * a + bq * bq - c * c - e * e, 2 * (bq * c - a * e), 2 * (bq * e + a * c)],
                       [2 * (bq * c + a * e), a * a - bq * bq + c * c - e * e, 2 * (c * e - a * bq)],
                       [2 * (bq * e - a * c), 2 * (c * e + a * bq), a * a - bq * bq - c * c + e * e]])
        T = R.rigid(dR, x[3:]) @ T
        out.append(T)
    return out, ties


def test_restatement_agrees_with_an_independent_scipy_gicp():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(7)
    s, n = R.box_scene(seed=5)
    Tt = R.rigid(R.rot(0.03, -0.02, 0.05), [0.4, -0.3, 0.2])
    tgt = R.apply(Tt, s)
    tgt[:, :3] += rng.normal(0, 0.01, (tgt.shape[0], 3)).astype(np.float32)  # sensor noise: no exact fixed point
    nt = n.copy()
    nt[:, :3] = n[:, :3] @ Tt[:3, :3].T
    o = G.run(s, n, tgt, nt, np.eye(4), max_d=1.0, max_iter=12, teps=0.0, feps=0.0)
    assert o["iterations"] == 12 and o["stop_reason"] == 1
    Ts, ties = _scipy_gicp(s, n, tgt, nt, np.eye(4), 1.0, 12)
    assert ties == 0  # (an exact distance tie could send the two searches to different neighbours: none on this scene)
    for k in range(12):
        assert np.abs(o["trace"][k, :16].reshape(4, 4) - Ts[k]).max() < 1e-9, k
    assert np.abs(o["T"] - Ts[-1]).max() < 1e-9
    assert R.rot_err_deg(o["T"], Tt) < 0.05 and np.abs(o["T"][:3, 3] - Tt[:3, 3]).max() < 0.02


def test_plane_regularised_covariance_is_a_function_of_the_normal():
    rng = np.random.default_rng(11)
    for _ in range(50):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        # a planar neighbourhood with normal n (a little noise off the plane: n stays the smallest eigenvector's span)
        u = np.cross(n, rng.normal(size=3))
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        ab = rng.normal(size=(40, 2))
        pts = ab[:, :1] * u + ab[:, 1:] * v
        w, U = np.linalg.eigh(np.cov(pts.T))
        assert abs(abs(U[:, 0] @ n) - 1) < 1e-12  # eigh: ascending eigenvalues, the normal first
        C = U @ np.diag([EPS, 1.0, 1.0]) @ U.T
        assert np.abs(C - (np.eye(3) - (1 - EPS) * np.outer(n, n))).max() < 1e-12


def test_normals_that_cannot_be_used_are_skipped():
    s, tgt, nt, T = _exact_pair()
    _, ns = R.box_scene()
    guess = T @ R.rigid(R.rot(0.01, -0.01, 0.01), [0.1, -0.1, 0.05])
    kw = dict(max_d=1.5, max_iter=1, teps=0.0, feps=0.0)
    base = G.run(s, ns, tgt, nt, guess, **kw)
    assert base["n_corr"] == s.shape[0] and (base["corr"] >= 0).all()
    # source side: skipped before the search
    ns2 = ns.copy()
    ns2[3, 0] = np.nan
    ns2[10, :3] = 0.0
    ns2[20, 2] = np.inf
    o = G.run(s, ns2, tgt, nt, guess, **kw)
    assert o["n_corr"] == base["n_corr"] - 3 and list(np.flatnonzero(o["corr"] < 0)) == [3, 10, 20]
    # target side: the correspondence is dropped, nothing else takes its place
    nt2 = nt.copy()
    hit = [int(base["corr"][5]), int(base["corr"][50])]
    nt2[hit[0], 1] = np.nan
    nt2[hit[1], :3] = 0.0
    o = G.run(s, ns, tgt, nt2, guess, **kw)
    lost = np.flatnonzero(np.isin(base["corr"], hit))
    assert len(lost) >= 2 and o["n_corr"] == base["n_corr"] - len(lost)
    assert np.array_equal(np.flatnonzero(o["corr"] < 0), lost)
    keep = o["corr"] >= 0
    assert np.array_equal(o["corr"][keep], base["corr"][keep])
    # a normal's length does not matter
    o = G.run(s, ns * np.float32(4.0), tgt, nt * np.float32(0.25), guess, **kw)
    assert np.array_equal(o["T"], base["T"])  # (powers of two: the normalised normals are the same doubles)


def test_fewer_than_four_correspondences_stop_the_loop():
    s, tgt, nt, T = _exact_pair()
    _, ns = R.box_scene()
    guess = T @ R.rigid(R.rot(0.01, -0.01, 0.01), [0.1, -0.1, 0.05])
    ns3 = np.zeros_like(ns)
    ns3[:3] = ns[:3]  # three usable source normals
    o = G.run(s, ns3, tgt, nt, guess, max_d=1.5)
    assert o["stop_reason"] == 4 and not o["valid"] and o["iterations"] == 0 and o["n_corr"] == 3
    assert np.array_equal(o["T"], guess)
    far = R.rigid(np.eye(3), [5000.0, 0, 0])
    o = G.run(s, ns, tgt, nt, far)
    assert o["stop_reason"] == 4 and not o["valid"] and o["n_corr"] == 0 and np.array_equal(o["T"], far)
