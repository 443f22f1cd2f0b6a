"""numpy float64 restatement of the registration evaluation (include/qtr_eval_math.h; quatro_amd/csrc/eval.hip).

Nothing of the header or the kernel is used: the correspondences come from the exhaustive search of tests/icp_brute.py (no
cell grid, no kd-tree), the terms are formed per point in the header's written order with numpy's binary64 + - * / sqrt
(numpy never fuses a product into a sum), and the sums take the header's shape: the 64-point fold of a wave, (w0 + w1) +
(w2 + w3) per 256-point chunk, the chunks in ascending order.  So the comparison with the header compiled by g++ and with
the device is equality of bits, not a tolerance.
"""
import numpy as np

import icp_brute as B

NT = 35
T_JTJ, T_R2, T_NPLANE, T_ST, T_STT, T_D2, T_CNT, T_NSRC = 0, 21, 22, 23, 26, 32, 33, 34
FIELDS_INT = ("valid", "n_source", "n_corr", "n_plane")
FIELDS_F64 = ("overlap", "sum_d2", "inlier_rmse", "plane_rmse", "information", "hessian_plane")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1).view(np.uint64)


def nearest_any(src4, tgt4, T):
    """The exhaustive search without a reach (icp_brute.search at an infinite distance): what evaluate() takes as `nearest`
    when one pair is evaluated at several distances — the nearest target is in reach exactly when any target is."""
    return B.search(src4, tgt4, T, np.inf)


def terms(src4, tgt4, T, max_d, tgt_nrm4=None, nearest=None):
    """(float64 [ns, NT] per-point terms, int32 [ns] correspondences)."""
    src4, tgt4 = B.f4(src4), B.f4(tgt4)
    ns = src4.shape[0]
    e = np.zeros((ns, NT))
    if nearest is not None:
        ok = nearest[1] <= float(max_d) * float(max_d)
        corr, d2 = np.where(ok, nearest[0], -1).astype(np.int32), np.where(ok, nearest[1], np.inf)
    else:
        corr, d2 = (B.search(src4, tgt4, T, max_d) if ns and tgt4.shape[0] else
                    (np.full(ns, -1, np.int32), np.full(ns, np.inf)))
    e[B.finite3(src4), T_NSRC] = 1.0
    has = np.flatnonzero(corr >= 0)
    if has.size == 0:
        return e, corr
    q = B.transform(src4[has], T)
    t = tgt4[corr[has], :3].astype(np.float64)
    e[has, T_ST:T_ST + 3] = t
    k = T_STT
    for a in range(3):
        for b in range(a, 3):
            e[has, k] = t[:, a] * t[:, b]
            k += 1
    e[has, T_D2] = d2[has]
    e[has, T_CNT] = 1.0
    if tgt_nrm4 is not None:
        tn = B.f4(tgt_nrm4)
        ok = B.finite3(tn)[corr[has]]
        rows = has[ok]
        q, t = q[ok], t[ok]
        n = tn[corr[rows], :3].astype(np.float64)
        r = ((q[:, 0] - t[:, 0]) * n[:, 0] + (q[:, 1] - t[:, 1]) * n[:, 1]) + (q[:, 2] - t[:, 2]) * n[:, 2]
        J = [q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2],
             q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
        k = T_JTJ
        for a in range(6):
            for b in range(a, 6):
                e[rows, k] = J[a] * J[b]
                k += 1
        e[rows, T_R2] = r * r
        e[rows, T_NPLANE] = 1.0
    return e, corr


def fold_sum(e):
    """The header's sum shape over the rows of e (source order)."""
    n, nt = e.shape
    if n == 0:
        return np.zeros(nt)
    nchunk = (n + 255) // 256
    a = np.zeros((nchunk * 256, nt))
    a[:n] = e
    a = a.reshape(nchunk, 4, 64, nt)
    off = 32
    while off >= 1:  # qtr_icp_fold64: p[l] = p[l] + p[l + off] for l < off
        a[:, :, :off] = a[:, :, :off] + a[:, :, off:2 * off]
        off >>= 1
    w = a[:, :, 0]
    c = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])  # qtr_icp_chunk_sum
    acc = c[0].copy()
    for k in range(1, nchunk):
        acc = acc + c[k]
    return acc


def finish(S):
    """qtr_eval_finish."""
    n, ns, npl = S[T_CNT], S[T_NSRC], S[T_NPLANE]
    out = {"valid": int(n > 0), "n_source": int(ns), "n_corr": int(n), "n_plane": int(npl),
           "overlap": n / ns if ns > 0 else 0.0, "sum_d2": float(S[T_D2]),
           "inlier_rmse": float(np.sqrt(S[T_D2] / n)) if n > 0 else 0.0,
           "plane_rmse": float(np.sqrt(S[T_R2] / npl)) if npl > 0 else 0.0}
    X = S[T_STT:T_STT + 6]
    sx, sy, sz = S[T_ST:T_ST + 3]
    I = np.zeros((6, 6))
    I[0, 0], I[1, 1], I[2, 2] = X[3] + X[5], X[0] + X[5], X[0] + X[3]
    I[0, 1], I[0, 2], I[1, 2] = -X[1], -X[2], -X[4]
    I[0, 4], I[0, 5] = -sz, sy
    I[1, 3], I[1, 5] = sz, -sx
    I[2, 3], I[2, 4] = -sy, sx
    I[3, 3] = I[4, 4] = I[5, 5] = n
    H = np.zeros((6, 6))
    k = T_JTJ
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = S[k]
            k += 1
    for a in range(6):
        for b in range(a):
            I[a, b], H[a, b] = I[b, a], H[b, a]
    out["information"], out["hessian_plane"] = I, H
    return out


def evaluate(src4, tgt4, T, max_d, tgt_nrm4=None, nearest=None):
    """The record as a dict (the fields of qtr_eval_result but status and T), plus "corr" and the summed terms "S"."""
    e, corr = terms(src4, tgt4, T, max_d, tgt_nrm4, nearest)
    S = fold_sum(e)
    out = finish(S)
    out["corr"], out["S"] = corr, S
    return out


def same_record(got, want):
    """Names of the fields of `got` (a record dict of the device or of the compiled header) whose bits differ from want's."""
    bad = [f for f in FIELDS_INT if int(got[f]) != int(want[f])]
    bad += [f for f in FIELDS_F64 if not np.array_equal(bits(got[f]), bits(want[f]))]
    return bad


def open3d_information(tgt4, corr):
    """Open3D's GetInformationMatrixFromPointClouds spelled out: sum over the correspondences of G^T G with the 3 x 6
    G = [ -[t]x | I ] on the target point (rows (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1))."""
    corr = np.asarray(corr)
    t = B.f4(tgt4)[corr[corr >= 0], :3].astype(np.float64)
    G = np.zeros((t.shape[0], 3, 6))
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = z, -y, -z, x, y, -x
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    return np.einsum("nij,nik->jk", G, G)
