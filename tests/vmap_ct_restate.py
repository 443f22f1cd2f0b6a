"""The host restatement of the continuous-time registration (tests/vmap_ct_ref/vmap_ct_ref.cpp against
include/qtr_vmap_ct_math.h), compiled on first use with g++ -ffp-contract=off and driven through ctypes: register_ct mirrors
quatro_amd.lib.VoxelMap.register_ct over a RefMap of vmap_restate, pose_at mirrors quatro_amd.lib.ct_pose_at, point is one
point of one iteration.  Beside it an independent restatement in plain Python floats (py_*): the header's expressions typed
again in their order, with math.sqrt and math.floor as the only calls, so its results must equal the header's bit for bit."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

import vmap_restate as M
from icp_restate import f4

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SKIPPED, EXTRAPOLATED = 1, 2
STOP_MAX_ITERATIONS, STOP_TRANSFORMATION, STOP_FITNESS, STOP_TOO_FEW, STOP_DEGENERATE = 1, 2, 3, 4, 5
_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vmap_ct_ref_"), "libvmap_ct_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall",
                               "-Werror", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "vmap_ct_ref", "vmap_ct_ref.cpp"), "-o", out])
        lib = ctypes.CDLL(out)
        P, I, D, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
        lib.vmap_ct_ref_layout.restype = None
        lib.vmap_ct_ref_layout.argtypes = [P]
        lib.vmap_ct_ref_pose_at.argtypes = [D, D, P, P, D, P]
        lib.vmap_ct_ref_point.restype = None
        lib.vmap_ct_ref_point.argtypes = [D, D, P, P, P, P, F, D, P, I, P, P, P]
        lib.vmap_ct_ref_register.restype = None
        lib.vmap_ct_ref_register.argtypes = [P, P, P, I, D, P, I, P, P, D, D, P, P, D, D, I, I, P, P, P, P, P, I, P]
        _lib = lib
    return _lib


def _pose16(T):
    return np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))


def pose_at(t_begin, t_end, begin_pose, end_pose, t):
    """The 4 x 4 pose at time t, or None where the interval is refused."""
    B, E, T = _pose16(begin_pose), _pose16(end_pose), np.zeros(16)
    ok = load().vmap_ct_ref_pose_at(float(t_begin), float(t_end), B.ctypes.data, E.ctypes.data, float(t), T.ctypes.data)
    return T.reshape(4, 4) if ok else None


def point(t_begin, t_end, begin_pose, E, p, a, time, side, record=None, members=0):
    """One point under the iterate E: a dict of the header's intermediate results (see vmap_ct_ref_point)."""
    B, E = _pose16(begin_pose), _pose16(E)
    p4, a4 = np.zeros(4, np.float32), np.zeros(4, np.float32)
    p4[:3], a4[:3] = p, a
    iv, out, key = np.zeros(20), np.zeros(54), ctypes.c_ulonglong(0)
    rec = None if record is None else np.ascontiguousarray(record, np.float64)
    load().vmap_ct_ref_point(float(t_begin), float(t_end), B.ctypes.data, E.ctypes.data, p4.ctypes.data, a4.ctypes.data,
                             ctypes.c_float(float(np.float32(time))), float(side), None if rec is None else rec.ctypes.data,
                             int(members), iv.ctypes.data, out.ctypes.data, ctypes.byref(key))
    return {"admitted": bool(out[0]), "flags": int(out[1]), "ok": bool(out[2]), "T": out[3:15].copy(), "q": out[15:18].copy(),
            "r": out[18:21].copy(), "s": float(out[21]), "terms": out[22:54].copy(), "key": int(key.value), "iv": iv}


def register_ct(refmap, src, src_nrm, times, t_begin, t_end, begin_pose, guess_end=None, teps=1e-7, feps=1e-6, max_iter=30,
                min_corr=0, corr_iter=-1) -> dict:
    """The restated loop over a vmap_restate.RefMap: a dict shaped like lib.VoxelMap.register_ct's plus 'trace'
    (iterations x 18) and 'corr' (0 matched, -1 none, at evaluation corr_iter; < 0: the last)."""
    src, nrm = f4(src), f4(src_nrm)
    times = np.ascontiguousarray(times, np.float32).reshape(-1)
    assert src.shape == nrm.shape and times.shape[0] == src.shape[0]
    f = refmap.fetch_all()
    coords, count, records = (np.ascontiguousarray(f[k]) for k in (M.COORDS, M.COUNT, M.RECORDS))
    B = _pose16(begin_pose)
    g = B if guess_end is None else _pose16(guess_end)
    T, info, fr, ct = np.zeros(16), np.zeros(5, np.int32), np.zeros(2), np.zeros(3, np.int32)
    trace = np.zeros((max_iter, 18))
    corr = np.full(max(src.shape[0], 1), -1, np.int32)
    load().vmap_ct_ref_register(coords.ctypes.data, count.ctypes.data, records.ctypes.data, coords.shape[0], refmap.voxel_size,
                                src.ctypes.data, src.shape[0], nrm.ctypes.data, times.ctypes.data, float(t_begin), float(t_end),
                                B.ctypes.data, g.ctypes.data, teps, feps, max_iter, min_corr, T.ctypes.data, info.ctypes.data,
                                fr.ctypes.data, trace.ctypes.data, corr.ctypes.data, corr_iter, ct.ctypes.data)
    it = int(info[0])
    return {"status": 0, "T": T.reshape(4, 4), "iterations": it, "stop_reason": int(info[1]), "valid": bool(info[2]),
            "converged": bool(info[3]), "n_corr": int(info[4]), "fitness": fr[0], "rmse": fr[1],
            "trace": trace[:it].copy(), "corr": corr[:src.shape[0]].copy(),
            "info": {"n_points": int(ct[0]), "n_skipped": int(ct[1]), "n_extrapolated": int(ct[2])}}


# ---- the independent restatement: plain Python floats, the header's expressions in their order --------------------------------
W_MIN = 0.70710678118654757
K_EPS = 1.0 - 1e-3


def _finite(x):
    return (x - x) == 0.0


def py_atan(x):
    for _ in range(3):
        x = x / (1.0 + math.sqrt(1.0 + x * x))
    z = x * x
    p = 1.0 / float(2 * 12 + 1)
    for k in range(11, -1, -1):
        p = 1.0 / float(2 * k + 1) - z * p
    return 8.0 * (x * p)


def py_log(Mx):
    """(admitted, w) of a relative rotation given as 9 floats."""
    tr = (Mx[0] + Mx[4]) + Mx[8]
    arg = 1.0 + tr
    qw = math.sqrt(arg) / 2.0 if arg >= 0.0 else float("nan")
    if not (qw >= W_MIN):
        return False, [0.0, 0.0, 0.0]
    f = 4.0 * qw
    v0, v1, v2 = (Mx[7] - Mx[5]) / f, (Mx[2] - Mx[6]) / f, (Mx[3] - Mx[1]) / f
    n = math.sqrt((qw * qw + v0 * v0) + (v1 * v1 + v2 * v2))
    u = qw / n
    v0, v1, v2 = v0 / n, v1 / n, v2 / n
    lv = math.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
    if not (lv > 0.0):
        return True, [0.0, 0.0, 0.0]
    g = (2.0 * py_atan(lv / u)) / lv
    return True, [v0 * g, v1 * g, v2 * g]


def py_exp(p):
    t2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    A = B = 1.0
    for k in range(15, 0, -1):
        A = 1.0 - (t2 * (1.0 / float((2 * k) * (2 * k + 1)))) * A
        B = 1.0 - (t2 * (1.0 / float((2 * k + 1) * (2 * k + 2)))) * B
    B = B / 2.0
    x, y, z = p
    return [1.0 - B * (y * y + z * z), B * (x * y) - A * z, B * (x * z) + A * y,
            B * (x * y) + A * z, 1.0 - B * (x * x + z * z), B * (y * z) - A * x,
            B * (x * z) - A * y, B * (y * z) + A * x, 1.0 - B * (x * x + y * y)]


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def py_interval(t_begin, t_end, B, E):
    """(admitted, iv) with iv = dict(tau, div, R[9], c[3], dc[3], w[3]); B and E as 16 floats, from the END."""
    B, E = [float(x) for x in np.asarray(B).reshape(-1)], [float(x) for x in np.asarray(E).reshape(-1)]
    R = [E[4 * r + c] for r in range(3) for c in range(3)]
    Mx = [_dot3(E[r], B[c], E[4 + r], B[4 + c], E[8 + r], B[8 + c]) for r in range(3) for c in range(3)]
    ok, w = py_log(Mx)
    return ok, {"tau": float(t_end), "div": float(t_begin) - float(t_end), "R": R, "c": [E[3], E[7], E[11]],
                "dc": [B[4 * r + 3] - E[4 * r + 3] for r in range(3)], "w": w}


def _transform(T, x, y, z):
    return [((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3] for r in range(3)]


def py_key_of(X, side):
    i = []
    for a in range(3):
        v = X[a] / side
        if not _finite(v):
            return None
        fl = float(math.floor(v))
        if not (fl >= -1048576.0 and fl < 1048576.0):
            return None
        i.append(int(fl))
    kx, ky, kz = (v + 1048576 for v in i)
    return ((kz << 21) + ky) * 2097152 + kx


def py_point(iv, p, a, time, side, record=None, members=0):
    """qtr_vmap_ct_flags, qtr_vmap_ct_query and qtr_vmap_ct_terms of one point (float32 inputs) under the interval iv."""
    px, py_, pz = (float(np.float32(v)) for v in p)
    ax, ay, az = (float(np.float32(v)) for v in a)
    t = float(np.float32(time))
    out = {"flags": 0, "ok": False, "T": [0.0] * 12, "q": [0.0] * 3, "r": [0.0] * 3, "s": 0.0, "terms": [0.0] * 32, "key": 0}
    normal_ok = all(_finite(v) for v in (ax, ay, az)) and ((ax * ax + ay * ay) + az * az) > 0.0
    if not (all(_finite(v) for v in (px, py_, pz)) and _finite(t) and normal_ok):
        out["flags"] = SKIPPED
        return out
    u = (t - iv["tau"]) / iv["div"]
    out["flags"] = EXTRAPOLATED if (u < 0.0 or u > 1.0) else 0
    X = py_exp([u * iv["w"][0], u * iv["w"][1], u * iv["w"][2]])
    R, T = iv["R"], [0.0] * 12
    for r in range(3):
        for c in range(3):
            T[4 * r + c] = _dot3(R[3 * r], X[c], R[3 * r + 1], X[3 + c], R[3 * r + 2], X[6 + c])
        T[4 * r + 3] = iv["c"][r] + u * iv["dc"][r]
    q = _transform(T, px, py_, pz)
    Tr = list(T)
    Tr[3], Tr[7], Tr[11] = iv["c"]
    rr = _transform(Tr, px, py_, pz)
    s = 1.0 - u
    key = py_key_of(q, side)
    out.update(T=T, q=q, r=rr, s=s, ok=key is not None, key=key or 0)
    if key is None or record is None:
        return out
    mu, Cb = [float(v) for v in record[:3]], [float(v) for v in record[3:9]]
    la = math.sqrt((ax * ax + ay * ay) + az * az)
    a0, a1, a2 = ax / la, ay / la, az / la
    m0 = (T[0] * a0 + T[1] * a1) + T[2] * a2
    m1 = (T[4] * a0 + T[5] * a1) + T[6] * a2
    m2 = (T[8] * a0 + T[9] * a1) + T[10] * a2
    k = K_EPS
    s00 = Cb[0] + (1.0 - k * (m0 * m0))
    s01 = Cb[1] + -(k * (m0 * m1))
    s02 = Cb[2] + -(k * (m0 * m2))
    s11 = Cb[3] + (1.0 - k * (m1 * m1))
    s12 = Cb[4] + -(k * (m1 * m2))
    s22 = Cb[5] + (1.0 - k * (m2 * m2))
    d0, d1, dz = q[0] - mu[0], q[1] - mu[1], q[2] - mu[2]
    c00 = s11 * s22 - s12 * s12
    c01 = s02 * s12 - s01 * s22
    c02 = s01 * s12 - s02 * s11
    c11 = s00 * s22 - s02 * s02
    c12 = s01 * s02 - s00 * s12
    c22 = s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    M00, M01, M02, M11, M12, M22 = c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det
    q0, q1, q2 = rr  # (the lever stands where the rigid terms have q)
    e0 = (M00 * d0 + M01 * d1) + M02 * dz
    e1 = (M01 * d0 + M11 * d1) + M12 * dz
    e2 = (M02 * d0 + M12 * d1) + M22 * dz
    B00, B01, B02 = q1 * M02 - q2 * M01, q1 * M12 - q2 * M11, q1 * M22 - q2 * M12
    B10, B11, B12 = q2 * M00 - q0 * M02, q2 * M01 - q0 * M12, q2 * M02 - q0 * M22
    B20, B21, B22 = q0 * M01 - q1 * M00, q0 * M11 - q1 * M01, q0 * M12 - q1 * M02
    o = [q1 * B02 - q2 * B01, q2 * B00 - q0 * B02, q0 * B01 - q1 * B00, B00, B01, B02,
         q2 * B10 - q0 * B12, q0 * B11 - q1 * B10, B10, B11, B12,
         q0 * B21 - q1 * B20, B20, B21, B22,
         M00, M01, M02, M11, M12, M22,
         q1 * e2 - q2 * e1, q2 * e0 - q0 * e2, q0 * e1 - q1 * e0, e0, e1, e2,
         (d0 * e0 + d1 * e1) + dz * e2]
    w = float(members)
    o = [w * v for v in o]
    ss = s * s
    o = [ss * v for v in o[:21]] + [s * v for v in o[21:27]] + o[27:]
    out["terms"] = o + [(d0 * d0 + d1 * d1) + dz * dz, 1.0, w, 0.0]
    return out
