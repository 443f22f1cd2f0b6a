"""The host restatement of the device ICP loop (tests/icp_ref/icp_ref.cpp against include/qtr_icp_math.h), compiled on
first use with g++ -ffp-contract=off and driven through ctypes, plus small helpers the ICP tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="icp_ref_"), "libicp_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "icp_ref", "icp_ref.cpp"),
                               "-o", out])
        lib = ctypes.CDLL(out)
        P = ctypes.c_void_p
        lib.icp_ref_run.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, P, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P, P, ctypes.c_int]
        _lib = lib
    return _lib


def f4(a):
    a = np.asarray(a, dtype=np.float32)
    if a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
    return np.ascontiguousarray(a)


def run(src, tgt, nrm=None, guess=None, max_d=1.0, teps=1e-7, feps=1e-6, max_iter=30, method=0, min_corr=0,
        corr_iter=-1):
    """The restated loop; returns a dict shaped like lib.Handle.icp's plus 'trace' (iterations x 18) and 'corr'."""
    src, tgt = f4(src), f4(tgt)
    nrm = f4(nrm) if nrm is not None else np.zeros_like(tgt)
    g = np.ascontiguousarray(np.eye(4) if guess is None else np.asarray(guess, np.float64).reshape(4, 4))
    T = np.zeros(16)
    info = np.zeros(5, np.int32)
    fr = np.zeros(2)
    trace = np.zeros((max_iter, 18))
    corr = np.full(max(src.shape[0], 1), -1, np.int32)
    load().icp_ref_run(src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], nrm.ctypes.data, g.ctypes.data,
                       max_d, teps, feps, max_iter, method, min_corr, T.ctypes.data, info.ctypes.data, fr.ctypes.data,
                       trace.ctypes.data, corr.ctypes.data, corr_iter)
    it = int(info[0])
    return {"T": T.reshape(4, 4), "iterations": it, "stop_reason": int(info[1]), "valid": bool(info[2]),
            "converged": bool(info[3]), "n_corr": int(info[4]), "fitness": fr[0], "rmse": fr[1],
            "trace": trace[:it].copy(), "corr": corr[:src.shape[0]].copy()}


def rot(roll=0.0, pitch=0.0, yaw=0.0):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def apply(T, pts):
    out = f4(pts).copy()
    out[:, :3] = (out[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


def rot_err_deg(A, B):
    R = A[:3, :3].T @ B[:3, :3]
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


def box_scene(n_per_face=700, seed=0):
    """Points on the inside of a 20 x 14 x 6 m box with a few interior slabs (well-conditioned for both methods),
    and their exact normals."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    dims = np.array([20.0, 14.0, 6.0])
    for ax in range(3):
        for side in (0.0, 1.0):
            uv = rng.random((n_per_face, 3)) * dims
            uv[:, ax] = side * dims[ax]
            n = np.zeros((n_per_face, 3))
            n[:, ax] = 1.0
            pts.append(uv)
            nrm.append(n)
    for k in range(3):  # slabs at irregular places break the box's symmetries
        c = rng.random(3) * dims * 0.6 + dims * 0.2
        uv = c + (rng.random((300, 3)) - 0.5) * np.array([4.0, 3.0, 2.0])
        ax = k % 3
        uv[:, ax] = c[ax]
        n = np.zeros((300, 3))
        n[:, ax] = 1.0
        pts.append(uv)
        nrm.append(n)
    return f4(np.concatenate(pts) - dims / 2), f4(np.concatenate(nrm))
