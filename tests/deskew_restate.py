"""The host restatement of sweep deskew (tests/deskew_ref/deskew_ref.cpp against include/qtr_deskew_math.h), compiled on
first use with g++ -ffp-contract=off and driven through ctypes: deskew mirrors quatro_amd.lib.Handle.deskew, pose_at mirrors
quatro_amd.lib.deskew_pose_at; atan, log and exp are the header's pieces.  Beside it an independent model in numpy
(model_*), which shares nothing with the header and takes sin, cos and arctan2 from numpy."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OK, BAD_K, BAD_TIME, BAD_POSE, BAD_ROTATION, BAD_TREF = 0, 1, 2, 3, 4, 5
MAX_KNOTS = 256
_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="deskew_ref_"), "libdeskew_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "deskew_ref", "deskew_ref.cpp"), "-o", out])
        lib = ctypes.CDLL(out)
        P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.deskew_ref_atan.restype = D
        lib.deskew_ref_atan.argtypes = [D]
        lib.deskew_ref_log.argtypes = [P, P]
        lib.deskew_ref_exp.restype = None
        lib.deskew_ref_exp.argtypes = [P, P]
        lib.deskew_ref_pose_at.argtypes = [P, P, I, D, P, P]
        lib.deskew_ref_interval.argtypes = [P, P, I, D, P, P]
        lib.deskew_ref_run.argtypes = [P, P, I, P, P, I, D, P, P]
        lib.deskew_ref_run_f64.argtypes = [P, P, I, P, P, I, D, P]
        _lib = lib
    return _lib


class Refused(ValueError):
    def __init__(self, why):
        super().__init__(f"refused ({why})")
        self.why = why


def _knots(knot_times, knot_poses):
    kt = np.ascontiguousarray(np.asarray(knot_times, np.float64).reshape(-1))
    kp = np.ascontiguousarray(np.asarray(knot_poses, np.float64).reshape(-1, 16))
    assert kt.shape[0] == kp.shape[0]
    return kt, kp


def atan(x: float) -> float:
    return float(load().deskew_ref_atan(float(x)))


def log(M):
    """Log of a relative rotation (3 x 3), or None where the header refuses it."""
    M, w = np.ascontiguousarray(np.asarray(M, np.float64).reshape(9)), np.zeros(3)
    return w if load().deskew_ref_log(M.ctypes.data, w.ctypes.data) else None


def exp(p):
    p, E = np.ascontiguousarray(np.asarray(p, np.float64).reshape(3)), np.zeros(9)
    load().deskew_ref_exp(p.ctypes.data, E.ctypes.data)
    return E.reshape(3, 3)


def pose_at(knot_times, knot_poses, t):
    """(T [4, 4], extrapolated) at time t."""
    kt, kp = _knots(knot_times, knot_poses)
    T, ex = np.zeros(16), ctypes.c_int(0)
    why = load().deskew_ref_pose_at(kt.ctypes.data, kp.ctypes.data, kt.shape[0], float(t), T.ctypes.data, ctypes.byref(ex))
    if why != OK:
        raise Refused(why)
    return T.reshape(4, 4), bool(ex.value)


def interval(knot_times, knot_poses, t):
    """(j, s) of time t."""
    kt, kp = _knots(knot_times, knot_poses)
    j, s = ctypes.c_int(0), ctypes.c_double(0)
    why = load().deskew_ref_interval(kt.ctypes.data, kp.ctypes.data, kt.shape[0], float(t), ctypes.byref(j), ctypes.byref(s))
    if why != OK:
        raise Refused(why)
    return j.value, s.value


def deskew(cloud, times, knot_times, knot_poses, t_ref=0.0):
    """(out [P, 4] float32, info dict): qtr_deskew restated."""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    times = np.ascontiguousarray(times, np.float32).reshape(-1)
    assert cloud.shape[0] == times.shape[0]
    kt, kp = _knots(knot_times, knot_poses)
    out, info = np.zeros_like(cloud), np.zeros(3, np.int32)
    why = load().deskew_ref_run(cloud.ctypes.data, times.ctypes.data, cloud.shape[0], kt.ctypes.data, kp.ctypes.data,
                                kt.shape[0], float(t_ref), out.ctypes.data, info.ctypes.data)
    if why != OK:
        raise Refused(why)
    return out, {"n_points": int(info[0]), "n_skipped": int(info[1]), "n_extrapolated": int(info[2])}


def deskew_f64(cloud, times, knot_times, knot_poses, t_ref=0.0):
    """The header's output points before their rounding to float32: [P, 3] float64 (zeros for a skipped point)."""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    times = np.ascontiguousarray(times, np.float32).reshape(-1)
    kt, kp = _knots(knot_times, knot_poses)
    q = np.zeros((cloud.shape[0], 3))
    why = load().deskew_ref_run_f64(cloud.ctypes.data, times.ctypes.data, cloud.shape[0], kt.ctypes.data, kp.ctypes.data,
                                    kt.shape[0], float(t_ref), q.ctypes.data)
    if why != OK:
        raise Refused(why)
    return q


# ---- an independent model: numpy's sin / cos / arctan2, no shared header ------------------------------------------------------
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def model_exp(p):
    """Rodrigues with 2 sin^2(th / 2) / th^2 for the second coefficient ((1 - cos th) / th^2 cancels at small th)."""
    p = np.asarray(p, np.float64)
    th = float(np.sqrt(p @ p))
    if th == 0.0:
        return np.eye(3)
    A = np.sin(th) / th
    B = 2.0 * np.sin(th / 2.0) ** 2 / (th * th)
    W = hat(p)
    return np.eye(3) + A * W + B * (W @ W)


def model_log(M):
    """The rotation vector of M from its antisymmetric part and trace: angle = arctan2(|a|, (trace - 1) / 2)."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    a = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])  # sin(th) axis
    la = float(np.sqrt(a @ a))
    if la == 0.0:
        return np.zeros(3)
    th = float(np.arctan2(la, 0.5 * (np.trace(M) - 1.0)))
    return a * (th / la)


def model_pose_at(knot_times, knot_poses, t):
    kt = np.asarray(knot_times, np.float64).reshape(-1)
    kp = np.asarray(knot_poses, np.float64).reshape(-1, 4, 4)
    j = int(np.clip(np.searchsorted(kt, t, side="right") - 1, 0, kt.shape[0] - 2))
    s = (t - kt[j]) / (kt[j + 1] - kt[j])
    T = np.eye(4)
    T[:3, :3] = kp[j, :3, :3] @ model_exp(s * model_log(kp[j, :3, :3].T @ kp[j + 1, :3, :3]))
    T[:3, 3] = kp[j, :3, 3] + s * (kp[j + 1, :3, 3] - kp[j, :3, 3])
    return T


def model_poses_at(knot_times, knot_poses, times):
    """model_pose_at for an array of times at once: (R [n, 3, 3], c [n, 3])."""
    kt = np.asarray(knot_times, np.float64).reshape(-1)
    kp = np.asarray(knot_poses, np.float64).reshape(-1, 4, 4)
    t = np.asarray(times, np.float64).reshape(-1)
    j = np.clip(np.searchsorted(kt, t, side="right") - 1, 0, kt.shape[0] - 2)
    s = (t - kt[j]) / (kt[j + 1] - kt[j])
    w = np.stack([model_log(kp[k, :3, :3].T @ kp[k + 1, :3, :3]) for k in range(kt.shape[0] - 1)])
    p = s[:, None] * w[j]
    th = np.sqrt(np.einsum("ni,ni->n", p, p))
    safe = np.where(th > 0.0, th, 1.0)
    A = np.where(th > 0.0, np.sin(safe) / safe, 1.0)
    B = np.where(th > 0.0, 2.0 * np.sin(safe / 2.0) ** 2 / (safe * safe), 0.5)
    W = np.zeros((t.shape[0], 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -p[:, 2], p[:, 1], p[:, 2], -p[:, 0], -p[:, 1], p[:, 0]
    E = np.eye(3)[None] + A[:, None, None] * W + B[:, None, None] * (W @ W)
    return kp[j, :3, :3] @ E, kp[j, :3, 3] + s[:, None] * (kp[j + 1, :3, 3] - kp[j, :3, 3])


def model_deskew(cloud, times, knot_times, knot_poses, t_ref=0.0):
    """The output points in float64 (not rounded to float32) of finite points; [P, 3]."""
    p = np.asarray(cloud, np.float32)[:, :3].astype(np.float64)
    t = np.asarray(times, np.float32).astype(np.float64)
    Tr = model_pose_at(knot_times, knot_poses, float(t_ref))
    R, c = model_poses_at(knot_times, knot_poses, t)
    world = np.einsum("nij,nj->ni", R, p) + c
    return (world - Tr[:3, 3]) @ Tr[:3, :3]
