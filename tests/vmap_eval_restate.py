"""The host restatement of the evaluation of a pose against the voxel map (tests/vmap_eval_ref/vmap_eval_ref.cpp against
include/qtr_vmap_eval_math.h), compiled on first use with g++ -ffp-contract=off and driven through ctypes with a map's
fetched sections (vmap_restate.RefMap.fetch_all, or the device map's fetches: the same keys)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import vmap_restate as M
from icp_restate import f4

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NT = 42
T_JTJ, T_JTR, T_R2, T_D2, T_CNT, T_W, T_MU, T_MUMU, T_NSRC = 0, 21, 27, 28, 29, 30, 32, 35, 41
FIELDS = ("valid", "n_source", "n_corr", "overlap", "sum_d2", "inlier_rmse", "sum_w", "chi2", "rmse", "information",
          "hessian", "gradient")
_lib = None


class Record(ctypes.Structure):  # QtrVmapEvalRecord
    _fields_ = [("valid", ctypes.c_int), ("n_source", ctypes.c_int), ("n_corr", ctypes.c_int), ("reserved", ctypes.c_int),
                ("overlap", ctypes.c_double), ("sum_d2", ctypes.c_double), ("inlier_rmse", ctypes.c_double),
                ("sum_w", ctypes.c_double), ("chi2", ctypes.c_double), ("rmse", ctypes.c_double),
                ("information", ctypes.c_double * 36), ("hessian", ctypes.c_double * 36), ("gradient", ctypes.c_double * 6)]


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vmap_eval_ref_"), "libvmap_eval_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall",
                               "-Werror", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "vmap_eval_ref", "vmap_eval_ref.cpp"), "-o", out])
        lib = ctypes.CDLL(out)
        P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.vmap_eval_ref_run.argtypes = [D, I, P, P, P, P, P, P, I, P, ctypes.POINTER(Record), P, P, P]
        lib.vmap_eval_ref_finish.restype = None
        lib.vmap_eval_ref_finish.argtypes = [P, ctypes.POINTER(Record)]
        lib.vmap_eval_ref_best.argtypes = [ctypes.POINTER(Record), I]
        lib.vmap_eval_ref_layout.restype = None
        lib.vmap_eval_ref_layout.argtypes = [P]
        _lib = lib
    return _lib


def record_dict(r: Record) -> dict:
    return {"valid": bool(r.valid), "n_source": r.n_source, "n_corr": r.n_corr, "overlap": r.overlap, "sum_d2": r.sum_d2,
            "inlier_rmse": r.inlier_rmse, "sum_w": r.sum_w, "chi2": r.chi2, "rmse": r.rmse,
            "information": np.array(r.information[:]).reshape(6, 6), "hessian": np.array(r.hessian[:]).reshape(6, 6),
            "gradient": np.array(r.gradient[:])}


def sections(m) -> dict:
    """What evaluate needs of a map: its voxel side and its COORDS, COUNT, SUMS and RECORDS sections.  m: a RefMap, or
    anything with fetch(what) and info() (the device's VoxelMap)."""
    side = float(m.voxel_size) if hasattr(m, "voxel_size") else float(m.info()["voxel_size"])
    sec = {k: np.ascontiguousarray(m.fetch(k)) for k in (M.COORDS, M.COUNT, M.SUMS, M.RECORDS)}
    sec["side"] = side
    return sec


def evaluate(sec, src, src_nrm, T) -> dict:
    """The restated evaluation of the cloud under T against the map whose sections `sec` holds (sections(), or a RefMap): the
    record's fields plus 'S' (the QTR_VMAP_EVAL_NT sums), 'corr' (int32 [n]) and 'point' (float64 [n, 2])."""
    if not isinstance(sec, dict):
        sec = sections(sec)
    src, nrm = f4(src), f4(src_nrm)
    assert src.shape == nrm.shape
    n = src.shape[0]
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))
    rec, S = Record(), np.zeros(NT)
    corr, point = np.full(max(n, 1), -1, np.int32), np.zeros((max(n, 1), 2))
    co, cn, su, re = (np.ascontiguousarray(sec[k]) for k in (M.COORDS, M.COUNT, M.SUMS, M.RECORDS))
    rc = load().vmap_eval_ref_run(sec["side"], int(cn.shape[0]), co.ctypes.data, cn.ctypes.data, su.ctypes.data, re.ctypes.data,
                                  src.ctypes.data, nrm.ctypes.data, n, T.ctypes.data, ctypes.byref(rec), S.ctypes.data,
                                  corr.ctypes.data, point.ctypes.data)
    assert rc == 0, "the map's RECORDS are not qtr_icp_voxel_finish of its SUMS and COUNT"
    out = record_dict(rec)
    out.update(S=S, corr=corr[:n].copy(), point=point[:n].copy())
    return out


def finish(S) -> dict:
    S = np.ascontiguousarray(np.asarray(S, np.float64).reshape(NT))
    rec = Record()
    load().vmap_eval_ref_finish(S.ctypes.data, ctypes.byref(rec))
    return record_dict(rec)


def best(rows) -> int:
    """qtr_vmap_eval_best over rows of (valid, n_corr, rmse)."""
    arr = (Record * max(len(rows), 1))()
    for a, (v, n, e) in zip(arr, rows):
        a.valid, a.n_corr, a.rmse = int(v), int(n), float(e)
    return int(load().vmap_eval_ref_best(arr, len(rows)))


def same_bits(a: dict, b: dict, fields=FIELDS) -> list:
    """The fields in which two evaluation dicts differ in any bit."""
    bad = []
    for k in fields:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f" or y.dtype.kind == "f":
            ok = np.array_equal(np.ascontiguousarray(x, np.float64).view(np.uint64), np.ascontiguousarray(y, np.float64).view(np.uint64))
        else:
            ok = np.array_equal(x, y)
        if not ok:
            bad.append(k)
    return bad
