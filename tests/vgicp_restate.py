"""The host restatement of the device loop's voxelised plane-to-plane method (tests/vgicp_ref/vgicp_ref.cpp against
include/qtr_icp_math.h), compiled on first use with g++ -ffp-contract=off and driven through ctypes."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from icp_restate import f4

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CAPACITY = -1
_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vgicp_ref_"), "libvgicp_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vgicp_ref", "vgicp_ref.cpp"),
                               "-o", out])
        lib = ctypes.CDLL(out)
        P = ctypes.c_void_p
        lib.vgicp_ref_run.argtypes = [P, ctypes.c_int, P, P, ctypes.c_int, P, P, P, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_int, ctypes.c_int, P, P, P, P, P, ctypes.c_int, P, P]
        _lib = lib
    return _lib


def run(src, src_nrm, tgt, tgt_nrm, guess=None, max_d=1.0, teps=1e-7, feps=1e-6, max_iter=30, min_corr=0, corr_iter=-1,
        feed=None):
    """The restated loop; returns a dict shaped like lib.Handle.gicp's plus 'trace' (iterations x 18), 'corr', 'records'
    (n_t x 11: at a voxel's representative [N, mu, C_b, cell]) and 'grid' (origin, dims, cells); 'status' is CAPACITY when
    the rule's grid exceeds the cell cap.  feed: the order in which the targets are handed to their cells."""
    src, tgt, src_nrm, tgt_nrm = f4(src), f4(tgt), f4(src_nrm), f4(tgt_nrm)
    assert src_nrm.shape == src.shape and tgt_nrm.shape == tgt.shape
    g = np.ascontiguousarray(np.eye(4) if guess is None else np.asarray(guess, np.float64).reshape(4, 4))
    fd = None if feed is None else np.ascontiguousarray(feed, np.int32)
    assert fd is None or sorted(fd.tolist()) == list(range(tgt.shape[0]))
    T = np.zeros(16)
    info = np.zeros(5, np.int32)
    fr = np.zeros(2)
    trace = np.zeros((max_iter, 18))
    corr = np.full(max(src.shape[0], 1), -1, np.int32)
    rec = np.zeros((max(tgt.shape[0], 1), 11))
    grid = np.zeros(7)
    rc = load().vgicp_ref_run(src.ctypes.data, src.shape[0], src_nrm.ctypes.data, tgt.ctypes.data, tgt.shape[0],
                              tgt_nrm.ctypes.data, None if fd is None else fd.ctypes.data, g.ctypes.data, max_d, teps, feps,
                              max_iter, min_corr, T.ctypes.data, info.ctypes.data, fr.ctypes.data, trace.ctypes.data,
                              corr.ctypes.data, corr_iter, rec.ctypes.data, grid.ctypes.data)
    it = int(info[0])
    return {"status": rc, "T": T.reshape(4, 4), "iterations": it, "stop_reason": int(info[1]), "valid": bool(info[2]),
            "converged": bool(info[3]), "n_corr": int(info[4]), "fitness": fr[0], "rmse": fr[1],
            "trace": trace[:it].copy(), "corr": corr[:src.shape[0]].copy(), "records": rec[:tgt.shape[0]].copy(),
            "grid": grid}
