"""include/qtr_pgo_math.h compiled by g++ and called through ctypes: the host side of the pose-graph optimisation's bit
contract.  A plain module (no fixtures): build() compiles the harness once per process, host_run() runs the header's serial
optimisation (qtr_pgo_reference) on a graph dict and returns the record pgo_restate.optimize returns, restate_run() runs the
numpy restatement on the same dict.  Used by tests/test_pgo_cpu.py and tests/test_pgo_cases_cpu.py."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pgo_restate as pr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

HOST_SRC = r'''
#include "qtr_pgo_math.h"
extern "C" {
void residual(const double* Xs, const double* Xt, const double* Z, double* r, double* J) { qtr_pgo_residual(Xs, Xt, Z, r, J); }
void edge_terms(const double* Xs, const double* Xt, const double* Z, const double* info, int unc, double mu, double* A,
                double* g, double* sc) { qtr_pgo_edge_terms(Xs, Xt, Z, info, unc, mu, A, g, sc); }
double dot(const double* a, const double* b, int n) { return qtr_pgo_dot_host(a, b, n); }
void update(const double* X, const double* x, double* Xn) { qtr_pgo_update_node(X, x, Xn); }
void run(const double* tol /* rel_tol, step_tol, tau, pcg_tol, mu */, int max_it, int pcg_max, int N, const double* poses,
         const unsigned char* fixed, int E, const int* src, const int* dst, const double* Z, const double* info,
         const unsigned char* unc, double* poses_out, double* weights, double* f_out /* F0, F, lambda */,
         int* i_out /* trials, accepted, pcg_total, reason */, double* trace, double* pcg_rr) {
  QtrPgoCfg c;
  c.rel_tol = tol[0]; c.step_tol = tol[1]; c.tau = tol[2]; c.pcg_tol = tol[3]; c.mu = tol[4];
  c.max_iterations = max_it; c.pcg_max_iterations = pcg_max;
  QtrPgoState st;
  qtr_pgo_reference(&c, N, poses, fixed, E, src, dst, Z, info, unc, poses_out, weights, &st, trace, pcg_rr);
  f_out[0] = st.F0; f_out[1] = st.F; f_out[2] = st.lambda;
  i_out[0] = st.trials; i_out[1] = st.accepted; i_out[2] = st.pcg_total; i_out[3] = st.reason;
}
}
'''

_lib = None


def build():
    """The harness as a ctypes library (compiled on the first call: g++ -O2 -ffp-contract=off)."""
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="qtr_pgo_host_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        cpp, so = os.path.join(tmp, "p.cpp"), os.path.join(tmp, "p.so")
        with open(cpp, "w") as f:
            f.write(HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), cpp,
                               "-o", so])
        lib = C.CDLL(so)
        lib.dot.restype = C.c_double
        lib.edge_terms.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_double] + [C.c_void_p] * 3
        _lib = lib
    return _lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_run(host, g, **params):
    P = dict(pr.DEFAULTS, **params)
    X = np.ascontiguousarray(np.asarray(g["poses"], dtype=np.float64).reshape(-1, 16))
    N, E = X.shape[0], len(g["src"])
    fixed = np.zeros(N, np.uint8)
    if g.get("fixed") is None:
        fixed[0] = 1
    else:
        fixed[:] = g["fixed"]
    src, dst = np.ascontiguousarray(g["src"], np.int32), np.ascontiguousarray(g["dst"], np.int32)
    Z, info = np.ascontiguousarray(g["Z"].reshape(E, 16)), np.ascontiguousarray(g["info"].reshape(E, 36))
    unc = np.ascontiguousarray(g["unc"], np.uint8)
    tol = np.array([P["rel_tol"], P["step_tol"], P["tau"], P["pcg_tol"], P["line_process_weight"]])
    out, w = np.zeros_like(X), np.zeros(E)
    f, i = np.zeros(3), np.zeros(4, np.int32)
    trace, rr = np.zeros((P["max_iterations"] + 1, 8)), np.full(P["pcg_max_iterations"] + 1, -1.0)
    host.run(vp(tol), P["max_iterations"], P["pcg_max_iterations"], N, vp(X), vp(fixed), E, vp(src), vp(dst), vp(Z), vp(info),
             vp(unc), vp(out), vp(w), vp(f), vp(i), vp(trace), vp(rr))
    return dict(valid=bool(np.isfinite(f[1])), iterations=int(i[0]), accepted=int(i[1]), pcg_iterations_total=int(i[2]),
                stop_reason=int(i[3]), n_pruned=int(((unc != 0) & (w < P["edge_prune_threshold"])).sum()),
                objective_initial=f[0], objective_final=f[1], lambda_final=f[2], poses=out, weights=w,
                trace=trace[:1 + int(i[0])], pcg_rr=rr[rr >= 0])


def restate_run(g, rr_log=None, **params):
    return pr.optimize(g["poses"], g.get("fixed"), g["src"], g["dst"], g["Z"], g["info"], g["unc"], rr_log=rr_log, **params)
