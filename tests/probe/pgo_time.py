"""Times qtr_pgo_optimize against the host route a caller would otherwise have (not a test; no test asserts a time).

Graph: a ring of N poses with one loop edge per 16 nodes, noisy measurements, a drifted start; N = 256, 1024, 4096, 16384.
The two arms alternate call by call, median [min - max] of 5:
  device  Handle.optimize_pose_graph (one workgroup runs the PCG of every LM step)
  host    the restatement's linearisation (tests/pgo_restate.py) with scipy.sparse.linalg.spsolve on the assembled
          H + lambda I per LM step, the same LM rules, at most 16 threads
Also recorded: LM iterations, PCG iterations per LM step and microseconds per PCG iteration (device wall time of the call
divided by its PCG iterations: an upper bound, it includes the linearisations and the host waits).
Writes profiles/pgo_time.json.   usage: python tests/probe/pgo_time.py [--sizes 256,1024]"""
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pgo_restate as pr  # noqa: E402


def graph(N):
    g = pr.ring(N, N // 16, 7, drift=(0.002, 0.02), noise=(0.002, 0.01))
    return g, [(int(g["src"][e]), int(g["dst"][e]), g["Z"][e], g["info"][e], False) for e in range(len(g["src"]))]


def host_route(g, max_iterations, rel_tol=1e-6, tau=1e-5):
    """LM with a sparse direct solve per step: the edge terms are the restatement's, H is assembled in CSR."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    X = g["poses"].reshape(-1, 16).copy()
    N, src, dst = X.shape[0], g["src"].astype(np.int64), g["dst"].astype(np.int64)
    Z, info = g["Z"].reshape(-1, 16), g["info"].reshape(-1, 36)
    full = np.array([[pr.u(a, b) for b in range(6)] for a in range(6)])

    def lin(X):
        A, ge, _, _, F = pr.edge_terms(X[src], X[dst], Z, info, np.zeros(len(src)), 0.0)
        B = A[:, full]
        r6 = np.arange(6)
        rows, cols, vals = [], [], []
        for a_, b_, sgn in ((src, src, 1.0), (dst, dst, 1.0), (src, dst, -1.0), (dst, src, -1.0)):
            rows.append((6 * a_[:, None, None] + r6[None, :, None] + 0 * r6[None, None, :]).reshape(-1))
            cols.append((6 * b_[:, None, None] + 0 * r6[None, :, None] + r6[None, None, :]).reshape(-1))
            vals.append((sgn * B).reshape(-1))
        H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * N, 6 * N)).tocsr()
        gv = np.zeros((N, 6))
        np.add.at(gv, src, ge)
        np.add.at(gv, dst, -ge)
        return H[6:, 6:], gv[1:].reshape(-1), float(F.sum())

    H, gv, F = lin(X)
    lam, nu, its = tau * H.diagonal().max(), 2.0, 0
    I = sp.identity(H.shape[0], format="csr")
    while its < max_iterations:
        d = spsolve((H + lam * I).tocsc(), -gv)
        Xt = X.copy()
        Xt[1:] = pr.update(X[1:], d.reshape(-1, 6))
        Ht, gt, Ft = lin(Xt)
        its += 1
        rho = (F - Ft) / float(d @ (lam * d - gv))
        if rho > 0:
            done = F - Ft <= rel_tol * F
            X, H, gv, F = Xt, Ht, gt, Ft
            lam, nu = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0
            if done:
                break
        else:
            lam, nu = lam * nu, 2.0 * nu
    return F, its


def main():
    from quatro_amd import lib as ql
    sizes = [256, 1024, 4096, 16384]
    if "--sizes" in sys.argv:
        sizes = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    h = ql.Handle(0, n_slots=1)
    out = {"what": "qtr_pgo_optimize vs restatement linearisation + scipy spsolve per LM step; ms, median [min, max] of 5",
           "sizes": {}}
    stat = lambda v: [float(np.median(v)), float(min(v)), float(max(v))]
    try:
        for N in sizes:
            g, edges = graph(N)
            prm = ql.default_pgo_params(max_iterations=20)
            h.optimize_pose_graph(g["poses"], edges, None, prm)  # (arena, first-launch costs)
            dev, host, rec = [], [], None
            for _ in range(5):
                t0 = time.perf_counter()
                _, _, rec = h.optimize_pose_graph(g["poses"], edges, None, prm)
                dev.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                Fh, ih = host_route(g, 20)
                host.append(1e3 * (time.perf_counter() - t0))
            steps = max(rec["iterations"], 1)
            out["sizes"][str(N)] = {
                "edges": len(edges), "device_ms": stat(dev), "host_ms": stat(host), "lm_iterations_device": rec["iterations"],
                "lm_iterations_host": ih, "F_device": rec["objective_final"], "F_host": Fh,
                "pcg_iterations_total": rec["pcg_iterations_total"],
                "pcg_iterations_per_lm_step": rec["pcg_iterations_total"] / steps,
                "us_per_pcg_iteration_upper_bound": 1e3 * float(np.median(dev)) / max(rec["pcg_iterations_total"], 1)}
            print(N, json.dumps(out["sizes"][str(N)]), flush=True)
    finally:
        h.close()
    dst = os.path.join(ROOT, "profiles", "pgo_time.json")
    json.dump(out, open(dst, "w"), indent=1)
    print("wrote", dst)


if __name__ == "__main__":
    main()
