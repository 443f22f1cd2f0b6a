"""Pose-graph optimisation without a GPU: include/qtr_pgo_math.h compiled by g++ equals the numpy float64 restatement
(tests/pgo_restate.py) bit for bit, piece by piece and over whole optimisations; the Jacobian against central differences of
the actual increment; the optimum against scipy.optimize.least_squares on the same residual; the line process prunes the
false loops and keeps the true ones; the two entry points are declared, exported, bound and refuse their arguments before
they touch a device; PoseGraph.add_loop takes the refined transform and the evaluation's information."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import pgo_host
import pgo_restate as pr
from pgo_host import host_run, restate_run, vp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ["qtr_default_pgo_params", "qtr_pgo_optimize"]

# Largest |J - central difference| / max|J| over the 50 random edges of the Jacobian test (h = 1e-6, rotations up to 60
# degrees), measured on the CPU and printed by the test: 2.8e-10 (the truncation and rounding of the difference quotient).
# Asserted: ten times that.
JACOBIAN_REL_MEASURED = 2.8e-10
# Case (a) of the independent optimum (noise-free 12-ring, drifted start), measured with the restatement: largest pose
# error against the truth 4.0e-15 (rotation entries and translations alike); F 8.4e+03 -> 2.5e-27, a ratio of 2.9e-31.
RING_TRUTH_MEASURED = 4.0e-15
# Case (b) (noisy Z): |F_ours - F_scipy| / F_scipy measured 2.4e-15.
RING_SCIPY_REL_MEASURED = 2.4e-15
TIGHT = dict(rel_tol=1e-30, step_tol=1e-14, pcg_tol=1e-13, pcg_max_iterations=400, max_iterations=60)


@pytest.fixture(scope="module")
def host():
    return pgo_host.build()


@pytest.fixture(scope="module")
def lib():
    from quatro_amd import build as qbuild
    qbuild.build(force=False, verbose=False)
    from quatro_amd import lib as ql
    return ql.load()


@pytest.fixture(scope="module")
def graphs():
    return pr.graphs()


def random_edges(n, seed, max_angle):
    rng = np.random.default_rng(seed)
    def poses():
        out = []
        for _ in range(n):
            w = rng.normal(size=3)
            w *= rng.uniform(0, max_angle) / np.linalg.norm(w)
            out.append(pr.rigid(w, rng.uniform(-20, 20, 3)))
        return np.stack(out)
    Xs, Xt, Zt = poses(), poses(), poses()
    Z = np.stack([pr.perturb(pr.measurement(Xs[k], Xt[k]), rng, 0.05, 0.3) if k % 2 else Zt[k] for k in range(n)])
    info = np.stack([pr.information(rng, 50) for _ in range(n)])
    return Xs.reshape(n, 16), Xt.reshape(n, 16), Z.reshape(n, 16), info.reshape(n, 36)


def test_header_pieces_equal_the_restatement_bit_for_bit(host):
    n = 40
    Xs, Xt, Z, info = random_edges(n, 5, np.pi / 3)
    r, J = pr.residual(Xs, Xt, Z)
    for mu, unc in ((0.0, 0), (7.5, 1), (7.5, 0), (-1.0, 1)):
        A, g, chi2, w, F = pr.edge_terms(Xs, Xt, Z, info, np.full(n, unc), mu)
        for k in range(n):
            hr, hJ, hA, hg, sc = np.zeros(6), np.zeros(36), np.zeros(21), np.zeros(6), np.zeros(3)
            host.residual(vp(Xs[k]), vp(Xt[k]), vp(Z[k]), vp(hr), vp(hJ))
            assert np.array_equal(pr.bits(hr), pr.bits(r[k])) and np.array_equal(pr.bits(hJ), pr.bits(J[k])), k
            host.edge_terms(vp(Xs[k]), vp(Xt[k]), vp(Z[k]), vp(info[k]), unc, mu, vp(hA), vp(hg), vp(sc))
            assert np.array_equal(pr.bits(hA), pr.bits(A[k])) and np.array_equal(pr.bits(hg), pr.bits(g[k])), (mu, unc, k)
            assert np.array_equal(pr.bits(sc), pr.bits([chi2[k], w[k], F[k]])), (mu, unc, k)
        assert (w == 1.0).all() == (not (unc and mu > 0))
    # the dot's shape: below, at and above one stride and one wave, and at 6 N = 1800 > 1024
    rng = np.random.default_rng(6)
    for m in (1, 63, 64, 65, 1023, 1024, 1025, 1800, 5000):
        a, b = rng.normal(size=m) * 10.0 ** rng.uniform(-6, 6, m), rng.normal(size=m)
        assert np.float64(host.dot(vp(a), vp(b), m)).view(np.uint64) == np.float64(pr.dot(a, b)).view(np.uint64), m
    # the increment
    x = rng.normal(size=(n, 6)) * 0.3
    Xn = pr.update(Xs, x)
    for k in range(n):
        h = np.zeros(16)
        host.update(vp(Xs[k]), vp(x[k]), vp(h))
        assert np.array_equal(pr.bits(h), pr.bits(Xn[k])), k


@pytest.mark.parametrize("name", ["n2_e1", "ring5", "n65_e70", "n300_e340"])
def test_whole_optimisations_equal_the_restatement_bit_for_bit(host, graphs, name):
    g = graphs[name]
    params = dict(max_iterations=12, pcg_max_iterations=60)
    if name == "n300_e340":
        from quatro_amd import api
        edges = [(0, 1, None, g["info"][e], g["unc"][e]) for e in range(len(g["src"]))]
        params["line_process_weight"] = api.default_line_process_weight(edges, 0.5)
        assert params["line_process_weight"] > 0 and 6 * 300 > 1024 and len(g["src"]) > 256 and g["unc"].sum() == 12
    rr = []
    want = restate_run(g, rr_log=rr, **params)
    got = host_run(host, g, **params)
    assert pr.differences(got, want) == [], (name, pr.differences(got, want))
    assert np.array_equal(pr.bits(got["pcg_rr"]), pr.bits(rr)), name  # one PCG solve, residual by residual
    assert want["iterations"] >= 1 and want["accepted"] >= 1 and want["objective_final"] < want["objective_initial"], name
    assert want["trace"].shape == (1 + want["iterations"], 8) and (want["trace"][1:, 4] >= 1).all()
    if name == "n300_e340":
        assert (want["weights"][g["unc"] != 0] < 1.0).any() and (want["weights"][g["unc"] == 0] == 1.0).all()


def test_stops_and_gauge(host, graphs):
    """Every stop reason but the ceiling is reached on purpose; a second component without a fixed node is optimised too."""
    g = graphs["n65_e70"]
    for params, reason in ((dict(max_iterations=2), pr.STOP_MAX_ITERATIONS), (dict(rel_tol=0.5), pr.STOP_RELATIVE),
                           (dict(step_tol=10.0), pr.STOP_STEP), (dict(max_iterations=0), pr.STOP_MAX_ITERATIONS)):
        want = restate_run(g, **params)
        assert want["stop_reason"] == reason and pr.differences(host_run(host, g, **params), want) == [], params
    a, b = graphs["ring5"], pr.ring(6, 1, 9, noise=(0.01, 0.05))
    two = dict(poses=np.concatenate([a["poses"], b["poses"]]), src=np.concatenate([a["src"], b["src"] + 5]),
               dst=np.concatenate([a["dst"], b["dst"] + 5]), Z=np.concatenate([a["Z"], b["Z"]]),
               info=np.concatenate([a["info"], b["info"]]), unc=np.concatenate([a["unc"], b["unc"]]))
    want = restate_run(two, max_iterations=15)
    assert pr.differences(host_run(host, two, max_iterations=15), want) == []
    assert want["objective_final"] < want["objective_initial"]
    assert not np.array_equal(want["poses"][5:], two["poses"].reshape(-1, 16)[5:])  # (the free component moved too)
    none = restate_run(dict(a, fixed=np.ones(5, np.uint8)))
    assert none["stop_reason"] == pr.STOP_NOTHING and np.array_equal(none["poses"], a["poses"].reshape(5, 16))


def test_jacobian_against_central_differences_of_the_actual_increment():
    """J_e against (r(delta = +h e_k) - r(-h e_k)) / 2h with the increment the optimiser applies (qtr_icp_rot_from_omega +
    qtr_icp_compose, restated), h = 1e-6, 50 random edges, rotations up to 60 degrees.  Measured on the CPU: 2.8e-10 (source 2.5e-10, target 2.7e-10) of the
    largest entry of J; asserted at ten times that.  d r / d delta_t = -J_e is what the code path does: one J per edge, the
    gradient and the product subtract it at t."""
    n, h = 50, 1e-6
    Xs, Xt, Z, _ = random_edges(n, 11, np.pi / 3)
    _, J = pr.residual(Xs, Xt, Z)
    worst = worst_t = 0.0
    for k in range(6):
        d = np.zeros((n, 6))
        d[:, k] = h
        num_s = (pr.residual(pr.update(Xs, d), Xt, Z)[0] - pr.residual(pr.update(Xs, -d), Xt, Z)[0]) / (2 * h)
        num_t = (pr.residual(Xs, pr.update(Xt, d), Z)[0] - pr.residual(Xs, pr.update(Xt, -d), Z)[0]) / (2 * h)
        scale = np.abs(J).max(axis=(1, 2))
        worst = max(worst, float((np.abs(num_s - J[:, :, k]).max(axis=1) / scale).max()))
        worst_t = max(worst_t, float((np.abs(num_t + J[:, :, k]).max(axis=1) / scale).max()))
    print(f"largest relative deviation of J from central differences: source {worst:.3e}, target (-J) {worst_t:.3e}")
    assert worst <= 10 * JACOBIAN_REL_MEASURED and worst_t <= 10 * JACOBIAN_REL_MEASURED, (worst, worst_t)
    # by construction: the gradient of a two-node graph is +g_e at s and -g_e at t, bit for bit
    A, g, _, _, _ = pr.edge_terms(Xs[:1], Xt[:1], Z[:1], np.eye(6).reshape(1, 36), np.zeros(1), 0.0)
    off, inc = pr.incidence(2, [0], [1])
    _, ng = pr.node_gather(2, off, inc, np.array([0]), A, g)
    assert np.array_equal(pr.bits(ng[0]), pr.bits(g[0])) and np.array_equal(pr.bits(ng[1]), pr.bits(-g[0]))


def _scipy_optimum(g):
    """least_squares on Omega^(1/2) r over left increments of the free nodes, from the same start."""
    from scipy.optimize import least_squares
    N, E = g["poses"].shape[0], len(g["src"])
    X0 = g["poses"].reshape(N, 16)
    Ls = [np.linalg.cholesky(g["info"][e]).T for e in range(E)]
    Z = g["Z"].reshape(E, 16)

    def fun(d):
        X = X0.copy()
        X[1:] = pr.update(X0[1:], d.reshape(N - 1, 6))
        r, _ = pr.residual(X[g["src"]], X[g["dst"]], Z)
        return np.concatenate([Ls[e] @ r[e] for e in range(E)])

    sol = least_squares(fun, np.zeros(6 * (N - 1)), xtol=1e-15, ftol=1e-15, gtol=1e-15, method="trf", x_scale=1.0)
    return float((fun(sol.x) ** 2).sum())


def _pose_error(X, truth):
    return float(np.abs(X.reshape(-1, 4, 4)[:, :3] - truth[:, :3]).max())


def test_optimum_against_scipy_least_squares():
    """(a) a noise-free 12-ring from a drifted start (0.05 rad / 0.3 m per step) reaches the truth: pose error measured 4.0e-15,
    asserted at ten times; F_final / F_initial measured 2.9e-31, asserted below 1e-20.  (b) the same ring with noisy Z (0.01
    rad / 0.05 m): |F_ours - F_scipy| / F_scipy measured 2.4e-15, asserted at ten times."""
    a = pr.ring(12, 0, 21, drift=(0.05, 0.3))
    ra = restate_run(a, **TIGHT)
    err = _pose_error(ra["poses"], a["truth"])
    print(f"(a) pose error {err:.3e}, F {ra['objective_initial']:.3e} -> {ra['objective_final']:.3e}, "
          f"{ra['iterations']} iterations, stop {ra['stop_reason']}")
    assert err <= 10 * RING_TRUTH_MEASURED, err
    assert ra["objective_final"] < 1e-20 * ra["objective_initial"]
    b = pr.ring(12, 0, 21, drift=(0.05, 0.3), noise=(0.01, 0.05))
    rb = restate_run(b, **TIGHT)
    Fs = _scipy_optimum(b)
    rel = abs(rb["objective_final"] - Fs) / Fs
    print(f"(b) F ours {rb['objective_final']:.15e}, scipy {Fs:.15e}, relative difference {rel:.3e}")
    assert rel <= 10 * RING_SCIPY_REL_MEASURED, rel


LINE_PROCESS_SEED = 3


def line_process_graph(seed=LINE_PROCESS_SEED):
    """A 16-ring with noisy odometry, 3 true and 2 false loop edges (Z random, information like the true ones), all five
    uncertain."""
    g = pr.ring(16, 3, seed, drift=(0.02, 0.1), noise=(0.005, 0.03), n_uncertain=3)
    rng = np.random.default_rng(1000 + seed)
    false = []
    while len(false) < 2:
        a, b = sorted(rng.choice(16, 2, replace=False))
        if 2 <= b - a <= 13:
            false.append((int(b), int(a)))
    w = rng.normal(size=(2, 3))
    Zf = np.stack([pr.rigid(w[k] / np.linalg.norm(w[k]) * rng.uniform(0.5, 2.5), rng.uniform(-6, 6, 3)) for k in range(2)])
    g["src"] = np.concatenate([g["src"], np.array([f[0] for f in false], np.int32)])
    g["dst"] = np.concatenate([g["dst"], np.array([f[1] for f in false], np.int32)])
    g["Z"] = np.concatenate([g["Z"], Zf])
    g["info"] = np.concatenate([g["info"], np.stack([pr.information(rng) for _ in range(2)])])
    g["unc"] = np.concatenate([g["unc"], np.ones(2, np.uint8)])
    g["true"], g["false"] = np.arange(16, 19), np.arange(19, 21)
    return g


def test_line_process_prunes_the_false_loops_and_keeps_the_true_ones():
    from quatro_amd import api
    g = line_process_graph()
    edges = [(int(g["src"][e]), int(g["dst"][e]), g["Z"][e], g["info"][e], bool(g["unc"][e])) for e in range(21)]
    assert g["unc"].sum() == 5 and list(np.flatnonzero(g["unc"])) == list(range(16, 21))
    mu = api.default_line_process_weight(edges, 0.5)
    assert mu == 0.25 * np.mean([g["info"][e][5, 5] for e in range(16, 21)])
    on = restate_run(g, line_process_weight=mu, max_iterations=60)
    off = restate_run(g, line_process_weight=0.0, max_iterations=60)
    print("weights of the uncertain edges:", on["weights"][16:], "pose error with / without the line process:",
          _pose_error(on["poses"], g["truth"]), _pose_error(off["poses"], g["truth"]))
    assert (on["weights"][g["false"]] < 0.25).all() and (on["weights"][g["true"]] > 0.25).all()
    assert on["n_pruned"] == 2 and off["n_pruned"] == 0 and (off["weights"] == 1.0).all()
    assert _pose_error(on["poses"], g["truth"]) < _pose_error(off["poses"], g["truth"])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib):
    from quatro_amd import lib as ql
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    declared = set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*\(", hdr))
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    for n in NAMES:
        assert n in declared and n in ql.EXPORTS and re.search(rf"\bT {n}\b", dyn), n
        assert getattr(lib, n).argtypes is not None, n
    assert len(lib.qtr_pgo_optimize.argtypes) == 15
    assert "#define QTR_PGO_MAX_NODES 65536" in hdr and ql.PGO_MAX_NODES == 65536
    assert "#define QTR_PGO_MAX_EDGES (1 << 20)" in hdr and ql.PGO_MAX_EDGES == 1 << 20
    assert "#define QTR_DBG_PGO_TRACE 19" in hdr and ql.DBG_PGO_TRACE == 19
    from quatro_amd import build as qbuild
    assert "qtr_pgo_math.h" in " ".join(qbuild.SOURCES) and "pgo.hip" in qbuild.SOURCES
    assert '#include "pgo.hip"' in open(os.path.join(ROOT, "quatro_amd", "csrc", "unity.hip")).read()
    assert "75 entry points" in open(os.path.join(ROOT, "README.md")).read() and len(ql.EXPORTS) == 75


def test_struct_sizes_match_a_compiled_c_program():
    from quatro_amd import lib as ql
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "quatro_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(qtr_pgo_params), sizeof(qtr_pgo_result), offsetof(qtr_pgo_params, rel_tol),
         offsetof(qtr_pgo_params, reserved), offsetof(qtr_pgo_result, objective_initial));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(ql.PgoParams), C.sizeof(ql.PgoResult), ql.PgoParams.rel_tol.offset, ql.PgoParams.reserved.offset,
                   ql.PgoResult.objective_initial.offset]
    assert got[:2] == [8 + 6 * 8 + 32, 32 + 24]


def test_the_abi_refuses_its_arguments_without_a_device(lib):
    """Every refusal of the validation list, with its message.  qtr_create hands back a handle even where no device can be
    opened (so that its error can be read): the argument checks answer on it before anything touches a device."""
    from quatro_amd import lib as ql
    bad, cap = ql.QTR_ERR_BAD_ARG, ql.QTR_ERR_CAPACITY
    prm = ql.default_pgo_params()
    assert (prm.max_iterations, prm.pcg_max_iterations, prm.rel_tol, prm.step_tol, prm.tau, prm.pcg_tol,
            prm.line_process_weight, prm.edge_prune_threshold, list(prm.reserved)) == (100, 500, 1e-6, 1e-9, 1e-5, 1e-8, 0.0,
                                                                                        0.25, [0] * 8)
    assert {k: prm.__getattribute__(k) for k in pr.DEFAULTS} == pr.DEFAULTS
    lib.qtr_default_pgo_params(None)  # (a NULL is ignored)
    g = pr.ring(5, 0, 2)
    X, _, src, dst, Z, info, unc = ql.pgo_arrays(g["poses"], [(int(g["src"][e]), int(g["dst"][e]), g["Z"][e], g["info"][e], 0)
                                                             for e in range(5)])
    out, w, res = np.zeros_like(X), np.zeros(5), ql.PgoResult()

    def call(h, N=5, X=X, fixed=None, E=5, src=src, dst=dst, Z=Z, info=info, prm=prm, out=out, res=res):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.qtr_pgo_optimize(h, 0, N, p(X), p(fixed), E, p(src), p(dst), p(Z), p(info), p(unc),
                                    None if prm is None else C.byref(prm), p(out), p(w), None if res is None else C.byref(res))

    res.status = 77
    assert call(None) == bad and res.status == 77  # (a call without a handle writes nothing)
    h = C.c_void_p()
    lib.qtr_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.qtr_create(0, None, C.byref(h))
    assert h, "qtr_create returns the handle even when it fails"
    lib.qtr_last_error.restype = C.c_char_p
    lib.qtr_last_error.argtypes = [C.c_void_p]
    try:
        def refused(code, text, **kw):
            res.status = 77
            assert call(h, **kw) == code, (text, lib.qtr_last_error(h))
            assert text in lib.qtr_last_error(h).decode(), (text, lib.qtr_last_error(h))
            assert kw.get("res", res) is None or res.status == code
        def changed(a, idx, v):
            b = a.copy()
            b.reshape(-1)[idx] = v
            return b
        for k in ("X", "out", "prm", "res"):
            refused(bad, "must not be NULL", **{k: None})
        for k in ("src", "dst", "Z", "info"):
            refused(bad, "must not be NULL with 5 edges", **{k: None})
        refused(bad, "0 nodes", N=0)
        refused(bad, "-1 edges", E=-1)
        refused(bad, "edge 2 names a node outside 0 .. 4", src=changed(src, 2, 5))
        refused(bad, "edge 3 names a node outside", dst=changed(dst, 3, -1))
        refused(bad, "edge 1 joins node", src=changed(src, 1, dst[1]))
        for v in (np.nan, np.inf):
            refused(bad, "pose 4 has a non-finite entry", X=changed(X, 4 * 16 + 7, v))
            refused(bad, "Z of edge 2 has a non-finite entry", Z=changed(Z, 2 * 16 + 11, v))
            refused(bad, "info of edge 4 has a non-finite entry", info=changed(info, 4 * 36 + 6 * 1 + 3, v))
        assert call(h, X=changed(X, 16 + 13, np.nan), info=changed(info, 36 + 6 * 3 + 1, np.nan)) != bad  # (never read)
        refused(bad, "no fixed node", fixed=np.zeros(5, np.uint8))
        for name in ("rel_tol", "step_tol", "tau", "pcg_tol"):
            for v in (0.0, -1.0, np.nan, np.inf):
                refused(bad, "is not finite and positive", prm=ql.default_pgo_params(**{name: v}))
        refused(bad, "max_iterations -1", prm=ql.default_pgo_params(max_iterations=-1))
        refused(bad, "pcg_max_iterations 0", prm=ql.default_pgo_params(pcg_max_iterations=0))
        refused(bad, "must be finite", prm=ql.default_pgo_params(line_process_weight=np.nan))
        refused(bad, "must be finite", prm=ql.default_pgo_params(edge_prune_threshold=np.inf))
        refused(cap, "exceed QTR_PGO_MAX_NODES", N=ql.PGO_MAX_NODES + 1)
        refused(cap, "exceed QTR_PGO_MAX_NODES", E=ql.PGO_MAX_EDGES + 1)
        assert lib.qtr_pgo_optimize(h, 99, 5, None, None, 0, None, None, None, None, None, None, None, None, None) == bad
        assert b"slot 99 out of range" in lib.qtr_last_error(h)
        # nothing to optimise needs no device either: all nodes fixed, and no edge
        for kw in (dict(fixed=np.ones(5, np.uint8)), dict(E=0)):
            assert call(h, **kw) == ql.QTR_OK and res.stop_reason == ql.PGO_STOP_NOTHING and res.valid == 1
            assert np.array_equal(out, X) and res.iterations == 0
    finally:
        lib.qtr_destroy.argtypes = [C.c_void_p]
        lib.qtr_destroy(h)


# ---- PoseGraph against faked close_loop outputs ---------------------------------------------------------------------------
def _loop(refined=True, evaluated=True, best=1):
    out = {"matches": [{"id": 4}, {"id": 9}, {"id": 2}], "best": best, "best_id": 9,
           "records": [{"valid": True, "T": np.eye(4) * (k + 1)} for k in range(3)]}
    if refined:
        out["refined"] = [{"status": 0 if k != 2 else 7, "T": np.eye(4) * (10 + k)} for k in range(3)]
    if evaluated:
        out["evaluations"] = [{"information": np.eye(6) * (100 + k)} if k != 0 else None for k in range(3)]
    return out


def test_pose_graph_add_loop_takes_the_refined_transform_and_the_evaluations_information(lib):
    from quatro_amd import api
    pg = api.PoseGraph()
    for k in range(12):
        pg.add_node(np.eye(4), fixed=(k == 0))
    e = pg.add_loop(11, _loop())
    s, t, T, info, unc = pg.edges[e]
    assert (s, t, T[0, 0], info[0, 0], unc) == (11, 9, 11.0, 101.0, True)  # refined over registration, best candidate
    s, t, T, info, unc = pg.edges[pg.add_loop(11, _loop(), use=2, uncertain=False)]
    assert (s, t, T[0, 0], info[0, 0], unc) == (11, 2, 3.0, 102.0, False)  # its refinement did not run: the registration's T
    s, t, T, info, unc = pg.edges[pg.add_loop(10, _loop(refined=False))]
    assert (s, t, T[0, 0], info[0, 0]) == (10, 9, 2.0, 101.0)
    for bad in (_loop(evaluated=False), _loop(best=-1), _loop(best=0)):  # no evaluate; no valid candidate; not evaluated
        with pytest.raises(ValueError):
            pg.add_loop(11, bad)
    with pytest.raises(ValueError):
        pg.add_edge(3, 3, np.eye(4), np.eye(6))
    with pytest.raises(ValueError):
        pg.add_edge(3, 12, np.eye(4), np.eye(6))
    assert pg.add_odometry(1, 0, {"valid": True, "T": np.eye(4)}, {"information": np.eye(6)}) == 3 and not pg.edges[3][4]
    with pytest.raises(ValueError):
        pg.add_odometry(2, 1, {"valid": True, "T": np.eye(4)}, None)

    class FakeHandle:
        def optimize_pose_graph(self, poses, edges, fixed, params, slot):
            self.seen = (np.array(poses), list(edges), fixed, params, slot)
            return np.array(poses) * 2.0, np.array([0.1, 1.0, 0.9, 1.0]), {"status": 0, "n_pruned": 1}

    h = FakeHandle()
    r = pg.optimize(h, params=None)
    assert r["pruned"] == [0] and h.seen[2][0] and not any(h.seen[2][1:]) and len(h.seen[1]) == 4
    assert pg.poses[5][0, 0] == 2.0 and len(pg.poses) == 12
    assert api.default_line_process_weight(pg.edges, 2.0, 0.5) == 0.5 * 4.0 * np.mean([101.0, 101.0])
    assert api.default_line_process_weight([pg.edges[1]], 2.0) == 0.0
