"""Named inputs for the pose-graph optimisation (qtr_pgo_optimize: k_pgo_linearize and k_pgo_step in quatro_amd/csrc/pgo.hip,
the contract include/qtr_pgo_math.h, the host driver in capi.hip).  A plain module: deterministic generators built on
pgo_restate's own (ring, perturb, information, measurement), no fixtures, no GPU work.  Used by
tests/test_pgo_cases_cpu.py (the header compiled by g++ against the numpy restatement, and every case against what it
claims) and tests/test_gpu_pgo_edges.py (the device against the restatement, bit for bit).

    case(name)    -> dict(poses, src, dst, Z, info, unc, fixed (None: node 0), params): cached, the arrays read-only
    expected(name)-> the restatement's record of the case (pgo_restate.optimize) with two logs added: "pcg_rr", <r, r> before
                     and after every iteration of the first solve, and "refusals", per preconditioner application the number
                     of free nodes whose block qtr_icp_solve6 refused.  Cached, computed once per process.
    WANTS[name]   -> a predicate of that record (and the case): the branch the case exists for.  It is a condition on the
                     REFERENCE: a change to a generator that moves a case off its branch fails the CPU test.

Every case is small enough for the restatement to take about 2 s or less.  The trace rows are those of qtr_pgo_decide:
[F_new, lambda after, rho, accepted, PCG iterations of the step judged, F after, denom, max_step]; row 0 is the start.
"""
import numpy as np

import pgo_restate as pr

MAX_ITERATIONS = 65536  # QTR_PGO_MAX_ITERATIONS (include/quatro_hip.h; compared by the CPU test)
STRIDE = dict(max_iterations=3, pcg_max_iterations=20)  # the stride and fold cases: cheap, the shapes are the point
NOISE = (0.01, 0.05)


def _seed(name):
    return [ord(c) for c in name]


def _graph(poses, src, dst, Z, info, unc=None, fixed=None, **params):
    E = len(src)
    return dict(poses=np.asarray(poses, np.float64), src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
                Z=np.asarray(Z, np.float64).reshape(E, 4, 4), info=np.asarray(info, np.float64).reshape(E, 6, 6),
                unc=np.zeros(E, np.uint8) if unc is None else np.asarray(unc, np.uint8),
                fixed=None if fixed is None else np.asarray(fixed, np.uint8), params=params)


def _ring(N, n_loops, seed, params=None, fixed=None, **kw):
    g = pr.ring(N, n_loops, seed, **kw)
    out = _graph(g["poses"], g["src"], g["dst"], g["Z"], g["info"], g["unc"], fixed, **(params or {}))
    out["truth"] = g["truth"]
    return out


def _fixed(N, *nodes):
    f = np.zeros(N, np.uint8)
    f[list(nodes)] = 1
    return f


def _with_edges(g, pairs, rng, noise=NOISE, unc=0):
    """g with the edges s -> t of `pairs` appended: measured on g's truth with noise, information like the others"""
    Z = [pr.perturb(pr.measurement(g["truth"][s], g["truth"][t]), rng, *noise) for s, t in pairs]
    g["src"] = np.concatenate([g["src"], np.array([p[0] for p in pairs], np.int32)])
    g["dst"] = np.concatenate([g["dst"], np.array([p[1] for p in pairs], np.int32)])
    g["Z"] = np.concatenate([g["Z"], np.stack(Z)])
    g["info"] = np.concatenate([g["info"], np.stack([pr.information(rng) for _ in pairs])])
    g["unc"] = np.concatenate([g["unc"], np.full(len(pairs), unc, np.uint8)])
    return g


def _long_ring(N, chords, fixed_node, rng):
    """pr.ring's trajectory, odometry edges and growing drift for the node counts past one pass of k_pgo_step, with the
    given chords and 20-point informations (ring's own 200-point ones cost seconds of generation at these sizes)"""
    R = N * 0.3
    truth = np.stack([pr.rigid([0.05 * np.sin(i), 0.03 * np.cos(2 * i), 2 * np.pi * i / N + np.pi / 2],
                               [R * np.cos(2 * np.pi * i / N), R * np.sin(2 * np.pi * i / N), 0.2 * np.sin(i)]) for i in range(N)])
    pairs = [(i + 1, i) for i in range(N - 1)] + [(0, N - 1)] + list(chords)
    Z = np.stack([pr.perturb(pr.measurement(truth[s], truth[t]), rng, *NOISE) for s, t in pairs])
    info = np.stack([pr.information(rng, 20) for _ in pairs])
    poses, acc = truth.copy(), np.eye(4)
    for i in range(1, N):
        acc = pr.rigid(rng.normal(0, 0.002, 3), rng.normal(0, 0.01, 3)) @ acc
        poses[i] = acc @ truth[i]
    g = _graph(poses, [p[0] for p in pairs], [p[1] for p in pairs], Z, info, None,
               None if fixed_node is None else _fixed(N, fixed_node), **STRIDE)
    g["truth"] = truth
    return g


def _star(n_leaves, hub, fixed_node, seed, **params):
    """N = n_leaves + 1 poses scattered at random, one edge leaf -> hub per leaf (ascending leaf index), noisy measurements,
    the start perturbed node by node"""
    rng = np.random.default_rng(seed)
    N = n_leaves + 1
    truth = np.stack([pr.rigid(rng.normal(0, 0.4, 3), rng.uniform(-20, 20, 3)) for _ in range(N)])
    pairs = [(i, hub) for i in range(N) if i != hub]
    Z = np.stack([pr.perturb(pr.measurement(truth[s], truth[t]), rng, *NOISE) for s, t in pairs])
    info = np.stack([pr.information(rng, 20) for _ in pairs])
    poses = np.stack([pr.perturb(truth[i], rng, 0.03, 0.2) for i in range(N)])
    g = _graph(poses, [p[0] for p in pairs], [p[1] for p in pairs], Z, info, None, _fixed(N, fixed_node), **params)
    g["truth"] = truth
    return g


def _false_loops(g, n_false, rng):
    """n_false uncertain chords with random measurements (information like the true ones) appended to g"""
    N = g["poses"].shape[0]
    false = []
    while len(false) < n_false:
        a, b = sorted(rng.choice(N, 2, replace=False))
        if 2 <= b - a <= N - 3:
            false.append((int(b), int(a)))
    w = rng.normal(size=(n_false, 3))
    Zf = np.stack([pr.rigid(w[k] / np.linalg.norm(w[k]) * rng.uniform(0.5, 2.5), rng.uniform(-6, 6, 3)) for k in range(n_false)])
    E0 = len(g["src"])
    g["src"] = np.concatenate([g["src"], np.array([f[0] for f in false], np.int32)])
    g["dst"] = np.concatenate([g["dst"], np.array([f[1] for f in false], np.int32)])
    g["Z"] = np.concatenate([g["Z"], Zf])
    g["info"] = np.concatenate([g["info"], np.stack([pr.information(rng) for _ in range(n_false)])])
    g["unc"] = np.concatenate([g["unc"], np.ones(n_false, np.uint8)])
    g["false"] = np.arange(E0, E0 + n_false)
    return g


def _mu(g, scale=0.5):
    """quatro_amd.api.default_line_process_weight restated: scale^2 times the mean translational information of the
    uncertain edges"""
    return float(scale * scale * np.mean([g["info"][e][5, 5] for e in np.flatnonzero(g["unc"])]))


def _rigid_inverse(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R.T, -(R.T @ t)
    return out


# ---------------------------------------------------------------------------------------------- the cases
REJECTS = dict(tau=1e-6, max_iterations=30)


def _rejecting_ring(**params):
    return _ring(12, 3, 4, params, drift=(0.8, 2.0), noise=NOISE)


def _outlier_ring(rng, **params):
    g = _ring(16, 3, 3, None, drift=(0.02, 0.1), noise=(0.005, 0.03), n_uncertain=3)
    g = _false_loops(g, 2, rng)
    g["params"] = dict(params, line_process_weight=_mu(g))
    return g


def _make(name):
    rng = np.random.default_rng(_seed(name))
    # ---- LM control
    if name == "rejects":
        return _rejecting_ring(**REJECTS)
    if name == "ends_on_a_reject":
        return _rejecting_ring(**dict(REJECTS, max_iterations=ENDS_ON_A_REJECT_AT))
    if name == "stop_lambda":
        return _ring(6, 1, 2, dict(step_tol=1e-300, rel_tol=1e-300, max_iterations=200))
    if name == "stop_step_at_optimum":
        return _ring(6, 1, 2, drift=(0.0, 0.0))
    if name == "stop_relative":
        return _ring(8, 1, 5, noise=NOISE)
    if name in ("max_iterations_0", "max_iterations_1"):
        return _ring(9, 2, 6, dict(max_iterations=int(name[-1])), noise=NOISE)
    if name == "max_iterations_ceiling":
        return _ring(9, 2, 6, dict(max_iterations=MAX_ITERATIONS), noise=NOISE)
    if name == "non_finite_start":
        g = _ring(6, 1, 2)
        g["poses"][3, 0, 3] = 1e200
        return g
    if name == "non_finite_trial":
        return _non_finite_trial()
    # ---- PCG
    if name == "pcg_cap_1":
        return _ring(40, 4, 2, dict(pcg_max_iterations=1, max_iterations=8), noise=NOISE)
    if name == "pcg_converges":
        return _ring(40, 4, 2, dict(pcg_max_iterations=400, pcg_tol=1e-12, max_iterations=8), noise=NOISE)
    if name == "zero_gradient":
        return _zero_gradient()
    if name == "precond_refuses":
        g = _ring(8, 1, 7, dict(max_iterations=6, pcg_max_iterations=20), noise=NOISE)
        on4 = (g["src"] == 4) | (g["dst"] == 4)
        g["info"][on4] = -0.01 * g["info"][on4]  # negative definite: D_4 + lambda I is too, solve6 refuses node 4
        return g
    # ---- strides and folds
    if name.startswith("nodes_"):
        N = int(name[6:])
        if N < 1024:
            return _ring(N, 3, N, STRIDE, noise=NOISE)
        if N == 1024:
            return _long_ring(N, [(700, 20), (1023, 400), (512, 3)], None, rng)
        far = {1025: [(1024, 500), (1024, 7), (900, 30)], 2049: [(2048, 1030), (1500, 1100), (2040, 3), (1024, 623)]}[N]
        return _long_ring(N, far, N - 1, rng)
    if name.startswith("edges_"):
        E = int(name[6:])
        N = 60 if E < 200 else 200  # (a ring has N edges already: E = 64 and 65 need fewer than 64 nodes)
        g = _ring(N, 0, E, STRIDE, noise=NOISE, extra=E - N)
        assert len(g["src"]) == E
        return g
    # ---- topology
    if name == "free_hub":
        return _star(300, 0, 300, 11, max_iterations=3, pcg_max_iterations=20)
    if name == "fixed_hub":
        return _star(100, 37, 37, 12, max_iterations=4, pcg_max_iterations=20)
    if name == "isolated_free_node":
        g = _ring(8, 1, 13, dict(max_iterations=6), noise=NOISE)
        lone = pr.rigid([0.3, -0.2, 0.9], [40.0, -3.0, 2.5])
        g["poses"] = np.concatenate([g["poses"][:4], lone[None], g["poses"][4:]])  # node 4 has no edge
        g["src"], g["dst"] = g["src"] + (g["src"] >= 4), g["dst"] + (g["dst"] >= 4)
        return g
    if name == "fixed_fixed_edge":
        return _ring(8, 1, 14, dict(max_iterations=6), _fixed(8, 0, 1), noise=NOISE)
    if name == "several_fixed":
        return _ring(12, 2, 15, dict(max_iterations=6), _fixed(12, 2, 5, 9), noise=NOISE)
    if name == "shuffled_edges":
        g = _ring(20, 6, 16, dict(max_iterations=6), noise=NOISE)
        E = len(g["src"])
        p, flip = rng.permutation(E), rng.random(E) < 0.5
        src, dst, Z = g["src"][p], g["dst"][p], g["Z"][p].copy()
        for e in np.flatnonzero(flip):  # the edge t -> s measures the inverse
            Z[e] = _rigid_inverse(Z[e])
        g.update(src=np.where(flip, dst, src).astype(np.int32), dst=np.where(flip, src, dst).astype(np.int32), Z=Z,
                 info=g["info"][p], unc=g["unc"][p], flipped=flip, order=p)
        return g
    if name == "parallel_edges_many":
        g = _ring(5, 0, 17, dict(max_iterations=6), noise=NOISE)
        return _with_edges(g, [(3, 1)] * 20, rng)
    # ---- line process and information
    if name == "mu_nonpositive":
        return _ring(10, 3, 18, dict(line_process_weight=-1.0, max_iterations=6), noise=NOISE, n_uncertain=3)
    if name == "all_uncertain":
        g = _ring(10, 3, 19, None, noise=NOISE, n_uncertain=13)
        g["params"] = dict(line_process_weight=_mu(g), max_iterations=8)
        return g
    if name == "outlier_loops":
        return _outlier_ring(rng, max_iterations=60)
    if name == "outlier_loops_ends_on_a_reject":
        return _outlier_ring(np.random.default_rng(_seed("outlier_loops")), max_iterations=OUTLIER_REJECT_AT,
                             **OUTLIER_REJECT_PARAMS)
    if name == "only_uncertain_edges_on_a_node":
        g = _ring(10, 0, 20, None, noise=NOISE)
        g["unc"] = ((g["src"] == 6) | (g["dst"] == 6)).astype(np.uint8)
        g["params"] = dict(line_process_weight=_mu(g), max_iterations=8)
        return g
    if name == "info_scales":
        g = _ring(10, 2, 21, dict(max_iterations=6), noise=NOISE)
        g["info"][1::3] *= 1e12
        g["info"][2::3] *= 1e-12
        return g
    if name == "zero_information":
        g = _ring(10, 2, 22, dict(max_iterations=6), noise=NOISE)
        g["info"][(g["src"] == 5) | (g["dst"] == 5)] = 0.0
        return g
    if name == "half_turn":
        g = _ring(6, 1, 23, dict(max_iterations=8), noise=NOISE)
        s, t = int(g["src"][2]), int(g["dst"][2])
        err = pr.rigid(np.array([0.6, -0.48, 0.64]) * (np.pi - HALF_TURN_GAP), [0.0, 0.0, 0.0])  # E_e at the start
        g["Z"][2] = _rigid_inverse(err) @ _rigid_inverse(g["poses"][t]) @ g["poses"][s]  # E = X_t^-1 X_s Z^-1
        return g
    raise KeyError(name)


HALF_TURN_GAP = 1e-9
# the first trial of `rejects` that is rejected right after an acceptance (read off its trace; the CPU test asserts that
# the run with max_iterations set to it ends on a rejection after at least one acceptance)
ENDS_ON_A_REJECT_AT = 3
# the outlier ring at tolerances it cannot meet rejects its trials from the eighth on (rounding is all that is left)
OUTLIER_REJECT_AT = 9
OUTLIER_REJECT_PARAMS = dict(rel_tol=1e-300, step_tol=1e-300)


def _zero_gradient():
    """Six poses of quarter turns and integer translations, every measurement the exact X_t^-1 X_s (integers throughout):
    every residual is 0.0, so g = 0, <r, r> = 0 at the entry of the solve, the loop body never runs, the step and
    delta^T (lambda delta - g) are 0."""
    quarter = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    poses = []
    for i in range(6):
        T = np.eye(4)
        T[:3, :3] = np.linalg.matrix_power(quarter, i % 4).round()
        T[:3, 3] = [i, 2 * i - 3, i % 2]
        poses.append(T)
    poses = np.stack(poses)
    pairs = [(i + 1, i) for i in range(5)] + [(0, 5), (4, 1)]
    Z = np.stack([(_rigid_inverse(poses[t]) @ poses[s]).round() for s, t in pairs])
    rng = np.random.default_rng(_seed("zero_gradient"))
    return _graph(poses, [p[0] for p in pairs], [p[1] for p in pairs], Z, [pr.information(rng) for _ in pairs])


def _non_finite_trial():
    """Two nodes, one edge.  The error at the start is a quarter turn about z short of c = 1e-150 (the matrix is written entry
    by entry: cos = c, sin = 1) with a lever of 2e4: r_z = 1, d r_z / d delta_z = c, d r_ty / d delta_z = 2e4.  The
    Gauss-Newton step is delta_z = -1 / c with a translation of 2e4 / c = 2e154 to match, whose chi2 overflows: F_new = inf and
    rho = -inf at every trial until lambda (from tau = 1e-30) has grown enough to shorten the step; then the trials are
    finite, still rejected, and lambda passes its ceiling.  F at the start is 1e299 and <g, g> 1e298: both finite."""
    c = 1e-150
    Xs = np.eye(4)
    Xs[:2, :2] = [[c, -1.0], [1.0, c]]
    Xs[0, 3] = 2e4
    info = np.diag([1.0, 1.0, 1e299, 1.0, 1.0, 1.0])
    return _graph(np.stack([np.eye(4), Xs]), [1], [0], [np.eye(4)], [info], tau=1e-30, max_iterations=80)


# ---------------------------------------------------------------------------------------------- what each case claims
def _acc(rec):
    return rec["trace"][1:, 3].astype(int)


def _pairs(rec, a, b):
    s = _acc(rec)
    return any(s[i] == a and s[i + 1] == b for i in range(len(s) - 1))


def _pcg_counts(rec):
    return rec["trace"][1:, 4].astype(int)


def _moved(rec, g):
    return not np.array_equal(rec["poses"], g["poses"].reshape(-1, 16))


def _free(g):
    N = g["poses"].shape[0]
    return np.arange(N) != 0 if g["fixed"] is None else g["fixed"] == 0


def _fixed_kept(rec, g):
    return np.array_equal(pr.bits(rec["poses"][~_free(g)]), pr.bits(g["poses"].reshape(-1, 16)[~_free(g)]))


def _stride(rec, g):
    """a stride or fold case ran its three trials with the PCG at its cap, moved every free node and no fixed one"""
    X0 = g["poses"].reshape(-1, 16)
    return (rec["iterations"] == 3 and rec["accepted"] >= 1 and rec["valid"] and (_pcg_counts(rec) == 20).all()
            and _fixed_kept(rec, g) and (rec["poses"][_free(g)] != X0[_free(g)]).any(axis=1).all())


WANTS = {
    "rejects": lambda r, g: (_pairs(r, 0, 0) and _pairs(r, 0, 1) and _pairs(r, 1, 0) and r["accepted"] < r["iterations"]
                             and r["valid"]),
    # the last evaluated trial is a rejection after at least one acceptance: the poses out are the accepted side's, which
    # is neither the start nor (checked against the longer run by the CPU test) the rejected trial
    "ends_on_a_reject": lambda r, g: (r["stop_reason"] == pr.STOP_MAX_ITERATIONS and _acc(r)[-1] == 0 and r["accepted"] >= 1
                                      and r["objective_final"] == r["trace"][-1, 5] != r["trace"][-1, 0] and _moved(r, g)),
    "stop_lambda": lambda r, g: (r["stop_reason"] == pr.STOP_LAMBDA and r["lambda_final"] > pr.LAMBDA_MAX and r["valid"]
                                 and _pairs(r, 0, 1) and _pairs(r, 1, 0) and r["accepted"] >= 2),
    "stop_step_at_optimum": lambda r, g: (r["stop_reason"] == pr.STOP_STEP and r["iterations"] == 0
                                          and r["pcg_rr"][0] > 0.0 and r["pcg_iterations_total"] >= 1),
    "stop_relative": lambda r, g: r["stop_reason"] == pr.STOP_RELATIVE and r["accepted"] == r["iterations"] >= 2,
    "max_iterations_0": lambda r, g: (r["stop_reason"] == pr.STOP_MAX_ITERATIONS and r["iterations"] == 0
                                      and r["pcg_iterations_total"] == 0 and r["trace"].shape == (1, 8) and not _moved(r, g)),
    "max_iterations_1": lambda r, g: (r["stop_reason"] == pr.STOP_MAX_ITERATIONS and r["iterations"] == 1
                                      and r["trace"].shape == (2, 8)),
    "max_iterations_ceiling": lambda r, g: (g["params"]["max_iterations"] == MAX_ITERATIONS
                                            and r["stop_reason"] in (pr.STOP_RELATIVE, pr.STOP_STEP)
                                            and 1 <= r["iterations"] < 100),
    "non_finite_start": lambda r, g: (not r["valid"] and r["stop_reason"] == pr.STOP_LAMBDA and r["iterations"] == 0
                                      and not np.isfinite(r["objective_initial"])
                                      and np.array_equal(pr.bits(r["poses"]), pr.bits(g["poses"]))),
    # F_new = inf at the first trials, finite at the later ones, every one rejected: the objective and the poses out are
    # the start's
    "non_finite_trial": lambda r, g: (np.isfinite(r["objective_initial"]) and r["valid"] and r["accepted"] == 0
                                      and np.isinf(r["trace"][1:3, 0]).all() and np.isinf(r["trace"][1:3, 2]).all()
                                      and np.isfinite(r["trace"][-3:, 0]).all() and r["stop_reason"] == pr.STOP_LAMBDA
                                      and r["objective_final"] == r["objective_initial"] and not _moved(r, g)),
    "pcg_cap_1": lambda r, g: (_pcg_counts(r) == 1).all() and r["iterations"] >= 3 and r["accepted"] >= 1,
    "pcg_converges": lambda r, g: (g["poses"].shape[0] >= 40 and (_pcg_counts(r) < 400).all() and (_pcg_counts(r) > 1).all()
                                   and len(set(_pcg_counts(r))) >= 2),
    "zero_gradient": lambda r, g: (r["pcg_rr"] == [0.0] and r["pcg_iterations_total"] == 0 and r["iterations"] == 0
                                   and r["stop_reason"] == pr.STOP_STEP and r["objective_initial"] == 0.0
                                   and r["lambda_final"] > 0.0),
    "precond_refuses": lambda r, g: max(r["refusals"]) >= 1 and r["iterations"] >= 1,
    "free_hub": lambda r, g: (_free(g)[0] and np.bincount(np.concatenate([g["src"], g["dst"]]))[0] == 300
                              and g["fixed"][300] == 1 and r["accepted"] >= 1 and _fixed_kept(r, g)
                              and not np.array_equal(r["poses"][0], g["poses"][0].reshape(16))),
    "fixed_hub": lambda r, g: (np.bincount(np.concatenate([g["src"], g["dst"]]))[37] == 100 and g["fixed"][37] == 1
                               and r["accepted"] >= 1 and _fixed_kept(r, g)),
    "isolated_free_node": lambda r, g: (_free(g)[4] and not ((g["src"] == 4) | (g["dst"] == 4)).any() and r["valid"]
                                        and np.array_equal(pr.bits(r["poses"][4]), pr.bits(g["poses"][4]))
                                        and r["accepted"] >= 1 and np.isfinite(r["trace"]).all()),
    "fixed_fixed_edge": lambda r, g: (((g["fixed"][g["src"]] == 1) & (g["fixed"][g["dst"]] == 1)).sum() == 1
                                      and r["accepted"] >= 1 and _fixed_kept(r, g)),
    "several_fixed": lambda r, g: g["fixed"].sum() == 3 and g["fixed"][0] == 0 and r["accepted"] >= 1 and _fixed_kept(r, g),
    "shuffled_edges": lambda r, g: (g["flipped"].any() and not g["flipped"].all() and (np.diff(g["order"]) < 0).any()
                                    and r["accepted"] >= 1),
    "parallel_edges_many": lambda r, g: ((g["src"] == 3) & (g["dst"] == 1)).sum() == 20 and r["accepted"] >= 1,
    "mu_nonpositive": lambda r, g: (g["unc"].sum() == 3 and g["params"]["line_process_weight"] < 0
                                    and (r["weights"] == 1.0).all() and r["n_pruned"] == 0 and r["accepted"] >= 1),
    "all_uncertain": lambda r, g: (g["unc"].all() and g["params"]["line_process_weight"] > 0 and (r["weights"] < 1.0).all()
                                   and r["accepted"] >= 1),
    "outlier_loops": lambda r, g: (r["n_pruned"] == 2 and (r["weights"][g["false"]] < 0.25).all()
                                   and (r["weights"][g["unc"] == 0] == 1.0).all()
                                   and (np.delete(r["weights"], g["false"]) >= 0.25).all()),
    "only_uncertain_edges_on_a_node": lambda r, g: (g["unc"].sum() == 2 and g["unc"][(g["src"] == 6) | (g["dst"] == 6)].all()
                                                    and (r["weights"][g["unc"] == 1] < 1.0).all() and r["accepted"] >= 1),
    "info_scales": lambda r, g: (g["info"][:, 5, 5].max() / g["info"][:, 5, 5].min() > 1e23 and r["accepted"] >= 1
                                 and r["valid"]),
    "zero_information": lambda r, g: (not g["info"][(g["src"] == 5) | (g["dst"] == 5)].any() and r["valid"]
                                      and np.array_equal(pr.bits(r["poses"][5]), pr.bits(g["poses"][5]))
                                      and r["accepted"] >= 1),
    "half_turn": lambda r, g: r["valid"] and r["iterations"] >= 1 and _half_turn_gap(g) < 2 * HALF_TURN_GAP,
}
for _n in (170, 171, 256, 257, 1024, 1025, 2049):
    WANTS[f"nodes_{_n}"] = lambda r, g, n=_n: (g["poses"].shape[0] == n and _stride(r, g) and (
        n <= 1024 or (g["fixed"][n - 1] == 1 and g["fixed"].sum() == 1
                      and (np.maximum(g["src"], g["dst"])[n:] >= 1024).any()  # (a loop closure past the first pass)
                      and (n == 1025 or (np.minimum(g["src"], g["dst"])[n:] >= 1024).any()))))
for _e in (64, 65, 256, 257, 512, 513):
    WANTS[f"edges_{_e}"] = lambda r, g, e=_e: len(g["src"]) == e and _stride(r, g)
WANTS["outlier_loops_ends_on_a_reject"] = lambda r, g: (
    WANTS["outlier_loops"](r, g) and r["stop_reason"] == pr.STOP_MAX_ITERATIONS and _acc(r)[-1] == 0 and r["accepted"] >= 1)


def _half_turn_gap(g):
    """pi minus the rotation angle of edge 2's error at the start (by the trace and the vee of E: angle = atan2(|vee|, ..))"""
    s, t = int(g["src"][2]), int(g["dst"][2])
    E = _rigid_inverse(g["poses"][t]) @ g["poses"][s] @ _rigid_inverse(g["Z"][2])
    sin = np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
    cos = (np.trace(E[:3, :3]) - 1) / 2
    return float(np.pi - np.arctan2(sin, cos))


NAMES = tuple(WANTS)

_cases, _expected = {}, {}


def case(name):
    """(cached: the arrays are shared and read-only)"""
    if name not in _cases:
        g = _make(name)
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cases[name] = g
    return _cases[name]


def restate(g, **logs):
    return pr.optimize(g["poses"], g["fixed"], g["src"], g["dst"], g["Z"], g["info"], g["unc"], **logs, **g["params"])


def expected(name):
    if name not in _expected:
        rr, refusals = [], []
        rec = restate(case(name), rr_log=rr, refusals=refusals)
        rec["pcg_rr"], rec["refusals"] = [float(x) for x in rr], refusals
        _expected[name] = rec
    return _expected[name]
