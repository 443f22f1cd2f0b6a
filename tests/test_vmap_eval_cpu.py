"""The evaluation of poses against the voxel map without a GPU: the header's entry points against the binding and
the extension library's symbol table (tests/ext_abi.py), the struct layouts, the restatement
(tests/vmap_eval_restate.py, g++ from include/qtr_vmap_eval_math.h) against an independent numpy implementation and against
the registration's own first iteration, what `information` means, qtr_vmap_eval_best against api.best_evaluation, the
named cases of tests/vmap_eval_cases.py (each makes the branch it claims), the pose-graph helpers on
tests/pgo_restate.optimize, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import ext_abi
import icp_restate as R
import pgo_restate as PG
import vmap_batch_cases as BC
import vmap_cases as K
import vmap_eval_cases as EC
import vmap_eval_restate as E
import vmap_restate as M

FIVE = {"qtr_default_vmap_eval_params", "qtr_voxel_map_evaluate", "qtr_voxel_map_evaluate_keyframe",
        "qtr_voxel_map_evaluate_batch", "qtr_voxel_map_eval_fetch"}

# Largest relative deviations (max |a - b| / max |b| per field) of the restatement from the independent numpy implementation
# on test_restatement_agrees_with_an_independent_numpy_implementation's scene, as measured; asserted at ten times.
NUMPY_DEV = {"overlap": 0.0, "sum_d2": 3.87e-16, "inlier_rmse": 3.29e-16, "sum_w": 0.0, "chi2": 6.3e-16, "rmse": 3.11e-16,
             "information": 1.42e-16, "hessian": 5.93e-16, "gradient": 9.28e-16}
# ... and of xi^T Omega xi from sum |exp(xi) mu - mu|^2 over 20 twists with |xi| <= 1e-4 (second order in |xi|)
INFO_DEV = 6.53e-6


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _evals(name, ref=None):
    build, items = EC.CASES[name]()
    sec = E.sections(ref if ref is not None else build(M.RefMap))
    return items, [E.evaluate(sec, p, a, T) for p, a, T in items]


# ---- symbol tables and layouts -------------------------------------------------------------------------------------------
def test_the_five_entry_points_are_declared_exported_and_bound():
    """The entry points of include/quatro_voxelmap_eval.h are five of libquatro_ext.so's exports; header and binding name the
    same five; libquatro_hip.so exports none of them."""
    assert ext_abi.check_header("quatro_voxelmap_eval.h") == FIVE


def test_struct_layouts_match_their_ctypes_mirrors():
    from quatro_amd import lib as ql
    got = np.zeros(24, np.int32)
    E.load().vmap_eval_ref_layout(got.ctypes.data)
    Rs, Pm = ql.VmapEvalResult, ql.VmapEvalParams
    want = [ctypes.sizeof(E.Record), ctypes.sizeof(Rs), ctypes.sizeof(Pm)]
    want += [getattr(Rs, f).offset for f in ("status", "valid", "n_source", "n_corr", "overlap", "sum_d2", "inlier_rmse", "sum_w",
                                             "chi2", "rmse", "information", "hessian", "gradient")]
    want += [Pm.per_point.offset, ql.VMAP_EVAL_MAX, ql.VMAP_EVAL_CORR, ql.VMAP_EVAL_POINT, ql.VMAP_EVAL_TIMES, E.NT,
             E.Record.overlap.offset, E.Record.information.offset]
    assert list(got) == want
    assert (int(got[0]), int(got[1]), int(got[2]), int(got[17]), int(got[21])) == (688, 688, 16, 1024, 42)
    assert [f for f, _ in Rs._fields_[1:]] == [f for f, _ in E.Record._fields_ if f != "reserved"]


# ---- the restatement against an independent implementation ----------------------------------------------------------------
def _numpy_evaluate(nm, src4, nrm4, T):
    """The evaluation with a dict keyed by voxel coordinates, np.linalg.inv and plain sums."""
    p, a = np.asarray(src4, np.float64)[:, :3], np.asarray(nrm4, np.float64)[:, :3]
    Rm, t = T[:3, :3], T[:3, 3]
    out = dict(n_source=0, n_corr=0, sum_d2=0.0, sum_w=0.0, chi2=0.0, information=np.zeros((6, 6)), hessian=np.zeros((6, 6)),
               gradient=np.zeros(6))
    for pi, ai in zip(p, a):
        if not np.isfinite(pi).all():
            continue
        out["n_source"] += 1
        la = np.linalg.norm(ai)
        if not (np.isfinite(ai).all() and la > 0):
            continue
        q = Rm @ pi + t
        c = tuple(int(v) for v in np.floor(q / nm.side))
        if c not in nm.vox:
            continue
        N, sx, smm = nm.vox[c]
        mu, m = sx / N, Rm @ (ai / la)
        Sigma = (np.eye(3) - (1 - K.EPS) * smm / N) + (np.eye(3) - (1 - K.EPS) * np.outer(m, m))
        Mi = np.linalg.inv(Sigma)
        d = q - mu
        skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        J = np.hstack([-skew(q), np.eye(3)])
        G = np.hstack([-skew(mu), np.eye(3)])
        out["n_corr"] += 1
        out["sum_d2"] += d @ d
        out["sum_w"] += N
        out["chi2"] += N * d @ Mi @ d
        out["hessian"] += N * J.T @ Mi @ J
        out["gradient"] += N * J.T @ Mi @ d
        out["information"] += G.T @ G
    out["overlap"] = out["n_corr"] / out["n_source"]
    out["inlier_rmse"] = np.sqrt(out["sum_d2"] / out["n_corr"])
    out["rmse"] = np.sqrt(out["chi2"] / out["sum_w"])
    return out


def test_restatement_agrees_with_an_independent_numpy_implementation():
    inserts = K.hand_built()[0]
    nm, ref = K.NumpyMap(K.SIDE), BC.hand_map(M.RefMap)
    for p, n, pose in inserts:
        nm.insert(p, n, pose)
    p, a = BC.plane_cloud(700, 91)
    T = BC.small(7)
    q = np.asarray(p, np.float64)[:, :3] @ T[:3, :3].T + T[:3, 3]
    f = q / K.SIDE - np.round(q / K.SIDE)
    assert np.abs(f).min() > 1e-9  # no coordinate within 1e-9 sides of a face: both sides pick the same voxel
    got, want = E.evaluate(ref, p, a, T), _numpy_evaluate(nm, p, a, T)
    assert (got["n_source"], got["n_corr"]) == (want["n_source"], want["n_corr"]) and got["n_corr"] > 100
    for k, bound in NUMPY_DEV.items():
        dev = float(np.max(np.abs(np.asarray(got[k]) - np.asarray(want[k]))) / np.max(np.abs(np.asarray(want[k]))))
        print(f"numpy deviation {k}: {dev:.3g}")
        assert dev <= 10.0 * bound, (k, dev)


def test_sums_are_the_ones_the_registration_linearises_on():
    """The evaluation at T against the first iteration of RefMap.register from guess T: the same matched set, n_corr, and —
    through fitness = sum_d2 / n_corr, rmse = sqrt(chi2 / sum_w) and the first update, which is qtr_icp_step of the 21 + 6
    places — the same sums, bit for bit."""
    ref = BC.hand_map(M.RefMap)
    for seed, T in ((92, BC.small(3)), (93, K.GUESS), (94, np.eye(4))):
        p, a = BC.plane_cloud(700, seed)
        e = E.evaluate(ref, p, a, T)
        r = ref.register(p, a, T, teps=0.0, feps=0.0, max_iter=1, corr_iter=0)
        assert r["valid"] and r["iterations"] == 1
        assert r["n_corr"] == e["n_corr"] == int(e["S"][E.T_CNT]) and np.array_equal(r["corr"], e["corr"])
        assert _bits(r["fitness"]) == _bits(e["sum_d2"] / e["n_corr"]) and _bits(r["rmse"]) == _bits(e["rmse"])
        assert _bits(e["sum_w"]) == _bits(e["S"][E.T_W]) and _bits(e["chi2"]) == _bits(e["S"][E.T_R2])
        # the update solves hessian x = -gradient: the restated step's T is [dR(x) | x_t] T
        x = np.linalg.solve(e["hessian"], -e["gradient"])
        step = r["trace"][0][:16].reshape(4, 4) @ np.linalg.inv(T)
        assert np.allclose(step[:3, 3], x[3:], atol=1e-9)
        assert np.allclose(step[:3, :3], PG.rot_from_omega(x[None, :3]).reshape(3, 3), atol=1e-9)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                assert _bits(e["hessian"][i, j]) == _bits(e["S"][k]) == _bits(e["hessian"][j, i])
                k += 1
        assert np.array_equal(_bits(e["gradient"]), _bits(e["S"][E.T_JTR:E.T_JTR + 6]))


def test_information_is_the_quadratic_form_of_the_voxel_means_motion():
    """xi^T Omega xi = sum |exp(xi) mu - mu|^2 to second order, xi = (rotation, translation), over the matched means."""
    items, evals = _evals("room")
    p, a, T = items[27]
    e = evals[27]
    ref = BC.room_map(M.RefMap)
    rec = {tuple(c): r[:3] for c, r in zip(ref.fetch(M.COORDS), ref.fetch(M.RECORDS))}
    q = np.asarray(p, np.float64)[:, :3] @ T[:3, :3].T + T[:3, 3]
    mu = np.array([rec[tuple(int(v) for v in np.floor(qi / BC.ROOM_SIDE))] for qi, c in zip(q, e["corr"]) if c == 0])
    assert len(mu) == e["n_corr"]
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(20):
        xi = rng.normal(size=6)
        xi *= rng.uniform(1e-5, 1e-4) / np.linalg.norm(xi)
        D = PG.rigid(xi[:3], xi[3:])
        moved = mu @ D[:3, :3].T + D[:3, 3]
        want = float(np.sum((moved - mu) ** 2))
        got = float(xi @ e["information"] @ xi)
        worst = max(worst, abs(got - want) / want)
    print(f"information: largest relative deviation {worst:.3g}")
    assert worst <= 10.0 * INFO_DEV


# ---- best ---------------------------------------------------------------------------------------------------------------
def test_best_equals_its_python_restatement():
    from quatro_amd import api

    def both(rows):
        c = E.best(rows)
        evs = [{"valid": bool(v), "n_corr": n, "rmse": r} for v, n, r in rows]
        assert c == api.best_evaluation(evs), rows
        order = api.evaluation_order(evs)
        assert sorted(order) == list(range(len(rows))) and (order[0] == c if c >= 0 else not any(v for v, _, _ in rows))
        # the order is the rule applied again and again
        left = list(range(len(rows)))
        for o in order:
            b = E.best([rows[i] for i in left])
            if b < 0:
                assert not rows[o][0]
                break
            assert left[b] == o
            left.pop(b)
        return c

    assert both([]) == -1
    assert both([(0, 100, 0.1), (0, 500, 0.1)]) == -1
    assert both([(1, 10, 0.5), (1, 30, 0.9), (1, 20, 0.1)]) == 1
    assert both([(1, 30, 0.5), (1, 30, 0.25), (1, 30, 0.75)]) == 1
    assert both([(1, 30, 0.5), (1, 30, 0.5), (1, 30, 0.5)]) == 0
    assert both([(0, 99, 0.0), (1, 30, 0.5), (1, 30, 0.5)]) == 1
    rng = np.random.default_rng(9)
    for _ in range(200):
        B = int(rng.integers(1, 65))
        both([(int(rng.integers(0, 2)), int(rng.integers(0, 4)), float(rng.integers(0, 3)) / 4) for _ in range(B)])


# ---- the named cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_case_makes_the_branch_it_claims(name):
    items, evals = _evals(name)
    EC.PREDICATES[name](items, evals)
    for e in evals:  # and the record is the finish of its sums
        assert not E.same_bits(E.finish(e["S"]), e)
        assert np.array_equal(e["information"], e["information"].T) and np.array_equal(e["hessian"], e["hessian"].T)


def test_room_winner_stands_among_the_first_scores():
    """The condition of relocalize(keep=): where the full batch's winner stands in the order of the 27 scores.  keep for the
    GPU test is that rank rounded up to the next multiple of 3."""
    from quatro_amd import api
    build, items = EC.room()
    ref = build(M.RefMap)
    sec = E.sections(ref)
    evals = [E.evaluate(sec, p, a, T) for p, a, T in items]
    results = [ref.register(p, a, T) for p, a, T in items[:27]]
    rank = EC.room_rank(evals, results)
    print(f"room: the winner {api.best_hypothesis(results)} stands {rank}. of 27 in the scores' order")
    assert rank == EC.ROOM_RANK and 1 <= rank <= EC.ROOM_KEEP_LIMIT and EC.ROOM_KEEP == 3 * -(-rank // 3)


# ---- the pose-graph helpers ----------------------------------------------------------------------------------------------
def test_pose_graph_localization_edges():
    from quatro_amd import api
    from quatro_amd import lib as ql
    _, evals = _evals("room")
    ev = dict(evals[27], status=0)
    g = api.PoseGraph()
    m = g.add_map_node()
    assert m == 0 and g.fixed == [True] and np.array_equal(g.poses[0], np.eye(4))
    n = g.add_node(BC.ROOM_TRUE)
    res = {"status": 0, "valid": True, "T": BC.ROOM_TRUE}
    k = g.add_localization(n, m, res, ev)
    s, t, T, info, unc = g.edges[k]
    assert (s, t, unc) == (n, m, False) and np.array_equal(T, BC.ROOM_TRUE) and np.array_equal(info, ev["information"])
    k = g.add_localization(n, m, res, ev, which="hessian", uncertain=True)
    assert np.array_equal(g.edges[k][3], ev["hessian"]) and g.edges[k][4] is True
    for bad in (lambda: g.add_localization(n, m, dict(res, valid=False), ev), lambda: g.add_localization(n, m, res, dict(ev, valid=False)),
                lambda: g.add_localization(n, m, res, None), lambda: g.add_localization(n, m, res, ev, which="plane"),
                lambda: g.add_localization(n, m, dict(res, status=7), ev)):
        with pytest.raises(ValueError):
            bad()
    # information[5][5] is n_corr: default_line_process_weight keeps its meaning
    assert api.default_line_process_weight([(n, m, BC.ROOM_TRUE, ev["information"], True)], 1.0) == float(ev["n_corr"])

    # a chain of six nodes whose odometry drifts 0.1 m per node and which starts 0.3 m off as a whole; nodes 2 and 5 are
    # localised in the map at their true poses
    truth = [R.rigid(R.rot(0.0, 0.0, 0.1 * i), [1.5 + 1.2 * i, 2.0 + 0.3 * i, 1.2]) for i in range(6)]
    drift = R.rigid(np.eye(3), [0.1, 0.0, 0.0])
    rng = np.random.default_rng(3)
    g = api.PoseGraph()
    m = g.add_map_node()
    start = [R.rigid(np.eye(3), [0.3, 0.0, 0.0]) @ truth[0]]
    Z = []
    for i in range(5):
        Z.append(np.linalg.inv(truth[i]) @ truth[i + 1] @ drift)  # (i + 1 -> i, with the drift)
        start.append(start[-1] @ Z[-1])
    ids = [g.add_node(X) for X in start]
    for i in range(5):
        g.add_edge(ids[i + 1], ids[i], Z[i], PG.information(rng))
    for i in (2, 5):
        g.add_localization(ids[i], m, {"status": 0, "valid": True, "T": truth[i]}, ev)
    X, fx, src, dst, Zs, info, unc = ql.pgo_arrays(np.stack(g.poses), g.edges, g.fixed)
    out = PG.optimize(X, fx, src, dst, Zs, info, unc)
    end = out["poses"].reshape(-1, 4, 4)
    e0 = [float(np.linalg.norm(start[i][:3, 3] - truth[i][:3, 3])) for i in range(6)]
    e1 = [float(np.linalg.norm(end[ids[i]][:3, 3] - truth[i][:3, 3])) for i in range(6)]
    print("chain: start errors", np.round(e0, 4), "end errors", np.round(e1, 4))
    assert np.array_equal(end[m], np.eye(4))
    assert all(b < a for a, b in zip(e0, e1))
    assert e1[2] < 0.1 * e0[2] and e1[5] < 0.1 * e0[5]


# ---- refusals that need no device -------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    from quatro_amd import lib as ql
    elib = ql.load_ext()
    prm = ql.default_vmap_eval_params()
    assert prm.per_point == 0 and ql.default_vmap_eval_params(True).per_point == 1
    res = (ql.VmapEvalResult * 2)()
    items = (ql.VmapRegItem * 2)()
    # a NULL handle is a bad slot for every entry, and nothing is written
    assert elib.qtr_voxel_map_evaluate_batch(None, 0, None, items, 2, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
    assert elib.qtr_voxel_map_evaluate(None, 0, None, None, None, 0, ql.MEM_HOST, None, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
    assert elib.qtr_voxel_map_evaluate_keyframe(None, 0, None, None, None, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
    assert elib.qtr_voxel_map_eval_fetch(None, 0, 0, ql.VMAP_EVAL_TIMES, None, 0) == -1
    elib.qtr_default_vmap_eval_params(None)  # (tolerated)
