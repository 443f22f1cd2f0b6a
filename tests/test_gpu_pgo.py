"""Pose-graph optimisation on the device (qtr_pgo_optimize): bit-exact against the numpy restatement (tests/pgo_restate.py) —
poses, weights, the result record and the per-iteration dump —, arena growth and the slot's other state, the capacity
refusal, the path place query -> registration -> evaluation -> optimisation end to end, and the C++ demo.  Everything goes
through the C ABI (quatro_amd.lib)."""
import os
import subprocess

import numpy as np
import pytest

import pgo_restate as pr

pytestmark = pytest.mark.gpu

PARAMS = dict(max_iterations=12, pcg_max_iterations=60)


@pytest.fixture(scope="module")
def hip():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


@pytest.fixture(scope="module")
def graphs():
    from quatro_amd import api
    g = pr.graphs()
    big = g["n300_e340"]
    big["params"] = dict(line_process_weight=api.default_line_process_weight(
        [(0, 1, None, big["info"][e], big["unc"][e]) for e in range(340)], 0.5))
    a, b = g["ring5"], pr.ring(6, 1, 9, noise=(0.01, 0.05))
    g["two_components"] = dict(poses=np.concatenate([a["poses"], b["poses"]]), src=np.concatenate([a["src"], b["src"] + 5]),
                               dst=np.concatenate([a["dst"], b["dst"] + 5]), Z=np.concatenate([a["Z"], b["Z"]]),
                               info=np.concatenate([a["info"], b["info"]]), unc=np.concatenate([a["unc"], b["unc"]]))
    g["all_fixed"] = dict(a, fixed=np.ones(5, np.uint8))
    g["no_edges"] = dict(poses=a["poses"], src=a["src"][:0], dst=a["dst"][:0], Z=a["Z"][:0], info=a["info"][:0], unc=a["unc"][:0])
    p = pr.ring(5, 0, 2, noise=(0.01, 0.05))  # the edge 1 -> 0 twice, the second time with another measurement
    g["parallel_edge"] = dict(poses=p["poses"], src=np.append(p["src"], p["src"][0]), dst=np.append(p["dst"], p["dst"][0]),
                              Z=np.concatenate([p["Z"], pr.perturb(p["Z"][0], np.random.default_rng(3), 0.01, 0.05)[None]]),
                              info=np.concatenate([p["info"], p["info"][1:2]]), unc=np.append(p["unc"], 0).astype(np.uint8))
    wants = {k: pr.optimize(v["poses"], v.get("fixed"), v["src"], v["dst"], v["Z"], v["info"], v["unc"],
                            **dict(PARAMS, **v.get("params", {}))) for k, v in g.items()}
    return g, wants


def edges_of(g):
    return [(int(g["src"][e]), int(g["dst"][e]), g["Z"][e], g["info"][e], bool(g["unc"][e])) for e in range(len(g["src"]))]


def device_run(h, g, slot=0, **params):
    from quatro_amd import lib as ql
    prm = ql.default_pgo_params(**dict(PARAMS, **g.get("params", {}), **params))
    X, w, res = h.optimize_pose_graph(g["poses"], edges_of(g), g.get("fixed"), prm, slot)
    return dict(res, poses=X.reshape(-1, 16), weights=w, trace=h.debug_fetch(ql.DBG_PGO_TRACE, np.float64, slot).reshape(-1, 8))


@pytest.mark.parametrize("name", ["n2_e1", "ring5", "n65_e70", "n300_e340", "two_components", "all_fixed", "no_edges",
                                  "parallel_edge"])
def test_device_equals_the_restatement_bit_for_bit(hip, graphs, name):
    g, wants = graphs
    got, want = device_run(hip, g[name]), wants[name]
    print(f"{name}: F {want['objective_initial']:.6e} -> {want['objective_final']:.6e}, {want['iterations']} iterations, "
          f"{want['pcg_iterations_total']} PCG iterations, stop {want['stop_reason']}")
    assert got["status"] == 0 and pr.differences(got, want) == [], (name, pr.differences(got, want))
    if name in ("all_fixed", "no_edges"):
        assert want["stop_reason"] == pr.STOP_NOTHING and got["trace"].shape == (0, 8)
        assert np.array_equal(got["poses"], g[name]["poses"].reshape(-1, 16))
    else:
        assert want["accepted"] >= 1 and want["objective_final"] < want["objective_initial"]


def test_arena_growth_and_the_slots_other_state(hip, graphs):
    """Two calls of different size on one slot equal the same calls on fresh handles (the restatement is what a fresh handle
    gives: the test above); a registration's state on the slot is what it was before the optimisation."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    g, wants = graphs
    h = ql.Handle(0, n_slots=1)
    try:
        s, t, _ = synth.kitti64_pair(3)
        with h.keyframe(s) as ks, h.keyframe(t) as kt:
            reg = h.register_keyframes(ks, kt, ql.default_frontend_params())
            corr = h.debug_fetch(ql.DBG_CORR, np.int32)
            ev = h.evaluate_pair()
            for name in ("ring5", "n300_e340", "n65_e70"):  # (small, grown, smaller again inside the grown arena)
                assert pr.differences(device_run(h, g[name]), wants[name]) == [], name
            assert np.array_equal(h.debug_fetch(ql.DBG_CORR, np.int32), corr)
            again = h.evaluate_pair()  # (still allowed: the slot's last working call is the registration)
            assert np.array_equal(pr.bits(again["information"]), pr.bits(ev["information"])) and again["n_corr"] == ev["n_corr"]
            assert np.array_equal(again["T"], reg["T"])
    finally:
        h.close()


def test_capacity_is_refused_and_the_slot_stays_usable(hip, graphs):
    from quatro_amd import lib as ql
    g, wants = graphs
    big = np.tile(np.eye(4).reshape(1, 16), (ql.PGO_MAX_NODES + 1, 1))
    with pytest.raises(ql.QuatroHipError) as e:
        hip.optimize_pose_graph(big, edges_of(g["n2_e1"]))
    assert e.value.code == ql.QTR_ERR_CAPACITY and "QTR_PGO_MAX_NODES" in str(e.value)
    assert pr.differences(device_run(hip, g["ring5"]), wants["ring5"]) == []


def _yaw_error(X, T):
    return float(np.abs(np.asarray(X)[:3] - T[:3]).max())


def test_place_query_to_optimised_poses_end_to_end():
    """A short synthetic trajectory with one revisit: odometry edges from register_one_to_many on neighbours (evaluated by
    evaluate_one_to_many), the loop from close_loop(..., evaluate=) through PoseGraph.add_loop, a deliberate drift in the
    initial poses.  The end pose is nearer the truth after the optimisation than before, and the loop edge is kept."""
    from quatro_amd import api
    from quatro_amd import lib as ql
    from quatro_amd import synth
    h = ql.Handle(0, n_slots=4)
    try:
        n = 7
        scans, truth = synth.kitti64_trajectory(0, n, 1.0)
        kfs = [h.keyframe(s, slot=i % 4) for i, s in enumerate(scans)]
        fp = ql.default_frontend_params(seed=0)
        ev_prm = ql.default_eval_params(max_correspondence_distance=0.5)
        pg = api.PoseGraph()
        rng = np.random.default_rng(1)
        drift = np.eye(4)
        for i in range(n + 1):  # node i: scan i; the revisit is the last node.  The drift grows along the trajectory
            pg.add_node(drift @ truth[i], fixed=(i == 0))
            drift = pr.rigid(rng.normal(0, 0.01, 3), rng.normal(0, 0.15, 3)) @ drift
        for i in range(1, n + 1):
            recs, ref, best = api.register_one_to_many(h, kfs[i], [kfs[i - 1]], fp, icp=ql.default_icp_params())
            assert best == 0 and ref[0]["status"] == 0, (i, recs[0])
            ev = api.evaluate_one_to_many(h, kfs[i], [kfs[i - 1]], [ref[0]["T"]], ev_prm)
            pg.add_odometry(i, i - 1, ref[0], ev[0])
        with h.place_index(n) as ix:
            for kf in kfs[:n - 2]:  # (the query's own neighbourhood is not searched)
                ix.add(kf)
            loop = api.close_loop(h, ix, kfs, kfs[n], 2, fp=fp, icp=ql.default_icp_params(), evaluate=ev_prm, min_overlap=0.5)
        assert loop["best"] >= 0, loop["matches"]
        e = pg.add_loop(n, loop)
        before = _yaw_error(pg.poses[n], truth[n])
        mu = api.default_line_process_weight(pg.edges, 0.5)
        res = pg.optimize(h, ql.default_pgo_params(line_process_weight=mu))
        after = _yaw_error(pg.poses[n], truth[n])
        print(f"loop {n} -> {loop['best_id']}: end-pose error {before:.4f} -> {after:.4f}, weight {res['weights'][e]:.4f}, "
              f"F {res['objective_initial']:.4e} -> {res['objective_final']:.4e}, {res['iterations']} iterations")
        assert res["status"] == 0 and res["valid"] and after < before
        assert e not in res["pruned"] and res["weights"][e] >= 0.25 and res["n_pruned"] == len(res["pruned"])
        for kf in kfs:
            kf.close()
    finally:
        h.close()


def test_cpp_pgo_demo_prints_what_the_python_call_returns(hip, graphs, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "pgo_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "pgo_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    g = graphs[0]["n300_e340"]
    mu = g["params"]["line_process_weight"]
    X, fx, src, dst, Z, info, unc = ql.pgo_arrays(g["poses"], edges_of(g), np.arange(300) == 0)
    path = str(tmp_path / "graph.bin")
    with open(path, "wb") as f:
        f.write(np.array([300, 340], np.int32).tobytes() + np.array([mu]).tobytes())
        for a in (X, fx, src, dst, Z, info, unc):
            f.write(a.tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    Xp, w, r = hip.optimize_pose_graph(g["poses"], edges_of(g), None, ql.default_pgo_params(line_process_weight=mu))
    assert out[0] == (f"status 0 valid {int(r['valid'])} iterations {r['iterations']} accepted {r['accepted']} pcg "
                      f"{r['pcg_iterations_total']} stop {r['stop_reason']} pruned {r['n_pruned']}"), out[0]
    words = np.array([int(x, 16) for ln in out[1:] for x in ln.split()], dtype=np.uint64).view(np.float64)
    assert np.array_equal(pr.bits(words[:3]), pr.bits([r["objective_initial"], r["objective_final"], r["lambda_final"]]))
    assert np.array_equal(pr.bits(words[3:3 + 4800]), pr.bits(Xp)) and np.array_equal(pr.bits(words[4803:]), pr.bits(w))
    assert r["iterations"] >= 1
