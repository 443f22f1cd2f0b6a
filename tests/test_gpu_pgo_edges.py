"""The pose-graph kernels (k_pgo_linearize, k_pgo_step and their host driver) on the named cases of tests/pgo_cases.py:
rejected steps and the two-sided buffers, every stop reason, a non-finite objective, the PCG's exits, node and edge counts on
either side of every stride and fold, hubs, isolated and fixed nodes, shuffled edge lists, the line process.  The device
must equal the numpy restatement (tests/pgo_restate.py) bit for bit — poses, weights, the result record and the
QTR_DBG_PGO_TRACE rows; no tolerance anywhere.  That the cases are on the branches they are named for is the CPU test's
business (tests/test_pgo_cases_cpu.py).  Everything goes through the C ABI (quatro_amd.lib)."""
import ctypes as C
import threading

import numpy as np
import pytest

import pgo_cases as pc
import pgo_restate as pr

pytestmark = pytest.mark.gpu

SEQUENCE = ("stop_lambda", "nodes_2049", "zero_gradient", "rejects", "non_finite_start", "non_finite_trial", "ring5")


@pytest.fixture(scope="module")
def hip():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


def _ring5():
    g = pr.graphs()["ring5"]
    return dict(poses=g["poses"], src=g["src"], dst=g["dst"], Z=g["Z"], info=g["info"], unc=g["unc"], fixed=None,
                params=dict(max_iterations=12, pcg_max_iterations=60))


def case(name):
    return _ring5() if name == "ring5" else pc.case(name)


_ring5_want = []


def expected(name):
    if name != "ring5":
        return pc.expected(name)
    if not _ring5_want:
        _ring5_want.append(pc.restate(_ring5()))
    return _ring5_want[0]


def edges_of(g):
    return [(int(g["src"][e]), int(g["dst"][e]), g["Z"][e], g["info"][e], bool(g["unc"][e])) for e in range(len(g["src"]))]


def device_run(h, g, slot=0):
    from quatro_amd import lib as ql
    X, w, res = h.optimize_pose_graph(g["poses"], edges_of(g), g["fixed"], ql.default_pgo_params(**g["params"]), slot)
    return dict(res, poses=X.reshape(-1, 16), weights=w, trace=h.debug_fetch(ql.DBG_PGO_TRACE, np.float64, slot).reshape(-1, 8))


def check(got, want, g, name):
    print(f"{name}: N {g['poses'].shape[0]} E {len(g['src'])} trials {want['iterations']} accepted {want['accepted']} PCG "
          f"{want['pcg_iterations_total']} stop {want['stop_reason']} valid {int(want['valid'])} pruned {want['n_pruned']}; "
          f"device: trials {got['iterations']} accepted {got['accepted']} PCG {got['pcg_iterations_total']} stop "
          f"{got['stop_reason']} valid {int(got['valid'])} pruned {got['n_pruned']}")
    assert got["status"] == 0, name
    assert got["n_pruned"] == want["n_pruned"] and bool(got["valid"]) == bool(want["valid"]), name
    assert pr.differences(got, want) == [], (name, pr.differences(got, want))
    assert got["trace"].shape == (1 + want["iterations"], 8), name


@pytest.mark.parametrize("name", pc.NAMES)
def test_device_equals_the_restatement_bit_for_bit(hip, name):
    g = pc.case(name)
    check(device_run(hip, g), pc.expected(name), g, name)


def test_one_slot_through_every_kind_of_stop():
    """One slot of one handle runs stop_lambda -> N = 2049 -> zero_gradient -> rejects -> the two non-finite objectives ->
    ring5: the arena grows and is reused by smaller graphs, the ticket, the state record and the trace start clean after a
    stop by lambda, by the iteration count, by the step, by the relative decrease and after an objective that is not finite.
    Every run equals what a fresh handle gives (the restatement: the test above)."""
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=1)
    try:
        stops = set()
        for name in SEQUENCE:
            g, want = case(name), expected(name)
            check(device_run(h, g), want, g, name)
            stops.add(want["stop_reason"])
        assert stops == {pr.STOP_LAMBDA, pr.STOP_MAX_ITERATIONS, pr.STOP_STEP, pr.STOP_RELATIVE}
    finally:
        h.close()


def test_two_slots_from_two_threads(hip):
    """`rejects` on slot 1 from a second thread while slot 0 runs N = 1025: the slots share nothing."""
    out = {}

    def run(name, slot):
        try:
            out[name] = device_run(hip, pc.case(name), slot)
        except BaseException as e:  # (reported by the main thread)
            out[name] = e

    t = threading.Thread(target=run, args=("rejects", 1))
    t.start()
    run("nodes_1025", 0)
    t.join()
    for name in ("nodes_1025", "rejects"):
        assert not isinstance(out[name], BaseException), (name, out[name])
        check(out[name], pc.expected(name), pc.case(name), name)


def test_poses_out_may_be_the_poses_in(hip):
    """Handle.optimize_pose_graph always hands the library an array of its own for poses_out; the C entry point takes
    poses_out == poses (the poses are uploaded before anything is written back), so that call goes through the bound
    function itself: `rejects`, whose answer is neither the start nor the last trial."""
    from quatro_amd import lib as ql
    g, want = pc.case("rejects"), pc.expected("rejects")
    X, fx, src, dst, Z, info, unc = ql.pgo_arrays(g["poses"], edges_of(g), g["fixed"])
    X = X.copy()
    w, res, prm = np.zeros(len(src)), ql.PgoResult(), ql.default_pgo_params(**g["params"])
    rc = hip._lib.qtr_pgo_optimize(hip._h, 0, int(X.shape[0]), X.ctypes.data, None, len(src), src.ctypes.data, dst.ctypes.data,
                                   Z.ctypes.data, info.ctypes.data, unc.ctypes.data, C.byref(prm), X.ctypes.data,
                                   w.ctypes.data, C.byref(res))
    assert rc == 0 and fx is None
    got = dict(ql._pgo_dict(res), poses=X, weights=w, trace=hip.debug_fetch(ql.DBG_PGO_TRACE, np.float64, 0).reshape(-1, 8))
    check(got, want, g, "rejects (in place)")
