"""No-GPU: the host restatements' correspondence search (tests/icp_ref/icp_ref.cpp, tests/gicp_ref/gicp_ref.cpp: hash
grids, 27 cells) against the exhaustive reference of tests/icp_brute.py, on every case tests/test_gpu_icp_search.py
runs on the device — array equality — and every case's precondition from the reference alone.  The clouds of the
voxelised pair come from the CPU oracle's voxel grid and normals here, from the device's in the GPU file."""
import numpy as np
import pytest

import gicp_restate as G
import icp_brute as B
import icp_restate as R


class _OracleFront:
    def __init__(self, qo):
        self.qo = qo

    def voxelize(self, pts, leaf):
        return self.qo.voxelize(pts, leaf)

    def normals(self, pts, radius):
        return self.qo.fpfh(pts, radius, radius)[0]


@pytest.fixture(scope="module")
def vp(qo):
    return B.VoxPair(_OracleFront(qo))


def restated(c, method, **kw):
    kw = dict({"max_iter": 1, "corr_iter": 0}, **kw)
    if method == 2:
        return G.run(c.src, c.src_nrm, c.tgt, c.tgt_nrm, c.guess, max_d=c.max_d, **kw)
    return R.run(c.src, c.tgt, c.tgt_nrm, c.guess, max_d=c.max_d, method=method, **kw)


def check_restatement(c):
    raw = B.search(c.src, c.tgt, c.guess, c.max_d)[0]
    for method in (0, 1, 2):
        want = B.drop(raw, method, c.tgt_nrm, c.src_nrm)
        o = restated(c, method)
        bad = np.flatnonzero(o["corr"] != want)
        assert bad.size == 0, (c.name, method, bad.size, bad[:5], o["corr"][bad[:5]], want[bad[:5]])
        assert o["n_corr"] == int((want >= 0).sum()), (c.name, method)


@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_restatements_find_the_exhaustive_nearest_neighbour(vp, family):
    cases = B.FAMILIES[family](vp)
    assert cases
    for c in cases:
        print(c.name, c.src.shape[0], c.tgt.shape[0], c.max_d, c.check_pre())
        check_restatement(c)
    if family == "grid":
        print(B.check_grid_family(cases))


def test_all_non_finite_target_leaves_the_guess(vp):
    c = B.nonfinite_cases(vp)[-1]
    for method in (0, 1, 2):
        o = restated(c, method)
        assert not o["valid"] and o["n_corr"] == 0 and np.array_equal(o["T"], c.guess) and (o["corr"] == -1).all()
    assert (B.nearest(c.src, c.tgt, c.guess, c.max_d) == -1).all()


@pytest.mark.parametrize("ns,nt,max_d", B.BOX_SIZES)
def test_restatements_on_the_box_scene(ns, nt, max_d):
    s, sn, t, tn, guess = B.box_pair(ns, nt, seed=ns + nt)
    check_restatement(B.Case(f"box_{ns}_{nt}_{max_d}", s, t, guess, max_d, sn, tn))


def test_reference_rules_on_a_hand_made_example():
    """The reference itself, where the answer is known without it: ties to the lowest index, d2 == max_d^2 kept, the next
    float above it dropped, non-finite points and each method's normals."""
    tgt = B.f4([[1, 0, 0], [-1, 0, 0], [np.nan, 0, 0], [0, 3, 0], [0, 3, 0], [0, 0, 10]])
    src = B.f4([[0, 0, 0], [0, 3.5, 0], [0, 0, 8.5], [0, 0, np.float32(8.5) - np.float32(1e-6)], [np.inf, 0, 0], [0, 0, 10]])
    tn = B.f4([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [np.nan, 0, 0]])
    sn = B.f4([[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]])
    corr, d2, ties = B.search(src, tgt, np.eye(4), 1.5, stats=True)
    assert corr.tolist() == [0, 3, 5, -1, -1, 5] and ties.tolist() == [2, 2, 1, 0, 0, 1]
    assert d2[2] == 2.25 and np.isinf(d2[3])
    assert B.nearest(src, tgt, np.eye(4), 1.5, tn, sn, 1).tolist() == [0, 3, 5, -1, -1, 5]
    assert B.nearest(src, tgt, np.eye(4), 1.5, tn, sn, 0).tolist() == [0, 3, -1, -1, -1, -1]
    assert B.nearest(src, tgt, np.eye(4), 1.5, tn, sn, 2).tolist() == [0, -1, -1, -1, -1, -1]
    n, mse = B.mse_count(src, tgt, np.eye(4), corr)
    assert n == 4 and mse == (1.0 + 0.25 + 2.25 + 0.0) / 4
    assert B.grid_of([0, 0, 0], [10, 10, 1], 1.0, 1 << 22)[1:] == ((10, 10, 1), 0)
    cell, dims, grown = B.grid_of([0, 0, 0], [100, 100, 100], 0.1, 1 << 20)
    assert grown > 0 and np.prod(dims) <= 1 << 20 and abs(cell / (0.1 * 1.001 * 1.25 ** grown) - 1) < 1e-12


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("max_d", [0.3, 1.0])
def test_restatements_search_exhaustively_at_every_iteration(vp, max_d, method):
    """Evaluation k of a full run, at T = trace[k - 1] (the guess for k = 0): the correspondences, the count and the MSE
    (relative bound (nchunk + 10) * 2^-53, derived in tests/test_gpu_icp_search.py) against the exhaustive reference."""
    c = vp.case(f"every_iteration_{max_d}", max_d)
    full = restated(c, method, max_iter=40, corr_iter=-1)
    trace, n_it = full["trace"], full["iterations"]
    assert full["valid"] and n_it >= 3
    bound = (-(-c.src.shape[0] // 256) + 10) * 2.0 ** -53
    for k in range(n_it):
        T = c.guess if k == 0 else trace[k - 1, :16].reshape(4, 4)
        want = B.nearest(c.src, c.tgt, T, max_d, c.tgt_nrm, c.src_nrm, method)
        assert np.array_equal(restated(c, method, max_iter=k + 1, corr_iter=k)["corr"], want), k
        count, mse = B.mse_count(c.src, c.tgt, T, want)
        assert trace[k, 17] == count and abs(trace[k, 16] - mse) <= bound * mse, (k, trace[k, 16:], count, mse)
    print(f"max_d {max_d} method {method}: {n_it} iterations")
