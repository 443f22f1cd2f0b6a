"""The ICP correspondence search on the MI355X (k_icp_iter / k_icp_iter_gicp and their grouped forms, the cell grid of
icp_grid_of) against the exhaustive reference of tests/icp_brute.py — array equality — across grid shapes: cells
enlarged under the single-pair cap (2^22) and under the batch cap (2^20) only, one-cell grids, grids flat in one or two
axes, queries in the layer outside the box and beyond it, cloud sizes on the chunk boundaries, exact ties and distances
exactly at the limit, map-sized and negative coordinates, signed zeros, non-finite points and normals; at every
iteration of a run; the batched path against the single-pair path where the two build different grids; one slot
through a large grid, a one-cell grid and a large one again.  Every case's result also stays bit-equal to the host
restatement.  tests/test_icp_brute_cpu.py runs the same cases through the restatement without a GPU."""
import math

import numpy as np
import pytest

import gicp_restate as G
import icp_brute as B
import icp_restate as R

pytestmark = pytest.mark.gpu

ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")


class _DeviceFront:
    def __init__(self, hip):
        self.hip = hip

    def voxelize(self, pts, leaf):
        return self.hip.voxelize(pts, leaf)

    def normals(self, pts, radius):
        return self.hip.fpfh(pts, radius, radius)[0]


@pytest.fixture(scope="module")
def vp(hip):
    return B.VoxPair(_DeviceFront(hip))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same_icp(a, b, what=""):
    assert a.get("status", 0) == b.get("status", 0), what
    assert np.array_equal(_bits(a["T"]), _bits(b["T"])), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _bits(a["fitness"]) == _bits(b["fitness"]) and _bits(a["rmse"]) == _bits(b["rmse"]), what


def device(h, c, method, max_iterations=1, slot=0):
    from quatro_amd import lib as ql
    prm = ql.default_icp_params(method=method, max_iterations=max_iterations, max_correspondence_distance=c.max_d)
    if method == 2:
        return h.gicp(c.src, c.tgt, c.src_nrm, c.tgt_nrm, c.guess, prm, slot=slot)
    return h.icp(c.src, c.tgt, c.tgt_nrm, c.guess, prm, slot=slot)


def restated(c, method, max_iter=1, corr_iter=0):
    if method == 2:
        return G.run(c.src, c.src_nrm, c.tgt, c.tgt_nrm, c.guess, max_d=c.max_d, max_iter=max_iter, corr_iter=corr_iter)
    return R.run(c.src, c.tgt, c.tgt_nrm, c.guess, max_d=c.max_d, method=method, max_iter=max_iter, corr_iter=corr_iter)


def check_case(hip, c):
    """One device call per method at T = guess: correspondences, n_corr and the trace's count against brute force; the
    whole record and the trace against the restatement."""
    from quatro_amd import lib as ql
    pre = c.check_pre()
    raw = B.search(c.src, c.tgt, c.guess, c.max_d)[0]
    counts = []
    for method in (0, 1, 2):
        want = B.drop(raw, method, c.tgt_nrm, c.src_nrm)
        count = int((want >= 0).sum())
        g = device(hip, c, method)
        corr = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
        trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
        bad = np.flatnonzero(corr != want) if corr.shape == want.shape else None
        assert bad is not None and bad.size == 0, (c.name, method, corr.shape, want.shape,
                                                   None if bad is None else (bad.size, bad[:5], corr[bad[:5]], want[bad[:5]]))
        assert g["n_corr"] == count, (c.name, method, g["n_corr"], count)
        assert trace.shape[0] == g["iterations"] and (g["iterations"] == 0 or trace[0, 17] == count), (c.name, method)
        o = restated(c, method)
        _same_icp(g, o, f"{c.name} method {method}")
        assert np.array_equal(_bits(trace), _bits(o["trace"])), (c.name, method)
        counts.append(count)
    print(f"{c.name}: ns {c.src.shape[0]} nt {c.tgt.shape[0]} max_d {c.max_d} correspondences {counts} {pre}")


@pytest.mark.parametrize("family", [f for f in B.FAMILIES if f != "non_finite"])
def test_search_equals_the_exhaustive_reference(hip, vp, family):
    cases = B.FAMILIES[family](vp)
    assert cases
    for c in cases:
        check_case(hip, c)
    if family == "grid":
        print(B.check_grid_family(cases))


def test_non_finite_points_and_normals(hip, vp):
    from quatro_amd import lib as ql
    scattered, all_nan = B.nonfinite_cases(vp)
    check_case(hip, scattered)
    assert (B.nearest(all_nan.src, all_nan.tgt, all_nan.guess, all_nan.max_d) == -1).all()
    for method in (0, 1, 2):  # no finite target point: no grid, valid = 0, T = guess
        g = device(hip, all_nan, method)
        assert not g["valid"] and g["n_corr"] == 0 and g["iterations"] == 0 and g["stop_reason"] == ql.ICP_STOP_TOO_FEW
        assert np.array_equal(_bits(g["T"]), _bits(all_nan.guess))
        _same_icp(g, restated(all_nan, method), f"all-NaN target, method {method}")


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("max_d", [0.3, 1.0])
def test_every_iteration_searches_like_the_exhaustive_reference(hip, vp, max_d, method):
    """Update k of a full run is made from the correspondences of evaluation k at T = trace[k - 1] (the guess for k = 0);
    the run cut at k + 1 iterations leaves that set behind.

    The MSE bound.  trace[k, 16] is sum(d2) / n with the sum in the device's fixed shape: every d2 passes through at most
    6 adds of the in-wave fold, 2 adds inside its chunk and nchunk - 1 sequential adds over the chunks, nchunk =
    ceil(ns / 256).  All summands are non-negative, so there is no cancellation and the computed sum is
    sum(d2_i (1 + e_i)) with |e_i| <= (nchunk + 7) u to first order, u = 2^-53; the division adds one u.  The reference
    (math.fsum, one division) is within 2 u of the exact mean.  The d2 values themselves are the same binary64 numbers
    on both sides.  Relative bound: (nchunk + 10) * 2^-53."""
    from quatro_amd import lib as ql
    c = vp.case(f"every_iteration_{max_d}", max_d)
    full = device(hip, c, method, max_iterations=40)
    trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    n_it = full["iterations"]
    assert full["valid"] and n_it >= 3 and trace.shape[0] == n_it
    o = restated(c, method, max_iter=40, corr_iter=-1)
    _same_icp(full, o, "full run")
    assert np.array_equal(_bits(trace), _bits(o["trace"]))
    bound = (math.ceil(c.src.shape[0] / 256) + 10) * 2.0 ** -53
    worst = 0.0
    for k in range(n_it):
        T = c.guess if k == 0 else trace[k - 1, :16].reshape(4, 4)
        gk = device(hip, c, method, max_iterations=k + 1)
        corr = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
        assert np.array_equal(_bits(gk["T"]), _bits(trace[k, :16].reshape(4, 4))), k
        want = B.nearest(c.src, c.tgt, T, max_d, c.tgt_nrm, c.src_nrm, method)
        assert np.array_equal(corr, want), (k, int((corr != want).sum()))
        count, mse = B.mse_count(c.src, c.tgt, T, want)
        assert trace[k, 17] == count, (k, trace[k, 17], count)
        rel = abs(trace[k, 16] - mse) / mse
        worst = max(worst, rel)
        assert rel <= bound, (k, trace[k, 16], mse, rel, bound)
    print(f"max_d {max_d} method {method}: {n_it} iterations, worst MSE error {worst:.3e} (bound {bound:.3e}), "
          f"last count {int(trace[-1, 17])}")


# ---- batch against single, on different grids ------------------------------------------------------------------------
TILT = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))


@pytest.fixture(scope="module")
def pairs():
    """The ten pairs of tests/test_gpu_icp_batch.py: kitti64_pair(0..4) and kitti64_pair_16k(0..4), every other one with
    its target tilted."""
    from quatro_amd import synth
    out = []
    for k in range(5):
        for big in (False, True):
            s, t, _ = (synth.kitti64_pair_16k if big else synth.kitti64_pair)(k)
            if (k + big) % 2 == 0:
                t = R.apply(TILT, t)
            out.append((s, t, 10 * k + big))
    return out


BATCH_MAX_D = (0.1, 0.3)


def _cells_of_both_caps(h1, max_d):
    from quatro_amd import lib as ql
    vt = h1.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
    mn, mx = B.bbox_of(vt)
    return B.grid_of(mn, mx, max_d, B.BATCH_CELLS)[0], B.grid_of(mn, mx, max_d, B.CELL_CAP)[0]


def test_batch_refine_equals_single_pair_where_their_grids_differ(pairs):
    from quatro_amd import lib as ql
    h1 = ql.Handle(0, n_slots=1)
    hb = ql.Handle(0, n_slots=16)
    try:
        single, cells = {}, {d: [] for d in BATCH_MAX_D}
        for i, (s, t, seed) in enumerate(pairs):
            for d in BATCH_MAX_D:
                for method in (0, 1, 2):
                    h1.register_pair(s, t, ql.default_frontend_params(seed=seed))
                    single[i, d, method] = h1.refine_pair(None, ql.default_icp_params(method=method,
                                                                                      max_correspondence_distance=d))
                cells[d].append(_cells_of_both_caps(h1, d))
        for d in BATCH_MAX_D:
            differ = [i for i, (c20, c22) in enumerate(cells[d]) if c20 != c22]
            print(f"max_d {d}: cell side under 2^20 / 2^22 per pair {[(round(a, 4), round(b, 4)) for a, b in cells[d]]}; "
                  f"different for pairs {differ}")
            assert differ, cells[d]
            for method in (0, 1, 2):
                icp = ql.default_icp_params(method=method, max_correspondence_distance=d)
                res, refined = hb.register_batch_refine(pairs, icp=icp)
                for i, g in enumerate(refined):
                    assert res[i]["status"] == ql.QTR_OK and g["status"] == ql.QTR_OK, (d, method, i)
                    _same_icp(g, single[i, d, method], f"max_d {d} method {method} pair {i}")
                print(f"max_d {d} method {method}: iterations {[g['iterations'] for g in refined]}, "
                      f"n_corr {[g['n_corr'] for g in refined]}")
    finally:
        h1.close()
        hb.close()


def test_one_to_many_refine_equals_single_pair_where_their_grids_differ(pairs):
    from quatro_amd import api
    from quatro_amd import lib as ql
    max_d = 0.3
    query = pairs[5][0]
    targets = [pairs[5][1], pairs[4][1], pairs[7][1]]  # (its own target, a small scan's, another large one's)
    fp = ql.default_frontend_params(seed=21)
    icp = ql.default_icp_params(max_correspondence_distance=max_d)
    h1 = ql.Handle(0, n_slots=1)
    hb = ql.Handle(0, n_slots=4)
    try:
        with hb.keyframe(query) as kq:
            cands = [hb.keyframe(t, slot=k % 4) for k, t in enumerate(targets)]
            recs, refined, _ = api.register_one_to_many(hb, kq, cands, fp, icp=icp)
            for c in cands:
                c.close()
        assert recs[0]["status"] == ql.QTR_OK and refined[0]["status"] == ql.QTR_OK and refined[0]["valid"]
        differ = []
        for k, t in enumerate(targets):
            if refined[k]["status"] != ql.QTR_OK:  # (a cross pair that did not register is not refined)
                continue
            h1.register_pair(query, t, fp)
            c20, c22 = _cells_of_both_caps(h1, max_d)
            differ.append(c20 != c22)
            _same_icp(refined[k], h1.refine_pair(None, icp), f"candidate {k}")
        print(f"one-to-many: {len(differ)} candidates refined, grids differ for {sum(differ)}")
        assert any(differ)
    finally:
        h1.close()
        hb.close()


# ---- slot hygiene ---------------------------------------------------------------------------------------------------------
def test_one_slot_through_large_one_cell_and_large_grids(vp, small_pair):
    """The cell table grows (0.02: the whole 2^22 cap), is reused for one cell (500), must be clean for the large grid
    again and for an ordinary one; afterwards the registration path gives what it gave before."""
    from quatro_amd import lib as ql
    s, t, _ = small_pair
    fp = ql.default_frontend_params(seed=2)
    h = ql.Handle(0)
    try:
        before = h.register_pair(s, t, fp)
        for max_d, method in ((0.02, 0), (500.0, 1), (0.02, 2), (0.3, 0)):
            c = vp.case(f"hygiene_{max_d}", max_d)
            g = device(h, c, method, max_iterations=3)
            corr = h.debug_fetch(ql.DBG_ICP_CORR, np.int32)
            fresh = ql.Handle(0)
            try:
                f = device(fresh, c, method, max_iterations=3)
                fcorr = fresh.debug_fetch(ql.DBG_ICP_CORR, np.int32)
            finally:
                fresh.close()
            _same_icp(g, f, f"max_d {max_d} method {method}")
            assert np.array_equal(corr, fcorr), (max_d, method)
            print(f"max_d {max_d} method {method}: dims {c.grid()[2]}, n_corr {g['n_corr']}, iterations {g['iterations']}")
        after = h.register_pair(s, t, fp)
    finally:
        h.close()
    for k in ("T", "clique", "final_inliers"):
        assert np.array_equal(before[k], after[k]), k
    assert (before["cost"], before["n_src"], before["n_tgt"], before["L"]) == (after["cost"], after["n_src"], after["n_tgt"],
                                                                              after["L"])

