"""The finalize stage on the named inputs of tests/finalize_cases.py: k_finalize (chain TIMs, gnc_wave / gnc3_wave, rotation
inliers, cote_axis4, final inliers) and the stage entry points that run the same device code, against the CPU oracle,
bit for bit (NaN equal to NaN, +inf to +inf).  What the cases reach that random data does not:

  * both sides of each layout switch of k_finalize (GNC arrays in LDS / scratch in both modes, the in-kernel range-sum
    chain behind them / at its scratch location, COTE in LDS / scratch), every parameter variant on the scratch side too;
  * the in-kernel range-sum chain itself (cote_noise_bound = 0: the host lays down no table), stale tables between calls;
  * mu = 1 / 0 in GNC and the NR == 0 fall-back behind it; exact, rank-deficient, mirrored, overflowing and non-finite TIMs;
  * COTE's median fall-back for keys shared by different X, NaN keys, a NaN first cost, a consensus of one, the unrolled
    running sums and their tails, the padding of the rank merge sort.

tests/test_finalize_cases_cpu.py holds the oracle to second restatements on the same inputs and the inputs to what they
claim (clique size, side of each switch).
"""
import os
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import finalize_cases as fc  # noqa: E402
from test_gpu_parity import _assert_same_solution  # noqa: E402

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=131072, max_voxels=32768, max_corr=8192)


def _assert_same_record(r, o, what=""):
    """_assert_same_solution plus the scalars k_finalize reports"""
    _assert_same_solution(r, o)
    assert r["gnc_iters"] == o["gnc_iters"], what
    assert list(r["n_card"]) == list(o["n_card"]), what
    assert fc.same_bits(r["cost"], o["cost"]), (what, r["cost"], o["cost"])
    assert r["n_rot_inliers"] == len(o["rot_inliers"]), what
    assert fc.same_bits(r["T"], o["T"]), what


def _solve_both(h, qo, c, **over):
    kw = dict(c.kw, **over)
    with np.errstate(all="ignore"):
        o = qo.solve(c.src, c.tgt, qo.default_params(**kw))
    return h.solve(c.src, c.tgt, ql.demo_params(**kw)), o


# ---------------------------------------------------------------------------------------------- stage entries
@pytest.mark.parametrize("name,dim", fc.GNC_CASES)
def test_gnc_stage_entries_match_oracle(hip, qo, name, dim):
    c = fc.gnc_case(name, dim)
    fo, fg = (qo.gnc_rotation2d, hip.gnc_rotation2d) if dim == 2 else (qo.gnc_rotation3d, hip.gnc_rotation3d)
    Ro, co, io, mo = fo(c.X, c.Y, c.noise_bound, c.gnc_factor, c.max_it, c.cost_thr)
    Rg, cg, ig, mg = fg(c.X, c.Y, c.noise_bound, c.gnc_factor, c.max_it, c.cost_thr)
    print(name, dim, "iters", ig, io, "cost", cg, co, "inliers", int(np.sum(mg)), int(np.sum(mo)))
    assert ig == io
    assert np.array_equal(np.asarray(mg, dtype=bool), mo)
    assert fc.same_bits(cg, co), (cg, co)
    assert fc.same_bits(Rg, Ro), (Rg, Ro)


@pytest.mark.parametrize("name", fc.COTE_NAMES)
def test_cote_stage_entries_match_oracle(hip, qo, name):
    c = fc.cote_case(name)
    uniform = np.isscalar(c.ranges)
    for median in (True, False):
        if name == "zero_range":
            # the stage entry's own contract is range > 0 (qtr_cote_estimate); the range of 0 reaches the device code
            # through qtr_solve with cote_noise_bound = 0 (test_cote_noise_bound_at_the_ends_of_its_range)
            with pytest.raises(ql.QuatroHipError) as ei:
                hip.cote_estimate(c.X, c.ranges, median)
            assert ei.value.code == ql.QTR_ERR_BAD_ARG
            continue
        eo, mo, no = qo.cote_estimate(c.X, c.ranges, median) if uniform else qo.cote_estimate_ranges(c.X, c.ranges, median)
        eg, mg, ng = hip.cote_estimate(c.X, c.ranges, median) if uniform else hip.cote_estimate_ranges(c.X, c.ranges, median)
        print(name, median, "est", eg, eo, "ncard", ng, no, "inliers", int(np.sum(mg)), int(np.sum(mo)))
        assert ng == no, (name, median)
        assert fc.same_bits(eg, eo), (name, median, eg, eo)
        assert np.array_equal(np.asarray(mg, dtype=bool), mo), (name, median)


# ---------------------------------------------------------------------------------------------- the whole back end
@pytest.mark.parametrize("name", fc.SOLVE_NAMES)
def test_solve_on_both_sides_of_every_layout_switch_matches_oracle(hip, qo, name):
    c = fc.solve_case(name)
    r, o = _solve_both(hip, qo, c)
    print(name, "clique", len(r["clique"]), "iters", r["gnc_iters"], "rot", r["n_rot_inliers"], "n_card", r["n_card"],
          "final", len(r["final_inliers"]), "cost", r["cost"])
    assert len(o["clique"]) == c.M and o["valid"]
    _assert_same_record(r, o, name)
    if name.startswith("mu_inf"):  # NR == 0: COTE runs on the whole clique whatever the rot-inlier option says
        assert r["n_rot_inliers"] == 0 and r["gnc_iters"] == 50 and len(r["final_inliers"]) == 4


def test_cote_noise_bound_sequence_on_one_handle_rewrites_and_bypasses_the_range_table(qo):
    """0.3 -> 0.15 -> 0.0 -> 0.3 at M = 433: the host's table of range sums rewritten, then stale while the chain runs in
    the kernel, then rewritten again."""
    c = fc.solve_case("yaw_433")
    h = ql.Handle(0, **LIMITS)
    try:
        for cnb in (0.3, 0.15, 0.0, 0.3):
            r, o = _solve_both(h, qo, c, cote_noise_bound=cnb)
            print(cnb, "n_card", r["n_card"], o["n_card"], "final", len(r["final_inliers"]))
            assert len(o["clique"]) == 433
            _assert_same_record(r, o, cnb)
    finally:
        h.close()


def test_batch_group_of_finalize_edge_pairs_equals_single_calls_and_oracle(qo):
    """One lane group through the correspondence-only batched entry: COTE in scratch and in LDS, everything in scratch,
    mu = 1 / 0 and a clique of one, under one set of parameters."""
    names = ["yaw_433", "yaw_432", "yaw_3892", "mu_inf"]
    sets = [(fc.solve_case(n).src, fc.solve_case(n).tgt) for n in names]
    sets.append((sets[0][0][:1].copy(), sets[0][1][:1].copy()))
    kw = dict(noise_bound=fc.MU_INF_NOISE_BOUND)
    ora = [qo.solve(s, t, qo.default_params(**kw)) for (s, t) in sets]
    assert [len(o["clique"]) for o in ora] == [433, 432, 3892, 4, 0] and ora[3]["gnc_iters"] == 50
    prm = ql.demo_params(**kw)
    h1 = ql.Handle(0, **LIMITS)
    hb = ql.Handle(0, n_slots=24, **LIMITS)   # two lanes of 12: the five pairs share one lane group
    try:
        seq = [h1.solve(s, t, prm) for (s, t) in sets]
        got = hb.register_batch([(None, None, 0, s, t) for (s, t) in sets], params=prm)
    finally:
        h1.close()
        hb.close()
    for i, (g, r, o) in enumerate(zip(got, seq, ora)):
        assert g["status"] == r["status"] and g["valid"] == r["valid"] == o["valid"], i
        assert g["L"] == sets[i][0].shape[0]
        for k in ("clique", "final_inliers"):
            assert np.array_equal(g[k], r[k]) and np.array_equal(g[k], o[k]), (i, k)
        if o["valid"]:
            assert fc.same_bits(g["T"], r["T"]) and fc.same_bits(g["T"], o["T"]), i
            assert g["gnc_iters"] == r["gnc_iters"] == o["gnc_iters"], i
            assert list(g["n_card"]) == list(r["n_card"]) == list(o["n_card"]), i
            assert fc.same_bits(g["cost"], r["cost"]) and fc.same_bits(g["cost"], o["cost"]), i
            assert g["n_rot_inliers"] == r["n_rot_inliers"] == len(o["rot_inliers"]), i
    assert got[4]["status"] == ql.QTR_ERR_CLIQUE_TOO_SMALL


# ---------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("field,value", [("cote_noise_bound", -0.1), ("cote_noise_bound", float("nan")),
                                         ("cbar2", -1.0), ("cbar2", float("nan"))])
def test_parameters_the_reference_gives_no_meaning_are_rejected(hip, field, value):
    c = fc.solve_case("yaw_431")
    with pytest.raises(ql.QuatroHipError) as ei:
        hip.solve(c.src, c.tgt, ql.demo_params(**{field: value}))
    assert ei.value.code == ql.QTR_ERR_BAD_ARG
    assert field in str(ei.value)


def test_cote_noise_bound_at_the_ends_of_its_range(hip, qo):
    """0 stays accepted (the reference computes with it under IEEE rules; the only way into the in-kernel chain), and so
    do 1e-300 (every weight overflows) and 1e200 (every weight underflows)."""
    for v in (0.0, 1e-300, 1e200):
        c = fc.solve_case("yaw_431")
        r, o = _solve_both(hip, qo, c, cote_noise_bound=v)
        print(v, "n_card", r["n_card"], o["n_card"], "final", len(r["final_inliers"]), len(o["final_inliers"]))
        _assert_same_record(r, o, v)
