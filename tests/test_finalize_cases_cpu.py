"""No-GPU checks of tests/finalize_cases.py, the inputs of tests/test_gpu_finalize_edges.py:

  * the oracle deserves to be the yardstick: on every case a restatement can judge, the oracle's GNC and COTE equal the
    second restatements of tests/backend_restate.py (numpy SVD, plain Python floats) with the margins
    tests/test_oracle_cpu.py uses; finite COTE cases also go through the compiled reference's estimate() where
    oracle/_ref is built; the cases on the fixed not-restated lists are held to hand-stated facts instead;
  * the cases stay what they claim: mu = 1 / 0 runs to max_it with an empty mask, the solve-level recipes give exactly
    the clique size and the side of every layout switch they are named after;
  * the switch values are derived from the kernel's own constant: FIN_LDS_BYTES here equals the #define in solver.hip.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import finalize_cases as fc  # noqa: E402
from backend_restate import ref_cote_python, ref_gnc_rotation2d_numpy, ref_gnc_rotation3d_numpy  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _oracle_gnc(qo, c, dim, **over):
    a = c._replace(**over)
    fn = qo.gnc_rotation2d if dim == 2 else qo.gnc_rotation3d
    with np.errstate(all="ignore"):
        return fn(a.X, a.Y, a.noise_bound, a.gnc_factor, a.max_it, a.cost_thr)


def _restated_gnc(c, dim, **over):
    a = c._replace(**over)
    fn = ref_gnc_rotation2d_numpy if dim == 2 else ref_gnc_rotation3d_numpy
    with np.errstate(all="ignore"):
        return fn(a.X, a.Y, a.noise_bound, a.gnc_factor, a.max_it, a.cost_thr)


# ---------------------------------------------------------------------------------------------- constants
def test_layout_switches_follow_the_kernels_constant():
    src = open(os.path.join(ROOT, "quatro_amd", "csrc", "solver.hip")).read()
    m = re.search(r"^#define FIN_LDS_BYTES \((\d+) \* (\d+)\)$", src, flags=re.M)
    assert m, "the #define FIN_LDS_BYTES line of solver.hip changed its form"
    assert int(m.group(1)) * int(m.group(2)) == fc.FIN_LDS_BYTES
    # the byte formulas of k_finalize, on both sides of each switch
    assert (fc.M_LDS_YAW, fc.M_LDS_3DOF, fc.M_LDS_CHAIN, fc.N_LDS_COTE) == (3891, 2779, 2432, 432)
    for per, last in ((40, fc.M_LDS_YAW), (56, fc.M_LDS_3DOF), (64, fc.M_LDS_CHAIN)):
        assert per * last <= fc.FIN_LDS_BYTES < per * (last + 1)
    assert fc.cote_lds_bytes(fc.N_LDS_COTE) <= fc.FIN_LDS_BYTES < fc.cote_lds_bytes(fc.N_LDS_COTE + 1)
    # every row of the table is straddled by solve-level cases
    for last, names in ((fc.M_LDS_YAW, "yaw_%d"), (fc.M_LDS_3DOF, "3dof_%d"), (fc.M_LDS_CHAIN, "cnb_0_%d"),
                        (fc.N_LDS_COTE, "yaw_%d"), (fc.N_LDS_COTE, "3dof_%d")):
        assert names % last in fc.SOLVE_NAMES and names % (last + 1) in fc.SOLVE_NAMES


def test_generators_are_deterministic_and_read_only():
    a = fc.gnc_case("planted_65", 3)
    assert fc.same_bits(a.X, fc._gnc("planted_65", 3).X) and not a.X.flags.writeable
    c = fc.cote_case("ladder_ranges_17")
    assert fc.same_bits(c.ranges, fc._cote("ladder_ranges_17").ranges) and not c.X.flags.writeable
    s = fc.solve_case("yaw_431")
    assert np.array_equal(s.src, fc._solve("yaw_431").src) and s.src.dtype == np.float32 and not s.src.flags.writeable
    assert len(set(fc.GNC_CASES)) == len(fc.GNC_CASES) and len(set(fc.COTE_NAMES)) == len(fc.COTE_NAMES)
    assert set(fc.GNC_NOT_RESTATED) <= set(fc.GNC_NAMES) and set(fc.GNC_NONUNIQUE) <= set(fc.GNC_NAMES)
    assert set(fc.COTE_NOT_RESTATED) <= set(fc.COTE_NAMES)
    for name, dim in fc.GNC_CASES:  # a case is on the not-restated list exactly when something in it is not finite
        c = fc.gnc_case(name, dim)
        with np.errstate(over="ignore"):
            finite = np.isfinite(c.X).all() and np.isfinite(c.Y).all() and np.isfinite(c.X.T @ c.Y).all()
        assert finite == (name not in fc.GNC_NOT_RESTATED or name == "mu_inf"), name
    for name in fc.COTE_NAMES:
        c = fc.cote_case(name)
        assert np.isfinite(c.X).all() == (name not in fc.COTE_NOT_RESTATED or name == "zero_range"), name


# ---------------------------------------------------------------------------------------------- GNC
def _proper(R):
    d = R.shape[0]
    return abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(d)).max() < 1e-12


@pytest.mark.parametrize("name,dim", [c for c in fc.GNC_CASES if c[0] not in fc.GNC_NOT_RESTATED])
def test_oracle_gnc_equals_the_svd_restatement(qo, name, dim):
    c = fc.gnc_case(name, dim)
    assert c.X.shape == c.Y.shape and c.X.shape[1] == dim
    R, cost, iters, mask = _oracle_gnc(qo, c, dim)
    assert _proper(R)
    if name in fc.GNC_NONUNIQUE:
        # the optimum of a round is not unique: the same objective on the first round's H (unit weights), a proper
        # rotation, as test_rot3_matches_svd_construction has it — and the loop's bookkeeping where the residuals are
        # exact (zero, half_turn, collinear, tiny: round 0 ends the loop on mu < 0)
        R1 = _oracle_gnc(qo, c, dim, max_it=1)[0]
        Rr = _restated_gnc(c, dim, max_it=1)[0]
        H = c.X.T @ c.Y
        assert _proper(R1)
        assert np.trace(R1 @ H) >= np.trace(Rr @ H) - 1e-9 * max(1.0, abs(np.trace(Rr @ H)))
        if name in ("zero", "half_turn", "collinear", "tiny"):
            assert iters == 1 and np.isinf(cost) and mask.all()
        return
    Rr, costr, itr, maskr = _restated_gnc(c, dim)
    assert iters == itr and np.array_equal(mask, maskr)
    assert np.abs(R - Rr).max() < 1e-9
    assert (np.isinf(cost) and np.isinf(costr)) or abs(cost - costr) <= 1e-9 * max(1.0, abs(costr))
    # what the names promise
    if name == "all_exact":
        assert iters == 1 and np.isinf(cost) and mask.all()
    if name == "all_outliers":
        assert not mask.any() and cost == 0.0 and 2 < iters < c.max_it  # every weight reached 0; two rounds of cost 0
    if name == "never_converges":
        assert iters == c.max_it == 7
    if name == "one_round":
        assert iters == 2  # |cost - inf| = inf is not < inf: the second round's difference is the first finite one
    if name == "tiny_bound":
        assert c.noise_bound ** 2 < 1e-16 and iters > 1
    if name.startswith("planted_") and c.X.shape[0] >= 63:
        assert 1 < iters < c.max_it and 0.5 < mask.mean() < 0.9


@pytest.mark.parametrize("name,dim", [c for c in fc.GNC_CASES if c[0] in fc.GNC_NOT_RESTATED])
def test_oracle_gnc_on_what_no_restatement_judges(qo, name, dim):
    c = fc.gnc_case(name, dim)
    R, cost, iters, mask = _oracle_gnc(qo, c, dim)
    if name == "mu_inf":
        # R = I and r^2 = 2 a^2 exactly in round 0, so mu = 1 / 0: NaN thresholds, NaN weights, max_it rounds, nobody in
        with np.errstate(all="ignore"):
            R1, cost1, it1, _ = _oracle_gnc(qo, c, dim, max_it=1)
        assert np.array_equal(R1, np.eye(dim)) and cost1 == 4 * 2 * 0.25 ** 2 and it1 == 1
        assert 2 * (2 * 0.25 ** 2) / c.noise_bound ** 2 - 1 == 0.0
        assert iters == c.max_it and not mask.any() and np.isnan(cost)
        assert np.array_equal(R, np.eye(2)) if dim == 2 else np.isnan(R).all()
    elif name == "huge":
        # H overflows; the residuals overflow: max_r = inf, mu = 0, out in round 0 with the unit weights
        assert iters == 1 and np.isinf(cost) and mask.all()
        if dim == 2:
            assert np.array_equal(R, np.eye(2))  # inf - inf in the closed form: no direction, the identity
    else:
        # the member poisons H (w x y is NaN or inf - inf).  Where the rotation still has finite entries — the yaw's closed
        # form takes no direction from a NaN H: the identity — the member's own residual is NaN, so is its weight, and it
        # is never an inlier; where the rotation is NaN every residual is, max_r stays -inf, mu = 1 / (-inf) = -0 <= 0 and
        # the loop leaves in round 0 with the unit weights
        if name == "nan_member" and dim == 2:
            assert np.array_equal(R, np.eye(2)) and not mask[37] and iters > 1
        else:
            assert (np.isnan(R).any() and iters == 1 and mask.all() and np.isinf(cost)) or not mask[37]


# ---------------------------------------------------------------------------------------------- COTE
def _oracle_cote(qo, c, median):
    with np.errstate(all="ignore"):
        if np.isscalar(c.ranges):
            return qo.cote_estimate(c.X, c.ranges, median)
        return qo.cote_estimate_ranges(c.X, c.ranges, median)


@pytest.mark.parametrize("name", [n for n in fc.COTE_NAMES if n not in fc.COTE_NOT_RESTATED])
def test_oracle_cote_equals_the_python_restatement_and_the_compiled_reference(qo, name):
    c = fc.cote_case(name)
    for median in (True, False):
        e, inl, card = _oracle_cote(qo, c, median)
        e_ref, card_ref, inl_ref = ref_cote_python([float(v) for v in c.X], c.ranges, median)
        assert card == card_ref, (name, median)
        assert fc.same_bits(e, e_ref), (name, median, e, e_ref)
        assert inl.tolist() == inl_ref, (name, median)
        if qo.ref_solver_available() and name not in fc.COTE_TIED_KEYS and c.X.size >= 2 and not (median and card < 2):
            # (equal keys: the reference's sort order is unspecified, D3; one measurement: the reference asserts; a consensus
            # set of one: it reads past its candidate list, D4)
            er, mr = qo.ref_cote_estimate(c.X, c.ranges, median)
            assert fc.same_bits(e, er) and np.array_equal(inl, mr), (name, median, e, er)
    # what the names promise
    e, inl, card = _oracle_cote(qo, c, True)
    keys = np.concatenate([c.X - c.ranges, c.X + c.ranges])
    assert (np.unique(keys).size < keys.size) == (name in fc.COTE_TIED_KEYS)
    if name.startswith("same_key"):
        k0 = 150 if name == "same_key_embedded" else 0
        blk = c.X[k0:k0 + 40]
        assert np.all(np.diff(blk) < 0) and np.unique(blk - 4.0).size <= 21 and np.unique(blk + 4.0).size <= 11
        assert card >= 40 and inl[k0:k0 + 40].all()
    if name in ("disjoint", "n1", "huge", "cost0_nan"):
        assert card == 1
    if name == "cost0_nan":
        assert e == c.X[0]  # NaN first: Eigen's minCoeff never leaves it, whatever finite costs follow
    if name == "all_equal":
        assert card == c.X.size and e == 0.7 and inl.all()
    if name == "nested_ranges":
        assert inl[17] and card > 2
    if name == "range_ties":
        lo, hi = c.X - c.ranges, c.X + c.ranges
        assert np.intersect1d(lo, hi).size > 5


def _without(c, k):
    keep = np.arange(c.X.size) != k
    return fc.CoteCase(c.X[keep], c.ranges if np.isscalar(c.ranges) else c.ranges[keep]), keep


@pytest.mark.parametrize("name", fc.COTE_NOT_RESTATED)
def test_oracle_cote_on_what_no_restatement_judges(qo, name):
    c = fc.cote_case(name)
    for median in (True, False):
        e, inl, card = _oracle_cote(qo, c, median)
        if name == "zero_range":
            # every weight is 1 / 0: the first event's estimate is inf / inf, NaN first, Eigen's minCoeff stays there
            assert card == 1 and not inl.any() if not median else card == 1
            assert (e == c.X.min() and inl.sum() == 1) if median else np.isnan(e)
        elif name in ("nan_mid", "nan_first"):
            k = int(np.nonzero(np.isnan(c.X))[0][0])
            assert k == (0 if name == "nan_first" else 41)
            c2, keep = _without(c, k)
            e2, inl2, card2 = _oracle_cote(qo, c2, median)
            assert not inl[k]  # its endpoints sort last: never in the consensus set, never an inlier
            assert e == e2 and card == card2 and np.array_equal(inl[keep], inl2) and card2 > 40
        elif name == "inf_both":
            # -inf opens first: its cost is inf - inf, NaN first
            assert card == 1 and e == -np.inf and not inl.any()
        elif name == "all_nan":
            assert card == 1 and np.isnan(e) and not inl.any()


# ---------------------------------------------------------------------------------------------- solve-level recipes
@pytest.fixture(scope="module")
def qo8(qo):
    qo.set_threads(min(8, qo.max_threads()))
    return qo


@pytest.mark.parametrize("name", fc.SOLVE_NAMES)
def test_solve_level_recipe_gives_the_clique_and_the_layout_it_claims(qo8, name):
    c = fc.solve_case(name)
    with np.errstate(all="ignore"):
        o = qo8.solve(c.src, c.tgt, qo8.default_params(**c.kw))
    assert o["valid"] and o["status"] == 0
    assert len(o["clique"]) == c.M, (len(o["clique"]), c.M)
    L = c.src.shape[0]
    assert L <= 4100
    nrot = len(o["rot_inliers"])
    use_rot = bool(c.kw.get("using_rot_inliers_when_estimating_cote")) and nrot > 0
    N = nrot if use_rot else c.M
    if c.side is not None:
        assert fc._side(N) == c.side, (N, c.side)
    if name in fc.SOLVE_ITERATES:
        assert o["gnc_iters"] > 1 and 0 < nrot < c.M  # weights in all three bands: a strict subset
        if not name.startswith("cnb_"):
            assert len(set(o["n_card"])) == 3 or c.kw.get("reg_mode") == 1
    if name.startswith("var_") and name.endswith("rotinl"):
        assert N == nrot and fc._side(N) == ("lds" if c.M == 433 else "global")
    if name == "rotinl_lds":
        assert nrot == fc.N_LDS_COTE
    if name == "rotinl_global":
        assert fc.N_LDS_COTE < nrot <= fc.N_LDS_COTE + 8
    if name.startswith("mu_inf"):
        assert o["gnc_iters"] == 50 and nrot == 0 and N == c.M == 4 and np.isnan(o["cost"])
        assert len(o["final_inliers"]) == 4 and np.array_equal(o["T"][:3, :3], np.eye(3))
    if name == "all_exact_433":
        assert o["gnc_iters"] == 1 and np.isinf(o["cost"]) and nrot == 433 and len(o["final_inliers"]) == 433
    if name.startswith("cnb_0_") or name == "cnb_1e-300_300":
        assert o["n_card"] == [1, 1, 1]
    if name == "cnb_1e200_300":
        assert len(o["final_inliers"]) == c.M
