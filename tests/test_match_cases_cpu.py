"""The named pairs of tests/match_cases.py on the CPU: the oracle's matcher (lists and both nearest-neighbour tables)
against the binary32 numpy restatement of tests/match_restate.py, every pair against what it claims to be, the mirror of
nn_plan_single against the plan words written out by hand, the sequential mean against the restatement and against
numpy's own summation, and — where the reference's teaser::Matcher can be built — the reference itself on the pairs whose
outcome it defines (no NaN, no tie).  tests/test_gpu_match_cases.py then holds the device to the oracle on the same pairs.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402
import match_restate as mr  # noqa: E402

_tables = {}


def _restated(name, k):
    """the restatement of case `name` under its k-th setting; the nearest-neighbour tables are computed once per case"""
    c = mc.case(name)
    if name not in _tables:
        _tables[name] = mr.tables(c.desc_s, c.desc_t)
    return mr.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, tables_=_tables[name], **c.params[k])


def _oracle(qo, c, p):
    return qo.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, crosscheck=p["crosscheck"], tuple_test=p["tuple_test"],
                    tuple_scale=p["tuple_scale"], seed=p["seed"], debug=True)


@pytest.mark.parametrize("name", mc.ORDINARY_NAMES)
def test_oracle_equals_the_restatement(qo, name):
    c = mc.case(name)
    for k, p in enumerate(c.params):
        r = _restated(name, k)
        corr, nn_ij, nn_ji = _oracle(qo, c, p)
        assert np.array_equal(nn_ij, r["nn_large_of_small"]), (name, k)
        assert np.array_equal(nn_ji, r["nn_small_of_large"]), (name, k)
        assert np.array_equal(corr, r["corr"]), (name, k, corr.shape, r["corr"].shape)


def _large_small(c):
    swapped = c.desc_t.shape[0] > c.desc_s.shape[0]
    return (c.desc_t, c.desc_s, swapped) if swapped else (c.desc_s, c.desc_t, swapped)


def _outside_guard(d):
    d64 = d.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.any(~(np.abs(d64) <= 255.0)) or np.any(~(np.sum(d64 * d64, axis=1).astype(np.float32) < np.float32(65000.0))))


def _regime_holds(regime, unsafe, nq, gap, norm2_max):
    """What a claimed regime of the re-check count rests on.  zero: every query's winner is at least 1 ahead of the next
    row that is not a hidden repeat, while the f16 filter's bound u (76 |a|^2 + 108 |b|^2 + 40 (d1 + d2) + 800) 1.01 with
    u = 2^-24, |a|^2, |b|^2 <= norm2_max <= 15000 and d <= 4 norm2_max is below 0.35: certified.  some / many: a pair outside
    the guard lists every query; otherwise at least 1 / more than RC_SMALL_ROWS queries have a runner-up within 2^-20 of
    the winner, below the bound's constant term alone (800 u = 4.8e-5): never certified."""
    if regime is None:
        return True
    if regime == "zero":
        return (not unsafe) and norm2_max <= 15000 and bool(np.all(gap >= 1.0))
    listed = nq if unsafe else int((gap <= 2.0 ** -20).sum())
    return listed > (mc.RC_SMALL_ROWS if regime == "many" else 0)


@pytest.mark.parametrize("name", mc.ORDINARY_NAMES)
def test_every_claim_of_a_case_holds(name):
    c = mc.case(name)
    cl = dict(c.claims)
    large, small, swapped = _large_small(c)
    cc = [k for k, p in enumerate(c.params) if p["crosscheck"]][0]
    r = _restated(name, cc)
    assert (cl.pop("n_large"), cl.pop("n_small"), cl.pop("swapped")) == (large.shape[0], small.shape[0], swapped)
    assert c.xyz_s.shape == (c.desc_s.shape[0], 4) and c.xyz_t.shape == (c.desc_t.shape[0], 4)
    assert c.desc_s.dtype == c.desc_t.dtype == c.xyz_s.dtype == np.float32
    assert cl.pop("hidden_large") == int(mr.repeats(large).sum())
    assert cl.pop("hidden_small") == int(mr.repeats(small).sum())
    if "device_hidden_large" in cl:
        # the duplicate table by the mirror of its hash: a row is hidden when the LOWEST row with its slot and tag is
        # another row with the same 33 bit patterns
        hh = mc.desc_hash33(large)
        key = ((hh >> np.uint64(32)) << np.uint64(32)) | (hh & np.uint64(mc.dedup_slots(mc.HASH_CASE_MAX_VOXELS) - 1))
        _, first = np.unique(key, return_index=True)
        lowest = dict(zip(key[first].tolist(), first.tolist()))
        bits = large.view(np.uint32)
        hidden = [i for i in range(large.shape[0]) if lowest[int(key[i])] < i and np.array_equal(bits[lowest[int(key[i])]], bits[i])]
        assert cl.pop("device_hidden_large") == len(hidden) < int(mr.repeats(large).sum())
        assert key[40] == key[700] == key[1500] and not np.array_equal(bits[40], bits[700]) and np.array_equal(bits[700], bits[1500])
    unsafe = cl.pop("unsafe")
    assert unsafe == (_outside_guard(large) or _outside_guard(small))
    if "nhit" in cl:
        assert cl.pop("nhit") == r["nhit"]
    if "plan256" in cl:
        assert tuple(cl.pop("plan256")) == mc.plan_words(small.shape[0], large.shape[0], r["nhit"], 256)
    for j, i in cl.pop("nn_large_of_small", {}).items():
        assert r["nn_large_of_small"][j] == i, (j, i)
    for i, j in cl.pop("nn_small_of_large", {}).items():
        assert r["nn_small_of_large"][i] == j, (i, j)
    for i in cl.pop("nn_small_of_large_unasked", []):
        assert r["nn_small_of_large"][i] == -1, i
    for j, n in cl.pop("attain0", {}).items():
        assert r["ties0"][j] == n, (j, n, r["ties0"][j])
    pos = {int(i): k for k, i in enumerate(r["hit_rows"])}
    for i, n in cl.pop("attain1", {}).items():
        assert r["ties1"][pos[i]] == n, (i, n)
    if "listed0" in cl:
        assert cl.pop("listed0") == int((r["ties0"] == 2).sum())
    if "mutual_rows" in cl:
        assert list(cl.pop("mutual_rows")) == r["cross"][:, 0].tolist()
    if "mutual_per_block" in cl:
        nblk = (large.shape[0] + mc.CM_ROWS - 1) // mc.CM_ROWS
        assert list(cl.pop("mutual_per_block")) == np.bincount(r["cross"][:, 0] // mc.CM_ROWS, minlength=nblk).tolist()
    if "cross_has_00" in cl:
        assert cl.pop("cross_has_00") == bool(np.any((r["cross"][:, 0] == 0) & (r["cross"][:, 1] == 0)))
    for k, L in cl.pop("L", {}).items():
        assert _restated(name, k)["corr"].shape[0] == L, (k, L)
        if c.params[k]["tuple_test"] and L == 0:
            assert r["cross"].shape[0] > 0  # (the tuple test had something to reject)
    reg = cl.pop("recheck", (None, None))
    with np.errstate(invalid="ignore"):
        n2 = float(np.nanmax(np.r_[(large.astype(np.float64) ** 2).sum(1), (small.astype(np.float64) ** 2).sum(1)]))
    assert _regime_holds(reg[0], unsafe, small.shape[0], r["gap0"], n2), reg
    assert _regime_holds(reg[1], unsafe, r["nhit"], r["gap1"], n2), reg
    assert not cl, f"claims nobody checks: {sorted(cl)}"


def test_the_case_groups_cover_what_they_are_named_for():
    """the plan edges: queries on both sides of 512 against bases on both sides of 512, 1024 and 2048, both directions;
    1 / 512 / 513 hit rows; bases of 1, 31, 32, 33; 64 / 65 queries.  The tail: both swap states next to each other,
    every setting, a seed above 2^32.  The plan words written by hand equal the mirror, and the mirror's edges are where
    the issue says (one tile per slice up to 1024 base rows, two up to 2048, then three with a short last slice)."""
    shapes = set(mc.PLAN_SHAPES)
    d0 = {(s, l) for s, l, h in shapes}
    d1 = {(h, s) for s, l, h in shapes}
    for q in (512, 513):
        for b in (512, 513, 1024, 1025, 2048, 2049):
            if q <= b:
                assert (q, b) in d0, (q, b)
                assert (q, b) in d1, (q, b)
    assert {1, 512, 513} <= {h for _, _, h in shapes}
    assert {1, 31, 32, 33} <= {l for _, l, _ in shapes} and {1, 31, 32, 33} <= {s for s, _, _ in shapes}
    assert {64, 65} <= {s for s, _, _ in shapes} and {64, 65} <= {h for _, _, h in shapes}
    for pad, (sp, tps) in mc.PLAN_256.items():
        for qb in (1, 2, 3, 5):
            assert mc.nn_plan_single(qb, pad // 32, 256) == sp | (tps << 8), (pad, qb)
    assert mc.nn_plan_single(1, mc.padded(1) // 32, 256) == 16 | (1 << 8)         # 16 tiles, 15 of them pad-only
    assert mc.nn_plan_single(1, mc.padded(2049) // 32, 256) & 0xff == 27            # 80 tiles = 26 * 3 + 2
    assert mc.nn_plan_single(300, 80, 256) == 2 | (40 << 8)                         # more blocks than workgroups: T = 64
    sw = {mc.case(n).claims["swapped"] for n in mc.TAIL_NAMES}
    assert sw == {True, False}
    assert (mc.case("tail_l1024_middle_empty").desc_s.shape[0], mc.case("tail_l1024_middle_empty").desc_t.shape[0]) == (1024, 1024)
    assert (mc.case("tail_l1025_swap_all").desc_s.shape[0], mc.case("tail_l1025_swap_all").desc_t.shape[0]) == (1024, 1025)
    for n in mc.TAIL_NAMES:
        ps = mc.case(n).params
        assert {(p["crosscheck"], p["tuple_test"]) for p in ps} == {(True, True), (True, False), (False, True), (False, False)}
        assert {p["seed"] for p in ps if p["tuple_test"]} >= {0, mc.BIG_SEED} and mc.BIG_SEED > 2 ** 32
    assert {mc.case(n).claims["n_large"] for n in mc.TAIL_NAMES} >= {512, 513, 1024, 1025, 1537}
    # a good share of the mutual pairs passes the tuple test where the geometry is consistent for every second row
    r = _restated("tail_l1537_gap", 0)
    assert 0.2 * r["cross"].shape[0] < r["corr"].shape[0] < r["cross"].shape[0]


@pytest.mark.parametrize("n", mc.MEAN_SIZES)
def test_sequential_mean_is_the_restatement_and_not_a_pairwise_sum(qo, n):
    """The oracle's mean is observable through the tuple test only; its voxel order is what a keyframe stores, so the
    clouds are checked in that order: one voxel per point, the sequential binary32 sum differs from numpy's blocked
    pairwise sum in at least one coordinate (n = 1: nothing to differ), and the restatement equals a plain Python loop."""
    cloud = mc.mean_cloud(n)
    vox = qo.voxelize(cloud, mc.MEAN_LEAF)
    assert vox.shape[0] == n
    assert np.array_equal(np.sort(vox[:, 0]), np.sort(cloud[:, 0]))  # (a voxel of one point is that point)
    m = mr.seq_mean(vox)
    acc = np.zeros(3, dtype=np.float32)
    for p in vox[:, :3]:
        acc = acc + p
    assert np.array_equal(m, acc / np.float32(n))
    # (numpy sums a contiguous vector in blocks of eight interleaved partial sums, pairwise above 128 elements)
    other = np.array([np.sum(np.ascontiguousarray(vox[:, k]), dtype=np.float32) for k in range(3)]) / np.float32(n)
    assert np.array_equal(m, other) == (n == 1), (n, m, other)


@pytest.mark.parametrize("name", mc.SWITCH_NAMES[:1])
def test_the_tail_switch_pair_is_what_it_claims(name):
    """(the oracle alone judges these pairs: the restatement is exempt from their size)"""
    c = mc.case(name)
    n = mc.TAIL_MAXWG * 512
    assert (c.claims["n_large"], c.claims["n_small"], c.claims["swapped"]) == (n, mc.SWITCH_SMALL, False)
    assert c.desc_s.shape == (n, 33) and not c.claims["unsafe"] and c.claims["hidden_large"] == 0
    assert [mc.case(s).claims["n_large"] for s in mc.SWITCH_NAMES] == [n, n, n + 1, n + 1]


def _ref_defined(name):
    """no NaN anywhere and no query of either direction with two rows at its minimum"""
    c = mc.case(name)
    r = _restated(name, 0)
    return not (np.isnan(c.desc_s).any() or np.isnan(c.desc_t).any()) and r["ties0"].max() <= 1 and r["ties1"].max() <= 1


def test_reference_matcher_on_the_cases_it_defines(qo, capfd):
    """(ties go to whichever row the reference's search meets first, and a NaN has no defined outcome there: those cases
    are left to the oracle's written rules)"""
    if not qo.ref_buildable():
        pytest.skip("the reference's sources are not here")
    assert qo.build_ref() is not None
    ran = []
    for name in mc.ORDINARY_NAMES:
        if not _ref_defined(name):
            continue
        c = mc.case(name)
        for p in c.params:
            kw = dict(crosscheck=p["crosscheck"], tuple_test=p["tuple_test"], tuple_scale=p["tuple_scale"], seed=p["seed"])
            got = qo.ref_match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, **kw)
            assert np.array_equal(got, qo.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, **kw)), (name, p)
        ran.append(name)
    capfd.readouterr()  # (the reference prints its progress lines)
    print("reference matcher ran on", len(ran), "of", len(mc.ORDINARY_NAMES), "cases")
    assert len(ran) >= 20 and any(n.startswith("tail_") for n in ran) and "recheck_cluster" in ran
