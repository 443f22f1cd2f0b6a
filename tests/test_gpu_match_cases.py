"""The matcher's kernels (k_half_tables, k_nn_f16, k_nn_finish_f16, k_recheck_filter, k_hit_compact, the fused tail
k_cross_multi / k_tuple / k_pairs_multi, the six-launch tail above TAIL_MAXWG * 512 rows, the lists without the
cross-check) and the matcher mean on the named pairs of tests/match_cases.py, through Handle.match, keyframes and
debug_fetch of the product library, against the CPU oracle: np.array_equal on the correspondences and on both
nearest-neighbour tables, no tolerance anywhere.  tests/test_match_cases_cpu.py holds the oracle to an independent
restatement on the same pairs and asserts that every pair is what it claims to be.

From the counters of DBG_MATCH_STATS: the hit count, the hidden duplicates of either cloud and the out-of-guard flag equal
the case's claims, the two plan words equal the mirror of nn_plan_single evaluated with the device's compute-unit count,
the tail reported no look-back failure, and the re-check counts lie in the regime the case is built for — their VALUE
depends on the filter's rounding bound and is printed, not asserted.

Every case runs twice on one handle with a pair of another shape in between (stale plan words, look-back words, partial
records and hit lists would show), the tail cases once more on a second stream slot.
"""
import os
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402
import match_restate as mr  # noqa: E402

pytestmark = pytest.mark.gpu
# (max_voxels: the duplicate table of 16384 slots that the hash_collision case is built for)
LIMITS = dict(max_points=8192, max_voxels=mc.HASH_CASE_MAX_VOXELS, max_corr=4096)
from match_cases import (MC_HIDDEN_I, MC_HIDDEN_J, MC_NCORR, MC_NCROSS, MC_NHIT, MC_NQ0, MC_NSPLIT0, MC_NSPLIT1,  # noqa: E402
                         MC_RECHECK0, MC_RECHECK1, MC_SWAPPED, MC_TAILERR, MC_UNSAFE)
BETWEEN = ("plan_s65_l700_h64", "plan_s513_l1025_h513")  # the pair of another shape that runs between the two visits
_want = {}


@pytest.fixture(scope="module")
def h():
    hd = ql.Handle(0, n_slots=2, **LIMITS)
    yield hd
    hd.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _fp(p):
    return ql.default_frontend_params(use_crosscheck=int(p["crosscheck"]), use_tuple_test=int(p["tuple_test"]),
                                      tuple_scale=p["tuple_scale"], seed=p["seed"])


def _oracle(qo, name, k):
    """(correspondences, NN of the smaller cloud's rows, NN of the larger cloud's rows) of case `name` under its k-th
    setting, computed once"""
    if (name, k) not in _want:
        c = mc.case(name)
        p = c.params[k]
        _want[(name, k)] = qo.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, crosscheck=p["crosscheck"], tuple_test=p["tuple_test"],
                                    tuple_scale=p["tuple_scale"], seed=p["seed"], debug=True)
    return _want[(name, k)]


def _in_regime(regime, count):
    return {None: True, "zero": count == 0, "some": count > 0, "many": count > mc.RC_SMALL_ROWS}[regime]


def _run(hd, qo, n_cu, name, slot=0, visit=""):
    c = mc.case(name)
    cl = c.claims
    for k, p in enumerate(c.params):
        tag = (name, k, visit)
        corr_o, nn_ls_o, nn_sl_o = _oracle(qo, name, k)
        corr = hd.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, _fp(p), slot=slot)
        nn_ls = hd.debug_fetch(ql.DBG_NN_LARGE_OF_SMALL, np.int32, slot=slot)
        nn_sl = hd.debug_fetch(ql.DBG_NN_SMALL_OF_LARGE, np.int32, slot=slot)
        st = hd.debug_fetch(ql.DBG_MATCH_STATS, np.int32, slot=slot)
        nhit = int((nn_sl_o >= 0).sum())
        print(f"{name}[{k}]{visit}: L {corr.shape[0]} hit {st[MC_NHIT]} cross {st[MC_NCROSS]} hidden {st[MC_HIDDEN_I]}/{st[MC_HIDDEN_J]} "
              f"unsafe {st[MC_UNSAFE]} recheck {st[MC_RECHECK0]}/{st[MC_RECHECK1]} plan {st[MC_NSPLIT0]:#x}/{st[MC_NSPLIT1]:#x}")
        assert np.array_equal(nn_ls, nn_ls_o), tag
        assert np.array_equal(nn_sl, nn_sl_o), tag
        assert np.array_equal(corr, corr_o), tag
        assert st[MC_TAILERR] == 0 and st[MC_NCORR] == corr_o.shape[0] and st[MC_SWAPPED] == int(cl["swapped"]), (tag, st)
        assert st[MC_NHIT] == nhit == cl.get("nhit", nhit) and st[MC_NQ0] == cl["n_small"], (tag, st)
        assert (st[MC_HIDDEN_I], st[MC_HIDDEN_J]) == (cl.get("device_hidden_large", cl["hidden_large"]), cl["hidden_small"]), (tag, st)
        assert bool(st[MC_UNSAFE]) == cl["unsafe"], (tag, st)
        assert (st[MC_NSPLIT0], st[MC_NSPLIT1]) == mc.plan_words(cl["n_small"], cl["n_large"], nhit, n_cu), (tag, st, n_cu)
        if n_cu == 256 and "plan256" in cl:
            assert (st[MC_NSPLIT0], st[MC_NSPLIT1]) == tuple(cl["plan256"]), (tag, st)
        reg = cl.get("recheck", (None, None))
        assert _in_regime(reg[0], st[MC_RECHECK0]) and _in_regime(reg[1], st[MC_RECHECK1]), (tag, reg, st)
        if p["crosscheck"]:
            if "mutual_rows" in cl:
                assert st[MC_NCROSS] == len(cl["mutual_rows"]), (tag, st)
            if cl.get("L", {}).get(k) == 0:
                assert st[MC_NCROSS] > 0 and corr.shape[0] == 0, (tag, st)


@pytest.mark.parametrize("name", mc.ORDINARY_NAMES)
def test_case_equals_the_oracle_twice_with_another_shape_in_between(h, qo, n_cu, name):
    between = BETWEEN[1] if name == BETWEEN[0] else BETWEEN[0]
    _run(h, qo, n_cu, name)
    _run(h, qo, n_cu, between, visit=" (between)")
    _run(h, qo, n_cu, name, visit=" (again)")


@pytest.mark.parametrize("name", mc.TAIL_NAMES)
def test_tail_case_on_the_second_stream_slot(h, qo, n_cu, name):
    _run(h, qo, n_cu, name, slot=1, visit=" (slot 1)")


def test_tail_switch_at_131072_and_131073_rows(qo, n_cu):
    """TAIL_MAXWG * 512 rows: the fused tail with all 256 look-back words in use; one row more: k_cross_flags2,
    k_scan_flags, k_cross_compact, k_scatter_pairs, k_scan_nonneg, k_corr_compact2.  The larger cloud as the source and as
    the target, the tuple test on and off; a handle with room for one row more than the switch and a small max_corr."""
    n = mc.TAIL_MAXWG * 512 + 1
    hd = ql.Handle(0, max_points=n + 7, max_voxels=n + 7, max_corr=1024)
    try:
        for name in mc.SWITCH_NAMES:
            c = mc.case(name)
            for k, p in enumerate(c.params):
                corr_o, nn_ls_o, nn_sl_o = qo.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, crosscheck=p["crosscheck"],
                                                    tuple_test=p["tuple_test"], tuple_scale=p["tuple_scale"], seed=p["seed"], debug=True)
                corr = hd.match(c.xyz_s, c.desc_s, c.xyz_t, c.desc_t, _fp(p))
                st = hd.debug_fetch(ql.DBG_MATCH_STATS, np.int32)
                print(f"{name}[{k}]: L {corr.shape[0]} hit {st[MC_NHIT]} cross {st[MC_NCROSS]} recheck {st[MC_RECHECK0]}/{st[MC_RECHECK1]}")
                assert np.array_equal(hd.debug_fetch(ql.DBG_NN_LARGE_OF_SMALL, np.int32), nn_ls_o), (name, k)
                assert np.array_equal(hd.debug_fetch(ql.DBG_NN_SMALL_OF_LARGE, np.int32), nn_sl_o), (name, k)
                assert np.array_equal(corr, corr_o), (name, k)
                nhit = int((nn_sl_o >= 0).sum())
                assert st[MC_TAILERR] == 0 and st[MC_NHIT] == nhit and st[MC_SWAPPED] == int(c.claims["swapped"]), (name, k, st)
                assert (st[MC_HIDDEN_I], st[MC_HIDDEN_J], st[MC_UNSAFE]) == (0, 0, 0), (name, k, st)
                assert (st[MC_NSPLIT0], st[MC_NSPLIT1]) == mc.plan_words(c.claims["n_small"], c.claims["n_large"], nhit, n_cu)
                assert nn_ls_o[0] == 0 and nn_ls_o[-1] == c.claims["n_large"] - 1  # (pairs in the first and the last workgroup)
                assert 100 < corr_o.shape[0] <= mc.SWITCH_SMALL
    finally:
        hd.close()


@pytest.mark.parametrize("n", mc.MEAN_SIZES)
def test_keyframe_mean_is_the_sequential_sum_bit_for_bit(h, qo, n):
    """d_seq_mean on both sides of its unroll (31 / 32 / 33) and of its staged chunk (2047 / 2048 / 2049, 4097: three
    chunks), on coordinates whose sum depends on the order of the additions"""
    cloud = mc.mean_cloud(n)
    vox = qo.voxelize(cloud, mc.MEAN_LEAF)
    assert vox.shape[0] == n
    with h.keyframe(cloud, ql.default_frontend_params(voxel_size=mc.MEAN_LEAF)) as kf:
        assert kf.info["n_voxels"] == n and kf.info["passed_through"] == 0
        assert np.array_equal(kf.fetch(ql.KF_VOX).view(np.uint32), vox.view(np.uint32))
        got = kf.fetch(ql.KF_MEAN)
    want = mr.seq_mean(vox)
    assert np.array_equal(got[:3].view(np.uint32), want.view(np.uint32)), (n, got, want)


def _outcome(call):
    try:
        return call()
    except ql.QuatroHipError as e:
        return {"status": e.code, "valid": False, "L": None}


def test_grouped_keyframes_at_the_plan_and_tail_edges_equal_the_single_calls(qo):
    """Keyframes of 1, 512, 513 and 1025 voxels through register_batch_keyframes in ONE group of mixed sizes against
    register_keyframes pair by pair: the same status, L, T, clique and inliers; and L is the oracle's on what the keyframes
    store."""
    fp = ql.default_frontend_params(voxel_size=mc.GROUP_LEAF)
    hb = ql.Handle(0, n_slots=8, max_points=8192, max_voxels=2048, max_corr=2048)
    try:
        src = {n: hb.keyframe(mc.group_cloud(n, 0), fp) for n in mc.GROUP_VOXELS}
        tgt = {n: hb.keyframe(mc.group_cloud(n, 1), fp, slot=1) for n in mc.GROUP_VOXELS}
        for kfs in (src, tgt):
            for n, kf in kfs.items():
                assert kf.info["n_voxels"] == n, (n, kf.info)
        shapes = [(1, 512), (512, 513), (513, 513), (1025, 513), (513, 1025), (1025, 1025), (512, 1), (1, 1)]
        pairs = [(src[a], tgt[b], 40 + i) for i, (a, b) in enumerate(shapes)]
        singles = []
        for ks, kt, seed in pairs:
            f1 = ql.default_frontend_params(voxel_size=mc.GROUP_LEAF, seed=seed)
            singles.append(_outcome(lambda: hb.register_keyframes(ks, kt, f1)))
        group = hb.register_batch_keyframes(pairs, fp)
        for (a, b), (ks, kt, seed), one, g in zip(shapes, pairs, singles, group):
            want_L = qo.match(ks.fetch(ql.KF_VOX), ks.fetch(ql.KF_FPFH), kt.fetch(ql.KF_VOX), kt.fetch(ql.KF_FPFH), seed=seed).shape[0]
            print(f"{a} x {b}: status {one['status']} / {g['status']} L {one['L']} / {g['L']} oracle {want_L}")
            assert g["status"] == one["status"], (a, b)
            assert g["L"] == want_L and one["L"] in (want_L, None), (a, b)
            if one["L"] is None:
                continue
            assert g["valid"] == one["valid"], (a, b)
            if "clique" in one:
                assert np.array_equal(g["clique"], one["clique"]) and np.array_equal(g["final_inliers"], one["final_inliers"]), (a, b)
            if one["valid"]:
                assert np.array_equal(g["T"], one["T"]), (a, b)
    finally:
        hb.close()
