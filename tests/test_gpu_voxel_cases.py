"""The voxel grid's kernels (k2_minmax, k2_keys_hist, k2_radix_scatter, k2_vox_centroids) on the named clouds of
tests/voxel_cases.py — runs placed at every edge of the centroid kernel's window for both tile sizes, key widths on both
sides of every radix pass, 33 radix tiles, the int32 edge of the index arithmetic — against the CPU oracle, bit for bit.
tests/test_voxel_cases_cpu.py holds the oracle to an independent restatement on the same clouds, asserts that every cloud
is where it claims to be, and that each can tell the wrong variant it was built for from the right one.

Every route that runs the voxel stage, through the C ABI alone:

  * qtr_voxelize: every case (four passes launched, the adaptive ones return at once; 256-point tiles);
  * qtr_voxelize again and again on one slot, across pass counts, tile counts and a pass-through: what a call leaves in
    the rotating histogram buffers, the two key buffers and the look-back words is the next call's starting state;
  * qtr_keyframe_create: the one-cloud chain, which launches as many passes as the slot's previous calls needed and runs
    again when that was too few;
  * qtr_feature_pair: two clouds in one launch, the grid sized by the larger one (QTR_DBG_VOX_SRC / _TGT);
  * qtr_submit_batch: the grouped launch with 1024-point tiles; a lane's slot keeps its pair's voxels;
  * the capacity refusals of qtr_voxelize, with the exact count, and the call after one.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=65536, max_voxels=32768, max_corr=8192)
_want = {}


def _b(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle(qo, name):
    """what every route must reproduce, computed once"""
    if name not in _want:
        cloud, leaf, _ = vc.case(name)
        _want[name] = qo.voxelize(cloud, leaf)
        _want[name].setflags(write=False)
    return _want[name]


def _equal(got, want, what):
    got = np.asarray(got, dtype=np.float32).reshape(-1, 4)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.nonzero(np.any(_b(got) != _b(want), axis=1))[0]
    assert diff.size == 0, (what, "first differing voxel", int(diff[0]), got[diff[0]], want[diff[0]], "of", diff.size)


@pytest.fixture(scope="module")
def h():
    hd = ql.Handle(0, **LIMITS)
    yield hd
    hd.close()


def _fp(name):
    """the case's leaf, and radii that keep the neighbour lists behind the grid short: a few voxels each"""
    leaf = vc.case(name)[1]
    return ql.default_frontend_params(seed=1, voxel_size=leaf, normal_radius=2.0 * leaf, fpfh_radius=3.0 * leaf)


# ---------------------------------------------------------------------------------------------- qtr_voxelize
@pytest.mark.parametrize("name", vc.NAMES)
def test_voxelize_equals_the_oracle(h, qo, name):
    cloud, leaf, claims = vc.case(name)
    want = _oracle(qo, name)
    got = h.voxelize(cloud, leaf)
    _equal(got, want, name)
    if claims["passed"]:  # the input's bits, the fourth column included
        assert np.array_equal(_b(got), _b(cloud))


STATE_SEQUENCE = tuple(vc.BITS_SEQUENCE_NAMES[b] for b in (25, 8, 17, 1, 24, 9)) + ("line_31_bits", "line_overflow") + (
    vc.BITS_SEQUENCE_NAMES[16], "tiles_33", "tiny_1")


def test_voxelize_on_the_state_another_call_left(qo):
    """One slot, pass counts 4 1 3 1 3 2 4 4(pass-through) 2 2 1 and tile counts between 1 and 33, then the same backwards."""
    hd = ql.Handle(0, **LIMITS)
    try:
        for step, name in enumerate(STATE_SEQUENCE + STATE_SEQUENCE[::-1]):
            cloud, leaf, _ = vc.case(name)
            _equal(hd.voxelize(cloud, leaf), _oracle(qo, name), (step, name))
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- qtr_keyframe_create
def _keyframe_equals(hd, qo, name, step):
    cloud, _, claims = vc.case(name)
    want = _oracle(qo, name)
    with hd.keyframe(cloud, _fp(name)) as kf:
        assert kf.info["n_voxels"] == want.shape[0] and kf.info["passed_through"] == int(claims["passed"]), (step, name)
        _equal(kf.fetch(ql.KF_VOX), want, (step, name))


def test_keyframes_with_speculated_passes(qo):
    """A fresh slot launches four passes; four calls in a row that needed fewer make it launch fewer, and the first call
    that needs more runs again.  The key widths 24 25 8 25 9 24, the 256-point layout clouds (one or two passes, ten in a
    row: the slot then launches two), and the widths again, the first of which now finds too few passes launched.
    The results alone are compared: that the short launch and the second run happen follows from vox_passes_next of
    front_verdict.h (four calls in a row that needed fewer; tests/test_front_verdict_cpu.py pins it) — if that
    threshold rises above the ten layout clouds, this test still passes but no longer reaches the second run."""
    widths = tuple(vc.BITS_SEQUENCE_NAMES[b] for b in (24, 25, 8, 25, 9, 24))
    hd = ql.Handle(0, **LIMITS)
    try:
        for step, name in enumerate(widths + vc.layout_names(256) + widths):
            _keyframe_equals(hd, qo, name, step)
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- qtr_feature_pair
def _feature_pair_equals(hd, qo, src, tgt, slot=0):
    (cs, leaf, _), (ct, leaf_t, _) = vc.case(src), vc.case(tgt)
    assert leaf == leaf_t
    ws, wt = _oracle(qo, src), _oracle(qo, tgt)
    got = hd.feature_pair(cs, ct, _fp(src), slot=slot)
    assert (got["n_src"], got["n_tgt"]) == (ws.shape[0], wt.shape[0]), (src, tgt)
    _equal(hd.debug_fetch(ql.DBG_VOX_SRC, np.float32, slot), ws, (src, tgt, "source"))
    _equal(hd.debug_fetch(ql.DBG_VOX_TGT, np.float32, slot), wt, (src, tgt, "target"))


@pytest.mark.parametrize("src,tgt", [("from_start_t256", "tiny_1"), ("tiny_1", "tile_last_t256"),
                                     ("tiles_33", vc.BITS_SEQUENCE_NAMES[25]), (vc.BITS_SEQUENCE_NAMES[8], "tiles_33")])
def test_two_unequal_clouds_in_one_launch(h, qo, src, tgt):
    """One cloud of a single tile (a single point) beside one whose tiles size the launch grid, on either side; 33 radix
    tiles and two passes beside three tiles and four passes (and beside one pass)."""
    _feature_pair_equals(h, qo, src, tgt)


# ---------------------------------------------------------------------------------------------- qtr_submit_batch
BATCH_PAIRS = (("from_start_t1024", "tile_last_t1024"), ("scalar_rest_t1024", "headless_t1024"),
               ("last_global_t1024", "last_global_mid_t1024"), ("last_single_t1024", "last_full_t1024"),
               ("singles_3t_t1024", "singles_3t1_t1024"))


def test_batch_with_1024_point_tiles(qo):
    """Every cloud of the batch has its own voxel count (asserted): a slot's counts say which pair it ran."""
    import torch
    dev = torch.device("cuda", 0)
    count = {n: _oracle(qo, n).shape[0] for pair in BATCH_PAIRS for n in pair}
    assert len(set(count.values())) == len(count)
    n_slots = 6  # two lanes of three slots: no slot serves two of the five pairs
    fp = _fp(BATCH_PAIRS[0][0])
    hd = ql.Handle(0, n_slots=n_slots, **LIMITS)
    try:
        items = [{"src": torch.from_numpy(np.array(vc.case(s)[0])).to(dev), "tgt": torch.from_numpy(np.array(vc.case(t)[0])).to(dev),
                  "fp": fp} for s, t in BATCH_PAIRS]
        torch.cuda.synchronize()
        got = hd.register_batch_dev(items, ql.demo_params(), fp)
        for (s, t), r in zip(BATCH_PAIRS, got):
            assert (r["n_src"], r["n_tgt"]) == (count[s], count[t]), (s, t, r)
        by_counts, seen = {(count[s], count[t]): (s, t) for s, t in BATCH_PAIRS}, set()
        for slot in range(n_slots):
            vs = hd.debug_fetch(ql.DBG_VOX_SRC, np.float32, slot).reshape(-1, 4)
            vt = hd.debug_fetch(ql.DBG_VOX_TGT, np.float32, slot).reshape(-1, 4)
            if (vs.shape[0], vt.shape[0]) == (0, 0):
                continue  # the sixth slot
            s, t = by_counts[(vs.shape[0], vt.shape[0])]
            _equal(vs, _oracle(qo, s), (slot, s))
            _equal(vt, _oracle(qo, t), (slot, t))
            seen.add((s, t))
        assert seen == set(BATCH_PAIRS)
    finally:
        hd.close()
    fresh = ql.Handle(0, **LIMITS)  # the same clouds through the pair path's 256-point tiles
    try:
        for s, t in BATCH_PAIRS:
            _feature_pair_equals(fresh, qo, s, t)
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------- capacity
def test_capacity_refusals_carry_the_exact_count(h, qo):
    name = "from_start_t256"
    cloud, leaf, claims = vc.case(name)
    want = _oracle(qo, name)
    assert want.shape[0] == claims["n_voxels"]
    out, n = np.zeros((want.shape[0] - 1, 4), dtype=np.float32), C.c_int(-1)
    rc = h._lib.qtr_voxelize(h._h, 0, cloud.ctypes.data, cloud.shape[0], leaf, out.ctypes.data, out.shape[0], C.byref(n), ql.MEM_HOST)
    assert (rc, n.value) == (ql.QTR_ERR_CAPACITY, want.shape[0])
    assert h.last_error() == "voxel count %d exceeds output capacity %d" % (want.shape[0], want.shape[0] - 1)
    assert not out.any()
    big = "tile_last_t256"
    assert _oracle(qo, big).shape[0] > 1024 >= want.shape[0]
    small = ql.Handle(0, max_points=65536, max_voxels=1024, max_corr=8192)
    try:
        with pytest.raises(ql.QuatroHipError) as e:
            small.voxelize(*vc.case(big)[:2])
        assert e.value.code == ql.QTR_ERR_CAPACITY
        assert small.last_error() == "voxel count %d exceeds max_voxels=1024" % _oracle(qo, big).shape[0]
        _equal(small.voxelize(cloud, leaf), want, name)  # 1018 voxels: the next call on the handle that refused
    finally:
        small.close()
