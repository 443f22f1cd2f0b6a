"""The FPFH chain's kernels (k2_cell_* / k2_ranges, k2_neighbors, k2_neighbors_big, k2_normals, k2_spfh, k2_fpfh) and the
voxel grid on the named clouds of tests/front_cases.py — degenerate geometry, list lengths on both sides of every sort
and staging switch, pairs that only the margin of the cell side keeps in reach — against the CPU oracle, bit for bit:
`(bits equal) | (both NaN)` for every float, no tolerance anywhere.  tests/test_front_cases_cpu.py holds the oracle to
independent references on the same clouds and asserts that every cloud is on the branch it is named after.

Every cloud runs along both forms of the neighbour grid:

  * qtr_fpfh: no voxel stage in front, the points are sorted by packed cell keys and k2_ranges finds the nine key ranges;
    the chain always carries k2_neighbors_big.  Normals, QTR_DBG_SPFH and descriptors against the oracle, the offsets and —
    as far as qtr_debug_fetch defines them — the lists against the brute force;
  * qtr_keyframe_create + qtr_keyframe_fetch: the voxel grid first, at a leaf that leaves every point a voxel of its own
    (or, for a grid beyond int32, hands the cloud back as it is), then the dense cell table (k2_cell_count / _scan /
    _place): every cloud here has a grid of at most QTR_CELL_CAP cells, which is what cell_table_cells of capi.hip asks
    for.  Voxels, normals and descriptors against the oracle's voxelize + fpfh.

far_plane and denormal_d2 produce NaN normals and NaN descriptors on purpose and take the keyframe route too: the tail of
k2_fpfh that prepares a descriptor for the matcher forms its norm (a float, NaN), hashes the BIT PATTERNS of the 33
values, and enters the duplicate table at `hash & mask`, probing at most mask + 1 slots — no index depends on the value
of a NaN, and the keyframe's pack is a plain copy.
"""
import os
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=4096, max_voxels=1024, max_corr=1024, max_long_neighbors=1 << 18)
_want = {}


def _b(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((_b(got) == _b(want)) | (np.isnan(got) & np.isnan(want))))


@pytest.fixture(scope="module")
def h():
    """the handle of the qtr_fpfh route and of the keyframes without long lists: its keyframe chains never carry
    k2_neighbors_big"""
    hd = ql.Handle(0, **LIMITS)
    yield hd
    hd.close()


def _oracle(qo, name, route):
    """(points, normals, SPFH, descriptors) the route must reproduce, computed once"""
    if (name, route) not in _want:
        c = fc.case(name)
        pts = c.cloud if route == "fpfh" else qo.voxelize(c.cloud, fc.keyframe_leaf(name))
        _want[(name, route)] = (pts,) + tuple(qo.fpfh(pts, c.r_normal, c.r_fpfh))
    return _want[(name, route)]


@pytest.mark.parametrize("name", fc.FPFH_NAMES)
def test_fpfh_by_sorted_keys_equals_the_oracle(h, qo, name):
    c = fc.case(name)
    n = c.cloud.shape[0]
    _, nrm_o, sp_o, de_o = _oracle(qo, name, "fpfh")
    nrm_g, de_g = h.fpfh(c.cloud, c.r_normal, c.r_fpfh)
    off_g = h.debug_fetch(ql.DBG_NBR_OFFSETS, np.int32).astype(np.int64)
    sp_g = h.debug_fetch(ql.DBG_SPFH, np.float32).reshape(n, 33)
    boff, bidx, bd2 = fc.brute_neighbors(c.cloud, c.r_fpfh)
    assert np.array_equal(off_g, boff)
    # qtr_debug_fetch hands out the head of the fixed-stride slot array, sum(k) entries of it: the list of point i lies at
    # QTR_KMAX i while it is no longer than the slot (a longer one lives in the arena, its slot holds the offset there)
    idx_g, d2_g = h.debug_fetch(ql.DBG_NBR_INDEX, np.int32), h.debug_fetch(ql.DBG_NBR_DIST2, np.float32)
    assert idx_g.size == d2_g.size == boff[-1]
    seen = 0
    for i in range(n):
        k, at = int(boff[i + 1] - boff[i]), fc.QTR_KMAX * i
        if k > fc.QTR_KMAX or at + k > idx_g.size:
            continue
        assert np.array_equal(idx_g[at:at + k], bidx[boff[i]:boff[i + 1]]), (name, i)
        assert np.array_equal(_b(d2_g[at:at + k]), _b(bd2[boff[i]:boff[i + 1]])), (name, i)
        seen += 1
    assert seen >= 1 or boff[1] > fc.QTR_KMAX
    assert _same(nrm_g, nrm_o)
    assert _same(sp_g, sp_o)
    assert _same(de_g, de_o)


def _keyframe_equals_the_oracle(hd, qo, name):
    c = fc.case(name)
    dims, _ = fc.grid_cells(c.cloud, c.r_fpfh)
    assert 0 < dims.prod() <= fc.QTR_CELL_CAP  # the route taken: the dense cell table (capi.hip, cell_table_cells)
    pts, nrm_o, _, de_o = _oracle(qo, name, "keyframe")
    fp = ql.default_frontend_params(voxel_size=fc.keyframe_leaf(name), normal_radius=c.r_normal, fpfh_radius=c.r_fpfh)
    with hd.keyframe(c.cloud, fp) as kf:
        assert kf.info["n_voxels"] == pts.shape[0] == c.cloud.shape[0]
        assert np.array_equal(_b(kf.fetch(ql.KF_VOX)), _b(pts))
        assert _same(kf.fetch(ql.KF_NORMALS), nrm_o)
        assert _same(kf.fetch(ql.KF_FPFH), de_o)


@pytest.mark.parametrize("name", [n for n in fc.FPFH_NAMES if n not in fc.LONG_LIST_NAMES])
def test_keyframe_by_the_dense_cell_table_equals_the_oracle(h, qo, name):
    """wide_extent: its box is 267 cells long, cell_of clamps at 255 and the grid has 256 x 2 x 1 cells — far below
    QTR_CELL_CAP, so the host takes the dense cell table, with every point beyond cell 255 in the last cell."""
    _keyframe_equals_the_oracle(h, qo, name)


@pytest.mark.parametrize("name", fc.LONG_LIST_NAMES)
def test_keyframe_with_long_lists_on_a_fresh_and_on_a_warm_handle(qo, name):
    """A fresh handle's chain starts without k2_neighbors_big: the counts come back pending, the chain runs again with it.
    The second keyframe of the same handle has it from the start."""
    hd = ql.Handle(0, **LIMITS)
    try:
        _keyframe_equals_the_oracle(hd, qo, name)
        _keyframe_equals_the_oracle(hd, qo, name)
    finally:
        hd.close()


def test_voxel_grid_on_voxel_borders(h, qo):
    c = fc.case("voxel_borders")
    leaf = c.claims["leaf"]
    got = h.voxelize(c.cloud, leaf)
    assert got.shape[0] == c.claims["n_voxels"]
    assert np.array_equal(_b(got), _b(qo.voxelize(c.cloud, leaf)))
    assert np.array_equal(_b(got[:, :3]), _b(fc.voxelize_numpy(c.cloud, leaf)))


def test_spfh_angle_bin_on_the_device(h, qo):
    """fn 4 is the bin k2_spfh stores (the shortcut, then the arc tangent where it is not sure), fn 6 the shortcut alone.
    fn 4 equals the oracle's plain arithmetic everywhere; fn 6 equals the numpy mirror exactly — a difference would be a
    finding about the build's arithmetic (a contraction, a constant rounded otherwise), not something to tolerate."""
    inp = fc.angle_bin_inputs()
    y, x = inp.y, inp.x
    want = qo.math_fn(4, y, x)
    assert np.array_equal(want.astype(np.int64), fc.angle_bin_want(qo, y, x))
    full = h.debug_math(4, y, x)
    raw = h.debug_math(6, y, x)
    assert np.array_equal(_b(full), _b(want))
    assert np.all((raw == -1) | ((raw >= 0) & (raw <= 10) & (raw == np.floor(raw))))
    assert (raw[inp.uniform] >= 0).mean() > 0.9999
    assert np.all(raw[inp.zero_y | inp.nonfinite | inp.out_of_guard] == -1)
    assert np.array_equal(raw[raw >= 0], full[raw >= 0])
    sure, got = fc.angle_bin_mirror(y, x)
    assert np.array_equal(raw >= 0, sure)
    assert np.array_equal(raw[sure].astype(np.int64), got[sure])
    assert set(np.unique(raw[sure])) == set(float(b) for b in range(11))
