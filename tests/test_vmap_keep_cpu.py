"""The contract of the voxel map's upkeep (include/qtr_vmap_keep_math.h) on the host: the window rule at its edges, the
restatement (tests/vmap_ref/vmap_keep_ref.cpp, compiled by g++ from the shared headers) against an independent model in plain
Python (a dict keyed by coordinate triples, the rule in Python integers), evict followed by inserts, restore and its refusals,
and the header's entry points in the extension library's symbol table."""
import math

import numpy as np
import pytest

import vmap_cases as K
import vmap_keep_restate as KR
import vmap_restate as M

LO, HI = K.LO, K.HI
SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_sections(fa, fb, what="", keys=SECTIONS):
    for k in keys:
        assert fa[k].shape == fb[k].shape and np.array_equal(_bits(fa[k]), _bits(fb[k])), (what, k)


def _rows(f, keep):
    return {k: f[k][keep] for k in f}


def _hand_map(n_inserts=3, capacity=4096):
    inserts, _, _ = K.hand_built()
    m = KR.RefMap(K.SIDE, capacity)
    for c in inserts[:n_inserts]:
        m.insert(*c)
    return m, inserts


def _both(centre, radius, side, coords):
    """The header's verdict, checked against the Python-integer rule; None: refused by both."""
    got = KR.verdict(centre, radius, side, coords)
    win = KR.window_py(centre, radius, side)
    assert (got is None) == (win is None) == (KR.window(centre, radius, side) is None), (centre, radius, side)
    if win is None:
        return None
    assert KR.window(centre, radius, side) == win, (centre, radius, side)
    assert got == KR.kept_py(win, coords), (centre, radius, side, coords)
    return got


def test_window_rule_at_its_edges():
    for side in (1.0, 0.5, 0.3):
        # radius 0 (and -0.0) keeps exactly the centre's voxel
        for centre, C in (((0.25 * side, 0.25 * side, 0.25 * side), (0, 0, 0)), ((-0.25 * side, 7.5 * side, -3.5 * side), (-1, 7, -4)),
                          ((-0.0, 0.0, -0.0), (0, 0, 0))):
            for r0 in (0.0, -0.0, 0.999 * side):
                assert KR.window(centre, r0, side) == (C, 0)
                assert _both(centre, r0, side, C) is True
                for a in range(3):
                    for d in (-1, 1):
                        n = list(C)
                        n[a] += d
                        assert _both(centre, r0, side, n) is False
    for side in (1.0, 0.5):  # (k side is exact)
        # a centre exactly on the face k side belongs to voxel k, for negative k too
        assert KR.window((3 * side, -3 * side, 0.0), 0.0, side)[0] == (3, -3, 0)
        assert KR.window((np.nextafter(3 * side, 0), np.nextafter(-3 * side, -np.inf), -1e-300), 0.0, side)[0] == (2, -4, -1)
        # the tie: |(3, 4, 0)|^2 = 25 = R^2 is kept; one ulp less radius is R = 4 and evicts it
        c = (0.5 * side, 0.5 * side, 0.5 * side)
        assert KR.window(c, 5 * side, side) == ((0, 0, 0), 25)
        assert _both(c, 5 * side, side, (3, 4, 0)) is True and _both(c, 5 * side, side, (-4, 0, -3)) is True
        assert _both(c, 5 * side, side, (3, 4, 1)) is False
        assert KR.window(c, np.nextafter(5 * side, 0), side) == ((0, 0, 0), 16)
        assert _both(c, np.nextafter(5 * side, 0), side, (3, 4, 0)) is False
        assert _both(c, np.nextafter(5 * side, 0), side, (0, 4, 0)) is True
        # the ends of the grid against each other: differences of 2^21 - 1 per axis, sums near 2^44, no overflow
        far = (HI * side, HI * side, HI * side)
        assert KR.window(far, 0.0, side)[0] == (HI, HI, HI)
        D = (1 << 21) - 1
        assert _both(far, D * side, side, (LO, HI, HI)) is True          # D^2 <= D^2
        assert _both(far, (D - 1) * side, side, (LO, HI, HI)) is False
        assert _both(far, D * side, side, (LO, LO, HI)) is False         # 2 D^2 > D^2
        big = ((1 << 22) - 1) * side
        assert KR.window(far, big, side)[1] == ((1 << 22) - 1) ** 2
        assert _both(far, big, side, (LO, LO, LO)) is True               # 3 D^2 < (2^22 - 1)^2
        near = (LO * side, LO * side, LO * side)
        assert _both(near, (D + 1) * side, side, (HI, HI, HI)) is False and _both(near, big, side, (HI, HI, HI)) is True
        # refused
        ok = (0.25, 0.25, 0.25)
        for bad in (np.nan, np.inf, -np.inf):
            for a in range(3):
                c = list(ok)
                c[a] = bad
                assert _both(c, 1.0, side, (0, 0, 0)) is None
        for bad_r in (-1.0, -1e-300, np.nan, np.inf, -np.inf, (1 << 22) * side, 1e300):
            assert _both(ok, bad_r, side, (0, 0, 0)) is None, bad_r
        assert _both(ok, np.nextafter((1 << 22) * side, 0), side, (0, 0, 0)) is True
        for a in range(3):
            for x, inside in (((1 << 20) * side, False), (np.nextafter((1 << 20) * side, 0), True), (-(1 << 20) * side, True),
                              (np.nextafter(-(1 << 20) * side, -np.inf), False), (1e300, False)):
                c = list(ok)
                c[a] = x
                assert (_both(c, 1.0, side, (0, 0, 0)) is not None) == inside, (a, x)
    # at random: the header against Python integers
    rng = np.random.default_rng(5)
    n_kept = 0
    for _ in range(2000):
        side = float(rng.choice([1.0, 0.5, 0.3, 0.7]))
        centre = rng.normal(scale=20.0, size=3)
        radius = float(abs(rng.normal(scale=15.0)))
        coords = np.floor(centre / side).astype(np.int64) + rng.integers(-40, 41, 3)
        n_kept += bool(_both(centre, radius, side, coords))
    assert 200 < n_kept < 1800


def test_evict_is_the_rows_that_pass_in_both_models():
    m0, _ = _hand_map()
    before = m0.fetch_all()
    n_before, members_before = len(m0), m0.info()["n_members"]
    assert n_before > 100
    for centre, radius in (((0.3, -0.2, 0.1), 1.6), ((1.6, -0.9, 0.6), 0.0), ((-2.0, 2.5, 0.0), 1.0), ((0.0, 0.0, 0.0), 2.5),
                           ((LO * K.SIDE, 0.25, 0.25), 3.0)):
        m, _ = _hand_map()
        model = KR.DictMap(K.SIDE, before)
        info = m.evict(centre, radius)
        assert info == model.evict(centre, radius), (centre, radius)
        win = KR.window_py(centre, radius, K.SIDE)
        keep = np.array([KR.kept_py(win, c) for c in before[M.COORDS]])
        assert 0 < keep.sum() < n_before, (centre, radius)
        after = m.fetch_all()
        _same_sections(after, _rows(before, keep), (centre, radius))          # every section: the rows that pass
        _same_sections(after, model.sections(), (centre, radius), (M.COORDS, M.COUNT, M.SUMS))
        assert info["n_kept"] == int(keep.sum()) == len(m) and info["n_evicted"] == n_before - len(m)
        assert info["n_members_evicted"] == int(before[M.COUNT][~keep].sum())
        i = m.info()
        assert (i["n_voxels"], i["n_inserts"], i["n_members"]) == (len(m), 3, members_before - info["n_members_evicted"])


def test_evict_then_insert_continues_kept_voxels_and_restarts_evicted_ones():
    centre, radius = (0.3, -0.2, 0.1), 1.6
    whole, inserts = _hand_map(3)       # never evicted
    m, _ = _hand_map(2)
    at_evict = m.fetch_all()
    m.evict(centre, radius)
    kept = {tuple(c) for c in m.fetch(M.COORDS)}
    gone = {tuple(c) for c in at_evict[M.COORDS]} - kept
    info = m.insert(*inserts[2])
    alone = KR.RefMap(K.SIDE, 4096)     # insert 2 into an empty map: what a restarted voxel holds
    alone.insert(*inserts[2])
    fw, fa, fm = whole.fetch_all(), alone.fetch_all(), m.fetch_all()
    iw = {tuple(c): j for j, c in enumerate(fw[M.COORDS])}
    ia = {tuple(c): j for j, c in enumerate(fa[M.COORDS])}
    n_cont = n_restart = n_new = 0
    for j, c in enumerate(map(tuple, fm[M.COORDS])):
        src, row = (fw, iw[c]) if c in kept else (fa, ia[c])
        for k in SECTIONS:
            assert np.array_equal(_bits(fm[k][j]), _bits(src[k][row])), (c, k)
        n_cont += c in kept and c in ia
        n_restart += c in gone
        n_new += c not in kept and c not in gone
    assert n_cont > 0 and n_restart > 0 and n_new > 0            # the third insert touches all three kinds
    assert set(map(tuple, fm[M.COORDS])) == kept | set(ia)
    assert info["n_new_voxels"] == n_restart + n_new and info["n_touched_voxels"] == len(ia)
    assert m.info()["n_inserts"] == 3
    # nothing evicted: the identity;  everything evicted: an empty map that takes inserts
    same, _ = _hand_map()
    f0, i0 = same.fetch_all(), same.info()
    assert same.evict((0.0, 0.0, 0.0), (1 << 21) * K.SIDE) == {"n_kept": len(same), "n_evicted": 0, "n_members_evicted": 0}
    _same_sections(same.fetch_all(), f0)
    assert same.info() == i0
    e = same.evict((1000.0, 1000.0, 1000.0), 0.0)
    assert (e["n_kept"], e["n_evicted"], e["n_members_evicted"]) == (0, i0["n_voxels"], i0["n_members"])
    assert len(same) == 0 and same.info()["n_members"] == 0 and same.info()["n_inserts"] == 3
    assert all(v.shape[0] == 0 for v in same.fetch_all().values())
    same.insert(*inserts[2])
    _same_sections(same.fetch_all(), fa)
    # an empty map: nothing to evict
    assert KR.RefMap(1.0, 4).evict((0, 0, 0), 1.0) == {"n_kept": 0, "n_evicted": 0, "n_members_evicted": 0}
    with pytest.raises(KR.BadArgError):
        same.evict((np.nan, 0, 0), 1.0)
    _same_sections(same.fetch_all(), fa)


def test_restore_gives_the_map_back_for_any_capacity_and_refuses_the_rest():
    src, inserts = _hand_map(2)
    f = src.fetch_all()
    n = len(src)
    extra = K.cloud_of_voxels([K.V65, (9, 9, 9), K.V1], K.SIDE, per_voxel=(4, 2, 3), seed=12)
    want_info = src.insert(*inserts[2])
    want_more = src.insert(*extra)
    want = src.fetch_all()
    for cap in (n, 1 << 10, 1 << 16):
        m = KR.RefMap(K.SIDE, cap)
        perm = np.random.default_rng(cap).permutation(n)       # the order of the rows is free
        m.restore(f[M.COORDS][perm], f[M.COUNT][perm], f[M.SUMS][perm])
        _same_sections(m.fetch_all(), f, cap)
        i = m.info()
        assert (i["n_voxels"], i["n_inserts"], i["n_members"]) == (n, 0, int(f[M.COUNT].sum()))
        if cap > n:   # the inserts that follow give the same bits as on the map the sections came from
            assert m.insert(*inserts[2]) == want_info and m.insert(*extra) == want_more
            _same_sections(m.fetch_all(), want, cap)
    # refusals: each leaves an empty map that works
    c, k, s = f[M.COORDS].copy(), f[M.COUNT].copy(), f[M.SUMS].copy()

    def refused(exc, cap, cc, kk, ss):
        m = KR.RefMap(K.SIDE, cap)
        with pytest.raises(exc):
            m.restore(cc, kk, ss)
        assert len(m) == 0 and m.info()["n_members"] == 0
        m.restore(c, k, s) if cap >= n else m.restore(c[:cap], k[:cap], s[:cap])
        assert len(m) == min(n, cap)

    refused(M.CapacityError, n - 1, c, k, s)
    dup = c.copy()
    dup[n - 1] = dup[3]
    refused(KR.BadArgError, 4096, dup, k, s)
    for bad_count in (0, -1, -(1 << 31)):
        kk = k.copy()
        kk[n // 2] = bad_count
        refused(KR.BadArgError, 4096, c, kk, s)
    for a, bad in ((0, HI + 1), (1, LO - 1), (2, (1 << 31) - 1), (0, -(1 << 31))):
        cc = c.copy()
        cc[5, a] = bad
        refused(KR.BadArgError, 4096, cc, k, s)
    full, _ = _hand_map(1)
    had = full.fetch_all()
    with pytest.raises(KR.BadArgError):  # a map that holds voxels: refused, and it keeps them
        full.restore(c, k, s)
    _same_sections(full.fetch_all(), had)
    empty = KR.RefMap(K.SIDE, 8)
    empty.restore(c[:0], k[:0], s[:0])
    assert len(empty) == 0


def test_the_two_entry_points_are_declared_exported_and_bound():
    """The entry points of include/quatro_voxelmap_keep.h are two of libquatro_ext.so's exports, both have their ctypes
    signatures, libquatro_hip.so exports neither, and the info struct is its ctypes mirror."""
    import ctypes
    import os
    import subprocess
    import tempfile
    import ext_abi
    from quatro_amd import lib as ql
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    assert ext_abi.check_header("quatro_voxelmap_keep.h") == {"qtr_voxel_map_evict", "qtr_voxel_map_restore"}
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "quatro_voxelmap_keep.h"
int main(void){printf("%zu %zu %zu %zu\n", sizeof(qtr_voxel_map_evict_info), offsetof(qtr_voxel_map_evict_info, n_kept),
  offsetof(qtr_voxel_map_evict_info, n_evicted), offsetof(qtr_voxel_map_evict_info, n_members_evicted)); return 0;}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", os.path.join(d, "s")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    E = ql.VoxelMapEvictInfo
    assert got == [ctypes.sizeof(E), E.n_kept.offset, E.n_evicted.offset, E.n_members_evicted.offset] == [16, 0, 4, 8]
