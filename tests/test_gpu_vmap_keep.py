"""The voxel map's upkeep on the MI355X (qtr_voxel_map_evict / qtr_voxel_map_restore, libquatro_ext.so): bit-parity
with the host restatement (tests/vmap_ref/vmap_keep_ref.cpp) of all five fetch sections and the info after an eviction and
after the inserts that follow it, a crowded table whose wrapping probe chains lose voxels from their middle, the windows
that keep everything and nothing, restore into maps of other capacities from host and device memory with its refusals, save
and load, the windowed scan-to-map odometry, and the C++ demo.  Everything goes through the C ABI (quatro_amd.lib)."""
import os
import subprocess

import numpy as np
import pytest

import icp_restate as R
import vmap_cases as K
import vmap_keep_restate as KR
import vmap_restate as M

pytestmark = pytest.mark.gpu

ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")
SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)
# the hand-built case's window: centre voxel (2, 0, -1), R = floor(1.6 / 0.5) = 3.  It keeps V1 (1 member, distance^2 9: the
# tie) and V300 (300 members, 8) among 19 of the 276 voxels and drops V65 (65 members) and VALL (21, from all three inserts)
CENTRE, RADIUS = (1.25, 0.25, -0.25), 1.6


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same_icp(a, b, what=""):
    assert a.get("status", 0) == b.get("status", 0), what
    assert np.array_equal(_bits(a["T"]), _bits(b["T"])), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _sections(m):
    return m.fetch_all() if isinstance(m, M.RefMap) else {k: m.fetch(k) for k in SECTIONS}


def _same_sections(fa, fb, what=""):
    for k in SECTIONS:
        assert fa[k].shape == fb[k].shape and np.array_equal(_bits(fa[k]), _bits(fb[k])), (what, k)


def _same_map(a, b, what="", inserts=True):
    _same_sections(_sections(a), _sections(b), what)
    ia, ib = a.info(), b.info()
    keys = ("n_voxels", "n_inserts", "n_members") if inserts else ("n_voxels", "n_members")
    assert all(ia[k] == ib[k] for k in keys), (what, ia, ib)


def _vg(**kw):
    from quatro_amd import lib as ql
    return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)


def _register(hip, vm, s, sn, guess, iters):
    """A registration of `iters` iterations (both epsilons 0): (result, trace, correspondence flags)."""
    from quatro_amd import lib as ql
    g = vm.register(s, sn, guess, _vg(max_iterations=iters, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0))
    return g, hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18), hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)


def _register_both(hip, vm, ref, s, sn, guess, iters, what=""):
    """... on the device and in the restatement: final record, the trace of every update (T, n_corr, stop, fitness, rmse) and
    the last correspondence flags, bit for bit.  Returns the device triple."""
    g, trace, corr = _register(hip, vm, s, sn, guess, iters)
    o = ref.register(s, sn, guess, teps=0.0, feps=0.0, max_iter=iters)
    _same_icp(g, o, what)
    assert np.array_equal(_bits(trace), _bits(o["trace"])) and np.array_equal(corr, o["corr"]), what
    return g, trace, corr


def _refused(code, word, fn, *a, **k):
    from quatro_amd import lib as ql
    with pytest.raises(ql.QuatroHipError) as ei:
        fn(*a, **k)
    assert ei.value.code == code and word in str(ei.value), (word, str(ei.value))


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


@pytest.fixture(scope="module")
def hand():
    return K.hand_built()


def _hand_maps(hip, hand, capacity=4096):
    inserts, _, _ = hand
    vm, ref = hip.voxel_map(K.SIDE, capacity), KR.RefMap(K.SIDE, capacity)
    for p, n, pose in inserts:
        assert vm.insert(p, n, pose) == ref.insert(p, n, pose)
    return vm, ref


@pytest.fixture(scope="module")
def hand_sections(hand):
    """The hand-built map's five sections, from the restatement (computed once, read only)."""
    inserts, _, _ = hand
    ref = KR.RefMap(K.SIDE, 4096)
    for c in inserts:
        ref.insert(*c)
    f = ref.fetch_all()
    for v in f.values():
        v.setflags(write=False)
    return f


def test_hand_built_map_after_an_eviction_is_bit_equal_to_the_restatement(hip, hand, hand_sections):
    vm, ref = _hand_maps(hip, hand)
    try:
        before = _sections(vm)
        _same_sections(before, hand_sections, "before")
        win = KR.window_py(CENTRE, RADIUS, K.SIDE)
        keep = np.array([KR.kept_py(win, c) for c in before[M.COORDS]])
        by = {tuple(c): bool(k) for c, k in zip(before[M.COORDS], keep)}
        assert (by[K.V1], by[K.V65], by[K.V300], by[K.VALL]) == (True, False, True, False) and keep.sum() == 19
        # sources that fall only into kept voxels (the seven within distance^2 5 of the centre's), drawn towards their centres
        kc = before[M.COORDS][keep]
        inner = kc[((kc - np.array(win[0])) ** 2).sum(axis=1) <= 5]
        s, sn = K.cloud_of_voxels(inner, K.SIDE, per_voxel=(9,), seed=4)
        s[:, :3] = (s[:, :3].astype(np.float64) * 0.6 + 0.4 * ((np.floor(s[:, :3] / K.SIDE) + 0.5) * K.SIDE)).astype(np.float32)
        guess = R.rigid(R.rot(0.004, -0.003, 0.005), [0.01, -0.008, 0.006])
        g0, trace0, corr0 = _register_both(hip, vm, ref, s, sn, guess, 6, "before the eviction")
        assert g0["valid"] and g0["iterations"] == 6 and g0["n_corr"] > 40
        got, want = vm.evict(CENTRE, RADIUS), ref.evict(CENTRE, RADIUS)
        assert got == want == {"n_kept": 19, "n_evicted": 257, "n_members_evicted": int(before[M.COUNT][~keep].sum())}
        _same_map(vm, ref, "after the eviction")
        _same_sections(_sections(vm), {k: before[k][keep] for k in SECTIONS}, "the rows that pass")   # moved, not recomputed
        g1, trace1, corr1 = _register_both(hip, vm, ref, s, sn, guess, 6, "after the eviction")
        _same_icp(g1, g0, "the same registration before and after")
        assert np.array_equal(_bits(trace1), _bits(trace0)) and np.array_equal(corr1, corr0)
        # one more insert: a kept voxel (V300 goes on from its 300 members), an evicted one (V65 starts anew) and a new one
        more, more_n = K.cloud_of_voxels([K.V300, K.V65, (9, 9, 9)], K.SIDE, per_voxel=(5, 3, 2), seed=9)
        i = vm.insert(more, more_n)
        assert i == ref.insert(more, more_n) and (i["n_new_voxels"], i["n_touched_voxels"]) == (2, 3)
        _same_map(vm, ref, "after the insert that follows")
        after = {tuple(c): int(n) for c, n in zip(vm.fetch(M.COORDS), vm.fetch(M.COUNT))}
        assert (after[K.V300], after[K.V65], after[(9, 9, 9)], after[K.V1]) == (305, 3, 2, 1) and K.VALL not in after
        _register_both(hip, vm, ref, s, sn, guess, 4, "after the insert that follows")
        # a second eviction (the staging exists now) and the insert's scratch after a rebuild
        e = vm.evict((4.6, 4.6, 4.6), 0.0)   # radius 0: only the new voxel (9, 9, 9) stays
        assert e == ref.evict((4.6, 4.6, 4.6), 0.0) and (e["n_kept"], e["n_evicted"]) == (1, 20)
        assert e["n_members_evicted"] == int(before[M.COUNT][keep].sum()) + 5 + 3
        _same_map(vm, ref, "a second eviction")
        assert vm.insert(more, more_n) == ref.insert(more, more_n)
        _same_map(vm, ref, "an insert after the second eviction")
    finally:
        vm.destroy()


def test_crowded_table_loses_voxels_from_the_middle_of_its_chains(hip):
    """64 voxels of capacity (128 slots), 62 voxels whose probe chains all start in the last six slots and wrap: they fill
    one run of slots, and a voxel's slot is as far from its home as the run is long.  The window (a ball of 200 voxels about
    the origin for coordinates drawn from [-200, 200)^3) drops about half of them wherever they sit in that run; writing the
    empty key over them would cut the chains of the rest."""
    from quatro_amd import lib as ql
    coords, extra = K.crowded(64, 62)
    S = M.table_slots(64)
    assert S == 128 and all(M.hash_slot(M.key(*c), S) >= S - 6 for c in np.concatenate([coords, extra]))
    pts, nrm = K.cloud_of_voxels(coords, 1.0)
    vm, ref = hip.voxel_map(1.0, 64), KR.RefMap(1.0, 64)
    try:
        assert vm.insert(pts, nrm) == ref.insert(pts, nrm)
        win = KR.window_py((0.5, 0.5, 0.5), 200.0, 1.0)
        keep = np.array([KR.kept_py(win, c) for c in coords])
        kept, gone = coords[keep], coords[~keep]
        assert 20 <= len(kept) <= 42, len(kept)
        assert vm.evict((0.5, 0.5, 0.5), 200.0) == ref.evict((0.5, 0.5, 0.5), 200.0)
        assert len(vm) == len(kept)
        _same_map(vm, ref, "after the eviction")
        # every kept voxel is still found: one source point per kept voxel, all of them matched ...
        s, sn = K.cloud_of_voxels(kept, 1.0, per_voxel=(1,), seed=8)
        g, _, corr = _register_both(hip, vm, ref, s, sn, np.eye(4), 1, "one point per kept voxel")
        assert g["n_corr"] == len(kept) and (corr == 0).all()
        s2, sn2 = K.cloud_of_voxels(gone, 1.0, per_voxel=(1,), seed=8)   # ... and none of the evicted ones
        g, _, corr = _register(hip, vm, s2, sn2, np.eye(4), 1)
        assert g["n_corr"] == 0 and (corr == -1).all()
        # ... and by an insert: points into kept voxels claim nothing
        again, again_n = K.cloud_of_voxels(kept, 1.0, per_voxel=(2, 1), seed=7)
        i = vm.insert(again, again_n)
        assert i == ref.insert(again, again_n) and (i["n_new_voxels"], i["n_touched_voxels"]) == (0, len(kept))
        _same_map(vm, ref, "kept voxels touched again")
        # the rollback invariant after a rebuild: up to exactly 64 voxels fits, one more is refused with nothing changed
        fill = np.concatenate([gone, extra[:2]])
        assert len(kept) + len(fill) == 64
        fit, fit_n = K.cloud_of_voxels(np.concatenate([kept[:5], fill]), 1.0, seed=5)
        i = vm.insert(fit, fit_n)
        assert i == ref.insert(fit, fit_n) and i["n_new_voxels"] == len(fill)
        _same_map(vm, ref, "64 of 64 voxels")
        before = _sections(vm)
        one, one_n = K.cloud_of_voxels(np.concatenate([kept[:3], extra[2:3]]), 1.0, seed=6)   # the 65th voxel
        _refused(ql.QTR_ERR_CAPACITY, "capacity=64", vm.insert, one, one_n)
        with pytest.raises(M.CapacityError):
            ref.insert(one, one_n)
        _same_sections(_sections(vm), before, "after the refusal")
        _same_map(vm, ref, "after the refusal")
        s3, sn3 = K.cloud_of_voxels(np.concatenate([coords, extra[:2]]), 1.0, per_voxel=(1,), seed=3)
        g, _, _ = _register_both(hip, vm, ref, s3, sn3, np.eye(4), 1, "full table")
        assert g["n_corr"] == 64
        # a second eviction on the full table, the other half this time
        assert vm.evict((150.5, 150.5, 150.5), 200.0) == ref.evict((150.5, 150.5, 150.5), 200.0)
        assert 0 < len(vm) < 64
        _same_map(vm, ref, "a second eviction")
        _register_both(hip, vm, ref, s3, sn3, np.eye(4), 1, "after the second eviction")
    finally:
        vm.destroy()


def test_windows_that_keep_everything_and_nothing(hip, hand, hand_sections):
    from quatro_amd import lib as ql
    inserts, s, sn = hand
    vm, ref = _hand_maps(hip, hand)
    try:
        info0 = vm.info()
        e = vm.evict((0.0, 0.0, 0.0), (1 << 21) * K.SIDE)
        assert e == ref.evict((0.0, 0.0, 0.0), (1 << 21) * K.SIDE) == {"n_kept": 276, "n_evicted": 0, "n_members_evicted": 0}
        _same_sections(_sections(vm), hand_sections, "everything kept")
        assert vm.info() == info0
        _register_both(hip, vm, ref, s, sn, K.GUESS, 3, "everything kept")
        e = vm.evict((1000.0, 1000.0, 1000.0), 0.0)
        assert e == ref.evict((1000.0, 1000.0, 1000.0), 0.0) == {"n_kept": 0, "n_evicted": 276, "n_members_evicted": info0["n_members"]}
        i = vm.info()
        assert (i["n_voxels"], i["n_members"], i["n_inserts"]) == (0, 0, 3) and len(vm) == 0
        assert vm.fetch(M.CLOUD).shape == (0, 4) and vm.fetch(M.COORDS).shape == (0, 3) and vm.fetch(M.SUMS).shape == (0, 9)
        g = vm.register(s, sn, K.GUESS)
        assert not g["valid"] and g["n_corr"] == 0 and g["stop_reason"] == ql.ICP_STOP_TOO_FEW and np.array_equal(g["T"], K.GUESS)
        assert vm.evict((0.0, 0.0, 0.0), 1.0) == {"n_kept": 0, "n_evicted": 0, "n_members_evicted": 0}   # an empty map
        for p, n, pose in inserts[1:]:
            assert vm.insert(p, n, pose) == ref.insert(p, n, pose)
        _same_map(vm, ref, "inserts after everything left")
        # refused windows: nothing happens
        want = _sections(vm)
        for centre, radius in (((np.nan, 0, 0), 1.0), ((0, np.inf, 0), 1.0), ((0, 0, 0), -1.0), ((0, 0, 0), np.nan),
                               ((0, 0, 0), (1 << 22) * K.SIDE), (((1 << 20) * K.SIDE, 0, 0), 1.0)):
            _refused(ql.QTR_ERR_BAD_ARG, "evict", vm.evict, centre, radius)
            with pytest.raises(KR.BadArgError):
                ref.evict(centre, radius)
        _refused(ql.QTR_ERR_BAD_ARG, "slot", vm.evict, (0, 0, 0), 1.0, slot=7)
        _same_sections(_sections(vm), want, "after the refused windows")
    finally:
        vm.destroy()


@pytest.mark.parametrize("centre,radius,kept", [((0.5, 0.5, 0.5), 10.0, 3), ((0.5, 0.5, 0.5), 2.0, 2), ((100.5, 0.5, 0.5), 0.0, 0)])
def test_three_voxels_in_128_slots_through_every_end_of_the_rebuild(hip, centre, radius, kept):
    """The smallest map that takes each path behind the mark pass: everything kept (the table is only read), exactly one
    voxel gone (stage, clear, put) and all gone (clear alone)."""
    coords = np.array([(0, 0, 0), (1, 0, 0), (5, 0, 0)])
    pts, nrm = K.cloud_of_voxels(coords, 1.0, per_voxel=(4, 2, 7), seed=12)
    assert M.table_slots(64) == 128
    vm, ref = hip.voxel_map(1.0, 64), KR.RefMap(1.0, 64)
    try:
        assert vm.insert(pts, nrm) == ref.insert(pts, nrm)
        before = _sections(vm)
        win = KR.window_py(centre, radius, 1.0)
        keep = np.array([KR.kept_py(win, c) for c in before[M.COORDS]], dtype=bool)
        assert keep.sum() == kept
        e = vm.evict(centre, radius)
        assert e == ref.evict(centre, radius) and (e["n_kept"], e["n_evicted"]) == (kept, 3 - kept)
        assert e["n_members_evicted"] == int(before[M.COUNT][~keep].sum())
        _same_map(vm, ref, f"{kept} of 3 kept")
        _same_sections(_sections(vm), {k: before[k][keep] for k in SECTIONS}, "the rows that stay")
        assert vm.insert(pts, nrm) == ref.insert(pts, nrm)
        _same_map(vm, ref, "an insert after it")
    finally:
        vm.destroy()


def test_restore_from_host_and_device_memory_into_other_capacities(hip, hand, hand_sections):
    import torch
    from quatro_amd import lib as ql
    inserts, s, sn = hand
    f = hand_sections
    n = f[M.COORDS].shape[0]
    assert n == 276
    src, ref = _hand_maps(hip, hand)
    made = [src]
    extra = K.cloud_of_voxels([K.V65, (9, 9, 9), K.V1], K.SIDE, per_voxel=(4, 2, 3), seed=12)
    try:
        g0, trace0, corr0 = _register_both(hip, src, ref, s, sn, K.GUESS, 12, "the original")
        assert g0["valid"] and g0["iterations"] == 12
        want_info = src.insert(*extra)
        assert want_info == ref.insert(*extra)
        want_after = _sections(src)
        for cap, dev in ((276, False), (512, True), (1 << 12, False), (1 << 16, True)):
            vm = hip.voxel_map(K.SIDE, cap)
            made.append(vm)
            perm = np.random.default_rng(cap).permutation(n)   # (the rows' order is free)
            c, k, a = (np.ascontiguousarray(f[x][perm]) for x in (M.COORDS, M.COUNT, M.SUMS))
            if dev:
                vm.restore(*[torch.from_numpy(x).cuda() for x in (c, k, a)], slot=1)
            else:
                vm.restore(c, k, a)
            _same_sections(_sections(vm), f, f"capacity {cap}")
            i = vm.info()
            assert (i["n_voxels"], i["n_inserts"], i["n_members"], i["capacity"]) == (n, 0, int(f[M.COUNT].sum()), cap)
            g, trace, corr = _register(hip, vm, s, sn, K.GUESS, 12)
            _same_icp(g, g0, f"capacity {cap}")
            assert np.array_equal(_bits(trace), _bits(trace0)) and np.array_equal(corr, corr0), cap
            if cap > n:
                assert vm.insert(*extra) == want_info
                _same_sections(_sections(vm), want_after, f"capacity {cap}: the insert that follows")
        # refusals: each leaves an empty map that works
        c, k, a = f[M.COORDS].copy(), f[M.COUNT].copy(), f[M.SUMS].copy()
        vm = hip.voxel_map(K.SIDE, 512)
        made.append(vm)

        def refused(code, word, cc, kk, dev=False):
            args = [torch.from_numpy(x).cuda() for x in (cc, kk, a)] if dev else (cc, kk, a)
            _refused(code, word, vm.restore, *args)
            i = vm.info()
            assert (i["n_voxels"], i["n_members"]) == (0, 0) and vm.fetch(M.COORDS).shape == (0, 3)
            g = vm.register(s, sn, K.GUESS)
            assert g["n_corr"] == 0 and not g["valid"]

        dup = c.copy()
        dup[n - 1] = dup[3]
        refused(ql.QTR_ERR_BAD_ARG, "twice", dup, k)
        for bad in (0, -1):
            kk = k.copy()
            kk[n // 2] = bad
            refused(ql.QTR_ERR_BAD_ARG, "count", c, kk, dev=bad == 0)
        for ax, bad in ((0, K.HI + 1), (1, K.LO - 1), (2, (1 << 31) - 1)):
            cc = c.copy()
            cc[5, ax] = bad
            refused(ql.QTR_ERR_BAD_ARG, "coordinate", cc, k, dev=ax == 1)
        small = hip.voxel_map(K.SIDE, 64)
        made.append(small)
        _refused(ql.QTR_ERR_CAPACITY, "capacity=64", small.restore, c, k, a)
        assert len(small) == 0
        small.restore(c[:64], k[:64], a[:64])     # n = capacity fits
        assert len(small) == 64 and np.array_equal(small.fetch(M.COORDS), c[:64])
        _refused(ql.QTR_ERR_BAD_ARG, "holds 64 voxels", small.restore, c[:3], k[:3], a[:3])   # a map that holds voxels
        assert len(small) == 64
        vm.restore(c, k, a)                       # after all its refusals the map takes the voxels
        _same_sections(_sections(vm), f, "after the refusals")
        vm.clear()
        vm.restore(c[:0], k[:0], a[:0])           # no voxel is not an error
        assert len(vm) == 0
    finally:
        for m in made:
            m.destroy()


def test_save_and_load_round_trip(hip, hand, hand_sections, tmp_path):
    _, s, sn = hand
    vm, ref = _hand_maps(hip, hand)
    back = other = None
    try:
        path = str(tmp_path / "map.npz")
        vm.save(path)
        back = hip.load_voxel_map(path)
        assert back.info()["capacity"] == 4096 and back.info()["voxel_size"] == K.SIDE
        _same_map(back, vm, "loaded", inserts=False)
        other = hip.load_voxel_map(path, capacity=300)
        assert other.info()["capacity"] == 300
        _same_sections(_sections(other), hand_sections, "loaded into another capacity")
        _register_both(hip, other, ref, s, sn, K.GUESS, 4, "the loaded map")
    finally:
        for m in (vm, back, other):
            if m is not None:
                m.destroy()


def test_the_same_bits_twice_and_two_maps_on_one_handle(hip, hand, hand_sections):
    a, ref = _hand_maps(hip, hand)
    b, _ = _hand_maps(hip, hand)
    c = hip.voxel_map(K.SIDE, 1024)
    try:
        assert a.evict(CENTRE, RADIUS) == ref.evict(CENTRE, RADIUS)
        _same_sections(_sections(b), hand_sections, "the other map while one was evicted")
        c.restore(hand_sections[M.COORDS], hand_sections[M.COUNT], hand_sections[M.SUMS], slot=1)
        _same_sections(_sections(b), hand_sections, "the other map while one was restored")
        _same_map(a, ref, "the evicted map while one was restored")
        assert b.evict(CENTRE, RADIUS, slot=1) == c.evict(CENTRE, RADIUS) == {"n_kept": 19, "n_evicted": 257,
                                                                             "n_members_evicted": 681 - ref.info()["n_members"]}
        _same_map(b, a, "twice")
        _same_map(c, a, "restored, then evicted", inserts=False)
    finally:
        for m in (a, b, c):
            m.destroy()


ODOMETRY_RADIUS = 25.0
ODOMETRY_CAPACITY = 1950  # (between the restatement's two sizes: see the docstring below)


def test_windowed_scan_to_map_odometry(hip):
    """scan_to_map_odometry(window_radius=25) on kitti64_trajectory(0)'s first six scans against the restatement driven with the
    fetched keyframe clouds, with a capacity only the windowed map fits into.  The restatement's sizes on these clouds
    (1 m voxels): the windowed map holds at most 1786 voxels, right after the sixth insert (1688, 1730, 1744, 1776, 1773,
    1786 after the six; 391 once the last eviction is done), the unwindowed map ends with 2122; the capacity, 1950, lies between
    them, and the test holds it to the sizes the restatement gives when it runs."""
    from quatro_amd import api, synth
    from quatro_amd import lib as ql
    scans, _ = synth.kitti64_trajectory(0, n_scans=6)
    scans = scans[:6]
    fp = ql.default_frontend_params()
    kfs = [hip.keyframe(s, fp) for s in scans]
    maps = []
    try:
        clouds, normals = [k.fetch(ql.KF_VOX) for k in kfs], [k.fetch(ql.KF_NORMALS) for k in kfs]
        want_w, ref_w, results_w, sizes_w = KR.odometry(clouds, normals, 1.0, 1 << 16, window_radius=ODOMETRY_RADIUS)
        want_0, ref_0, results_0 = M.odometry(clouds, normals, 1.0, 1 << 16)   # the restatement as it was: no window
        print(f"windowed odometry (restatement): sizes after each insert {sizes_w}, after the last eviction {len(ref_w)}; "
              f"unwindowed final size {len(ref_0)}")
        cap = ODOMETRY_CAPACITY
        assert max(sizes_w) < cap < len(ref_0), (sizes_w, cap, len(ref_0))
        poses, vm = api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, capacity=cap, window_radius=ODOMETRY_RADIUS)
        maps.append(vm)
        assert np.array_equal(_bits(poses), _bits(want_w))
        _same_map(vm, ref_w, "the windowed odometry's map")
        assert all(r["valid"] for r in results_w)
        with pytest.raises(ql.QuatroHipError) as ei:   # the same capacity without the window
            api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, capacity=cap)
        assert ei.value.code == ql.QTR_ERR_CAPACITY, str(ei.value)
        # window_radius=None is what it was: the unchanged restatement's poses and map
        poses, vm = api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, capacity=1 << 16, window_radius=None)
        maps.append(vm)
        assert np.array_equal(_bits(poses), _bits(want_0))
        _same_map(vm, ref_0, "window_radius=None")
    finally:
        for m in maps:
            m.destroy()
        for k in kfs:
            k.close()


def test_cpp_voxelmap_keep_demo_prints_what_the_python_calls_return(hip, hand, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "voxelmap_keep_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "voxelmap_keep_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath),
                           "-Wl,-rpath,/opt/rocm/lib"])
    p, n, pose = hand[0][1]
    args = [repr(K.SIDE)]
    for name, a in (("a", p), ("an", n), ("pa", pose)):
        path = str(tmp_path / name)
        if a.shape == (4, 4):
            np.savetxt(path, a, fmt="%.17g")
        else:
            synth.save_kitti_bin(path, a)
        args.append(path)
    args += [repr(float(x)) for x in CENTRE] + [repr(RADIUS), "32"]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    vm = hip.voxel_map(K.SIDE, 1 << 16)
    copy = hip.voxel_map(K.SIDE, 32)
    try:
        vm.insert(p, n, pose)
        i0 = vm.info()
        e = vm.evict(CENTRE, RADIUS)
        i1 = vm.info()
        copy.restore(vm.fetch(M.COORDS), vm.fetch(M.COUNT), vm.fetch(M.SUMS))
        i2 = copy.info()
        assert 0 < e["n_kept"] <= 32 and e["n_evicted"] > 0

        def line(what, i):
            return f"{what}: voxels {i['n_voxels']} members {i['n_members']} inserts {i['n_inserts']}"
        assert out[0] == line("map", i0), out[0]
        assert out[1] == f"evict: kept {e['n_kept']} evicted {e['n_evicted']} members {e['n_members_evicted']}", out[1]
        assert out[2] == line("window", i1) and out[3] == line("copy", i2), out[2:4]
        x = np.bitwise_xor.reduce(copy.fetch(M.SUMS).reshape(-1).view(np.uint64))
        assert out[4] == f"sums {int(x):016x} cloud {i2['n_voxels']}", out[4]
    finally:
        vm.destroy()
        copy.destroy()
