"""Visibility carving of the voxel map on the MI355X (qtr_voxel_map_carve / qtr_voxel_map_carve_keyframes,
libquatro_ext.so): all five fetch sections and the info bit-equal to the numpy restatement
(tests/vmap_carve_restate.py) over map sizes, capacities, cloud sizes, numbers of keyframes, image sizes and windows, from
host and device memory; the same call twice; inserts and registrations after a carve; the refusals; build_map(carve=) and
scan_to_map_odometry(carve=); and the C++ demo.  Everything goes through the C ABI (quatro_amd.lib)."""
import os
import subprocess

import numpy as np
import pytest

import icp_restate as R
import vmap_carve_cases as CC
import vmap_carve_restate as CR
import vmap_cases as K
import vmap_restate as M

pytestmark = pytest.mark.gpu

SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)
ZERO = {"n_kept": 0, "n_carved": 0, "n_tested": 0, "n_members_carved": 0}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _sections(m):
    return m.fetch_all() if isinstance(m, M.RefMap) else {k: m.fetch(k) for k in SECTIONS}


def _same_sections(fa, fb, what=""):
    for k in SECTIONS:
        assert fa[k].shape == fb[k].shape and np.array_equal(_bits(fa[k]), _bits(fb[k])), (what, k)


def _same_map(a, b, what=""):
    _same_sections(_sections(a), _sections(b), what)
    ia, ib = a.info(), b.info()
    assert all(ia[k] == ib[k] for k in ("n_voxels", "n_inserts", "n_members")), (what, ia, ib)


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


@pytest.fixture(scope="module")
def hand_scans(hand):
    """The hand-built map's sections (restatement) and three shell scans of it with their poses (computed once, read only)."""
    ref = CR.RefMap(K.SIDE, 4096)
    for c in hand[0]:
        ref.insert(*c)
    f = ref.fetch_all()
    clouds, poses = CC.hand_scans(f[M.CLOUD], n_scans=3)
    for v in list(f.values()) + clouds + [poses]:
        v.setflags(write=False)
    return f, clouds, poses


def _hand_maps(hip, hand, capacity=4096):
    vm, ref = hip.voxel_map(K.SIDE, capacity), CR.RefMap(K.SIDE, capacity)
    for p, n, pose in hand[0]:
        assert vm.insert(p, n, pose) == ref.insert(p, n, pose)
    return vm, ref


CLOUD_CASES = [(0, 0, CC.WIDE, False), (1, 1, CC.WIDE, True), (63, 2, CC.WIDE, False), (64, 3, CC.WIDE, True), (65, 0, CC.WIDE, False),
               (257, 1, CC.WIDE, True), (1000, 2, CC.WIDE, False), (1512, 0, CC.TINY, True), (1512, 1, CC.TINY, False),
               (1512, 2, CC.TINY, True), (1512, 3, CC.TINY, False), (1512, 3, CC.WIDE, True), (1512, 2, {}, False)]


@pytest.mark.parametrize("n,window,image,device", CLOUD_CASES)
def test_one_cloud_is_bit_equal_to_the_restatement(hip, hand, hand_scans, n, window, image, device):
    import torch
    f, clouds, poses = hand_scans
    vm, ref = _hand_maps(hip, hand)
    try:
        p = CR.Params(**image, window=window, margin_abs=0.4)
        cloud = np.array(clouds[0][:n])
        got = vm.carve(torch.from_numpy(cloud).cuda() if device else cloud, poses[0], p.to_lib(), slot=1 if device else 0)
        want = ref.carve(cloud, poses[0], p)
        print(f"n={n} window={window} image={p.rows}x{p.cols}: {got}")
        assert got == want and got["n_kept"] + got["n_carved"] == 276
        _same_map(vm, ref, "after the carve")
        _same_sections(_sections(vm), {k: f[k][np.isin(_keys(f[M.COORDS]), _keys(vm.fetch(M.COORDS)))] for k in SECTIONS},
                       "the kept rows of the sections before")
        again = vm.carve(cloud, poses[0], p.to_lib())      # the same call again: nothing left to carve, the table untouched
        assert again == ref.carve(cloud, poses[0], p) and again["n_carved"] == 0 and again["n_kept"] == got["n_kept"]
        _same_map(vm, ref, "after the second call")
    finally:
        vm.destroy()


def _keys(coords):
    c = np.asarray(coords, np.int64)
    return ((c[:, 2] + (1 << 20)) << 42) + ((c[:, 1] + (1 << 20)) << 21) + (c[:, 0] + (1 << 20))


@pytest.mark.parametrize("n_voxels,capacity", [(0, 64), (1, 64), (60, 64), (255, 4096), (256, 4096), (257, 4096), (5000, None)])
def test_map_sizes_and_capacities(hip, n_voxels, capacity):
    """Maps of 0 .. 5000 voxels in tables of 128 slots, 8192 slots and the default 2^21, carved with a raster scan of the
    default image (a return in four of five pixels, on a smooth surface that lies behind part of the voxels)."""
    cap = capacity or (1 << 20)
    vm, ref = hip.voxel_map(0.5, cap), CR.RefMap(0.5, cap)
    try:
        if n_voxels:
            pts, nrm = CC.random_map_cloud(n_voxels, 0.5, seed=n_voxels)
            assert vm.insert(pts, nrm) == ref.insert(pts, nrm)
        assert len(vm) == n_voxels
        p = CR.Params(min_votes=1, window=2 if n_voxels != 256 else 3)
        scan = CC.raster_scan(p, seed=n_voxels + 1, r_lo=2.0, r_hi=30.0, smooth=True)
        P = R.rigid(R.rot(0.0, 0.0, 0.3), [0.2, -0.1, 0.05])
        got, want = vm.carve(scan, P, p.to_lib()), ref.carve(scan, P, p)
        print(f"{n_voxels} voxels, capacity {cap}: {got}")
        assert got == want
        if n_voxels >= 60:
            assert n_voxels // 10 < got["n_carved"] < n_voxels - n_voxels // 10 and got["n_tested"] > n_voxels // 2
        _same_map(vm, ref, n_voxels)
        if n_voxels:   # the rebuilt table takes an insert like any other: kept voxels, carved ones and three new ones
            new, new_n = CC.random_map_cloud(3, 0.5, seed=n_voxels + 7)
            more, more_n = np.concatenate([pts[:40], new]), np.concatenate([nrm[:40], new_n])
            assert vm.insert(more, more_n) == ref.insert(more, more_n)
            _same_map(vm, ref, "the insert that follows")
    finally:
        vm.destroy()


def test_inserts_and_registrations_after_a_carve(hip, hand, hand_scans):
    from quatro_amd import lib as ql
    f, clouds, poses = hand_scans
    _, s, sn = hand
    vm, ref = _hand_maps(hip, hand)
    whole, _ = _hand_maps(hip, hand)
    copy = hip.voxel_map(K.SIDE, 1024)
    try:
        p = CR.Params(**CC.WIDE, window=1, min_votes=2)
        got = vm.carve_keyframes([], np.zeros((0, 4, 4)), p.to_lib())
        assert got == ZERO
        # (keyframes are covered below; here the three scans vote one cloud at a time with min_votes = 1)
        p1 = CR.Params(**CC.WIDE, window=1)
        for b in (0, 1):
            assert vm.carve(clouds[b], poses[b], p1.to_lib()) == ref.carve(clouds[b], poses[b], p1)
        _same_map(vm, ref, "two carves")
        kept = {tuple(c) for c in vm.fetch(M.COORDS)}
        assert 0 < len(kept) < 276
        # an insert continues kept voxels exactly as on an uncarved copy; a carved voxel that is touched again starts anew
        more, more_n = K.cloud_of_voxels(f[M.COORDS][::5], K.SIDE, per_voxel=(2,), seed=5)
        alone = CR.RefMap(K.SIDE, 4096)
        alone.insert(more, more_n)
        assert vm.insert(more, more_n) == ref.insert(more, more_n)
        whole.insert(more, more_n)
        _same_map(vm, ref, "the insert after the carves")
        fw, fa, fm = _sections(whole), alone.fetch_all(), _sections(vm)
        iw = {tuple(c): j for j, c in enumerate(fw[M.COORDS])}
        ia = {tuple(c): j for j, c in enumerate(fa[M.COORDS])}
        n_cont = n_new = 0
        for j, c in enumerate(map(tuple, fm[M.COORDS])):
            src, row = (fw, iw[c]) if c in kept else (fa, ia[c])
            for k in SECTIONS:
                assert np.array_equal(_bits(fm[k][j]), _bits(src[k][row])), (c, k)
            n_cont += c in kept and c in ia
            n_new += c not in kept
        assert n_cont > 0 and n_new > 0
        # a registration against the carved map equals one against a restored copy of its sections
        copy.restore(fm[M.COORDS], fm[M.COUNT], fm[M.SUMS])
        prm = ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, max_iterations=6, transformation_epsilon=0.0,
                                    euclidean_fitness_epsilon=0.0)
        a = vm.register(s, sn, K.GUESS, prm)
        ta = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).copy()
        b = copy.register(s, sn, K.GUESS, prm)
        tb = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64)
        o = ref.register(s, sn, K.GUESS, teps=0.0, feps=0.0, max_iter=6)
        assert a["n_corr"] > 10 and a["iterations"] == 6
        assert np.array_equal(_bits(a["T"]), _bits(b["T"])) and np.array_equal(_bits(a["T"]), _bits(o["T"]))
        assert np.array_equal(_bits(ta), _bits(tb)) and a["n_corr"] == b["n_corr"] == o["n_corr"]
    finally:
        for m in (vm, whole, copy):
            m.destroy()


def test_named_edge_cases_on_the_device(hip):
    """vmap_carve_cases.edge_clouds: the limit and one float above it, az = pi folded to column 0, the window across the column
    wrap and clamped at the first and the last row, an empty centre, returns without a pixel — the expected verdict, and the
    restatement's bits."""
    p = CR.Params(**CC.EDGE_IMAGE)
    up = np.zeros((1, 4), np.float32)
    up[0, 2] = 1.0
    for name, pts, scan, carved in CC.edge_clouds():
        vm, ref = hip.voxel_map(0.5, 64), CR.RefMap(0.5, 64)
        try:
            assert vm.insert(pts, up) == ref.insert(pts, up) and len(vm) == 1
            assert np.array_equal(vm.fetch(M.RECORDS)[0, :3], pts[0, :3].astype(np.float64)), name   # the mean is the member
            got = vm.carve(scan, None, p.to_lib())
            assert got == ref.carve(scan, None, p), name
            assert got["n_carved"] == int(carved) and got["n_kept"] == 1 - int(carved), (name, got)
            assert got["n_tested"] == (0 if name in ("empty", "skipped") else 1), (name, got)
            _same_map(vm, ref, name)
        finally:
            vm.destroy()


@pytest.mark.parametrize("far", [(), (0,), (0, 1, 2)])
def test_three_voxels_in_128_slots_through_every_end_of_the_rebuild(hip, far):
    """The smallest map that takes each path behind the mark pass: nothing carved (the table is only read), exactly one
    voxel carved (stage, clear, put) and all carved (clear alone).  Three voxels of one member each, 5 m from the sensor in
    the middle of pixels that are five columns apart (EDGE_IMAGE: limit 7.5 m); the scan's return on a voxel's ray lies at
    6 m (occupied: kept) or at 40 m (seen through: carved)."""
    def ray(az_deg, r):
        e, a = np.deg2rad(-5.0), np.deg2rad(az_deg)
        return [r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e)]
    az = (11.0, 124.0, -124.0)
    pts = R.f4(np.array([ray(a, 5.0) for a in az], np.float32))
    scan = R.f4(np.array([ray(a, 40.0 if j in far else 6.0) for j, a in enumerate(az)], np.float32))
    up = np.zeros((3, 4), np.float32)
    up[:, 2] = 1.0
    p = CR.Params(**CC.EDGE_IMAGE)
    assert M.table_slots(64) == 128
    vm, ref = hip.voxel_map(0.5, 64), CR.RefMap(0.5, 64)
    try:
        assert vm.insert(pts, up) == ref.insert(pts, up) and len(vm) == 3
        before = _sections(vm)
        got = vm.carve(scan, None, p.to_lib())
        assert got == ref.carve(scan, None, p), far
        assert (got["n_kept"], got["n_carved"], got["n_tested"], got["n_members_carved"]) == (3 - len(far), len(far), 3, len(far))
        _same_map(vm, ref, far)
        gone = _keys(np.floor(pts[list(far), :3].astype(np.float64) / 0.5).reshape(-1, 3))
        keep = ~np.isin(_keys(before[M.COORDS]), gone)
        assert keep.sum() == 3 - len(far)
        _same_sections(_sections(vm), {k: before[k][keep] for k in SECTIONS}, "the rows that stay")
        assert vm.insert(pts, up) == ref.insert(pts, up)
        _same_map(vm, ref, "an insert after it")
    finally:
        vm.destroy()


def test_refusals_leave_the_map_as_it_was(hip, hand, hand_scans, trajectory):
    import ctypes
    from quatro_amd import lib as ql
    f, clouds, poses = hand_scans
    kfs, kf_clouds, _, kf_poses, _ = trajectory
    vm, ref = _hand_maps(hip, hand)
    other = ql.Handle(0)
    closed = foreign_kf = foreign_map = None
    try:
        cloud = clouds[0]
        for name, value, _ in CC.BAD_PARAMS:
            prm = ql.default_carve_params()
            setattr(prm, name, value if name != "min_votes" or value == 0 else 2)   # (one cloud: one scan)
            _refused(ql.QTR_ERR_BAD_ARG, "carve", vm.carve, cloud, poses[0], prm)
        bad = np.array(poses[0])
        for rc in ((0, 0), (1, 3), (2, 2)):
            for v in (np.nan, np.inf):
                b = bad.copy()
                b[rc] = v
                _refused(ql.QTR_ERR_BAD_ARG, "pose", vm.carve, cloud, b, CR.Params(**CC.WIDE).to_lib())
        _refused(ql.QTR_ERR_BAD_ARG, "slot", vm.carve, cloud, poses[0], None, slot=9)
        _refused(ql.QTR_ERR_CAPACITY, "max_points", vm.carve, np.zeros((hip.limits.max_points + 1, 4), np.float32), poses[0])
        _refused(ql.QTR_ERR_BAD_ARG, "min_votes", vm.carve_keyframes, [], np.zeros((0, 4, 4)), ql.default_carve_params(min_votes=65))
        # owners: a map and a keyframe of another handle, a closed (NULL) keyframe, alone and among good ones
        wide = CR.Params(**CC.WIDE).to_lib()
        foreign_map = other.voxel_map(K.SIDE, 64)
        stolen = ql.VoxelMap(hip, foreign_map._m.value)   # the other handle's map through this handle
        _refused(ql.QTR_ERR_BAD_ARG, "another handle", stolen.carve, cloud, poses[0], wide)
        _refused(ql.QTR_ERR_BAD_ARG, "another handle", stolen.carve_keyframes, kfs[:2], kf_poses[:2], wide)
        stolen._m = None                                  # (not this wrapper's to destroy)
        foreign_kf = other.keyframe(kf_clouds[0])
        closed = hip.keyframe(kf_clouds[0])
        closed.close()
        _refused(ql.QTR_ERR_BAD_ARG, "another handle", vm.carve_keyframes, [foreign_kf], kf_poses[:1], wide)
        _refused(ql.QTR_ERR_BAD_ARG, "another handle", vm.carve_keyframes, [kfs[0], kfs[1], foreign_kf], kf_poses[:3], wide)
        _refused(ql.QTR_ERR_BAD_ARG, "keyframe is NULL", vm.carve_keyframes, [closed], kf_poses[:1], wide)
        _refused(ql.QTR_ERR_BAD_ARG, "keyframe is NULL", vm.carve_keyframes, [kfs[0], closed, kfs[2]], kf_poses[:3], wide)
        # a non-finite pose among several on the keyframe entry: the first, a middle and the last one
        for k in (0, 2, 5):
            for rc, v in (((0, 1), np.nan), ((2, 3), np.inf), ((1, 1), -np.inf)):
                b = kf_poses.copy()
                b[k][rc] = v
                _refused(ql.QTR_ERR_BAD_ARG, f"pose {k}", vm.carve_keyframes, kfs, b, wide)
        # what the Python layer never passes, through the C ABI itself: NULL arrays with a count, a memory kind that is none
        clib, info = ql.load_ext(), ql.VoxelMapCarveInfo()
        arr = (ctypes.c_void_p * 2)(kfs[0]._kf.value, kfs[1]._kf.value)
        P2 = np.ascontiguousarray(kf_poses[:2])
        c0 = np.array(cloud)
        calls = (("NULL cloud", lambda: clib.qtr_voxel_map_carve(hip._h, 0, vm._m, None, 5, None, wide, ql.MEM_HOST, ctypes.byref(info))),
                 ("mem=7", lambda: clib.qtr_voxel_map_carve(hip._h, 0, vm._m, c0.ctypes.data, 5, None, wide, 7, ctypes.byref(info))),
                 ("n=-1", lambda: clib.qtr_voxel_map_carve(hip._h, 0, vm._m, c0.ctypes.data, -1, None, wide, ql.MEM_HOST, ctypes.byref(info))),
                 ("n_kf=2", lambda: clib.qtr_voxel_map_carve_keyframes(hip._h, 0, vm._m, None, P2.ctypes.data, 2, wide, ctypes.byref(info))),
                 ("n_kf=2", lambda: clib.qtr_voxel_map_carve_keyframes(hip._h, 0, vm._m, arr, None, 2, wide, ctypes.byref(info))),
                 ("n_kf=-1", lambda: clib.qtr_voxel_map_carve_keyframes(hip._h, 0, vm._m, arr, P2.ctypes.data, -1, wide, ctypes.byref(info))),
                 ("voxel map is NULL", lambda: clib.qtr_voxel_map_carve(hip._h, 0, None, c0.ctypes.data, 5, None, wide, ql.MEM_HOST, ctypes.byref(info))),
                 ("voxel map is NULL", lambda: clib.qtr_voxel_map_carve_keyframes(hip._h, 0, None, arr, P2.ctypes.data, 2, wide, ctypes.byref(info))))
        for word, call in calls:
            assert call() == ql.QTR_ERR_BAD_ARG and word in hip.last_error(), (word, hip.last_error())
            assert (info.n_kept, info.n_carved, info.n_tested, info.n_members_carved) == (0, 0, 0, 0)
        _same_sections(_sections(vm), f, "after every refusal")
        assert vm.info()["n_inserts"] == 3 and vm.info()["n_members"] == int(f[M.COUNT].sum())
        ok = CR.Params(**CC.WIDE)
        assert vm.carve(cloud, poses[0], ok.to_lib()) == ref.carve(cloud, poses[0], ok)     # and the map still works
        _same_map(vm, ref, "a carve after the refusals")
    finally:
        vm.destroy()
        for x in (foreign_kf, foreign_map):
            if x is not None:
                x.close()
        other.close()


@pytest.fixture(scope="module")
def trajectory(hip):
    """Six keyframes of kitti64_trajectory(0) with their fetched voxels, normals and ground-truth poses."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    scans, poses = synth.kitti64_trajectory(0, n_scans=6)
    fp = ql.default_frontend_params()
    kfs = [hip.keyframe(s, fp) for s in scans[:6]]
    clouds, normals = [k.fetch(ql.KF_VOX) for k in kfs], [k.fetch(ql.KF_NORMALS) for k in kfs]
    yield kfs, clouds, normals, np.array(poses[:6]), fp
    for k in kfs:
        k.close()


# (the scans of the trajectory have their ground removed, so the default rule carves little of them; a window of 0 and a
# margin of 0.2 m carve plenty, which is what a parity test wants)
GREEDY = dict(window=0, margin_abs=0.2)


@pytest.mark.parametrize("B,min_votes", [(1, 1), (2, 2), (64, 1), (64, 20)])
def test_keyframes_vote_as_in_the_restatement(hip, trajectory, B, min_votes):
    kfs, clouds, normals, poses, _ = trajectory
    from quatro_amd import api
    from quatro_amd import lib as ql
    vm, ref = api.build_map(hip, kfs, poses, voxel_size=1.0), CR.build_map(clouds, normals, poses, 1.0)
    try:
        _same_map(vm, ref, "carve=None is the map it was")
        idx = [b % 6 for b in range(B)]
        P = np.stack([poses[i] @ R.rigid(R.rot(0.0, 0.0, 0.002 * (b // 6)), [0.01 * (b // 6), 0.0, 0.0]) for b, i in enumerate(idx)])
        p = CR.Params(**GREEDY, min_votes=min_votes)
        got = vm.carve_keyframes([kfs[i] for i in idx], P, p.to_lib(), slot=B % 2)
        want = ref.carve_scans([clouds[i] for i in idx], P, p)
        print(f"B={B} min_votes={min_votes}: {got}")
        assert got == want and got["n_carved"] > 0 and got["n_kept"] > 0
        _same_map(vm, ref, (B, min_votes))
        if B == 2:
            _refused(ql.QTR_ERR_BAD_ARG, "min_votes", vm.carve_keyframes, kfs[:2], poses[:2], CR.Params(min_votes=3).to_lib())
            _refused(ql.QTR_ERR_BAD_ARG, "n_kf=65", vm.carve_keyframes, [kfs[0]] * 65, np.stack([poses[0]] * 65), p.to_lib())
            _same_map(vm, ref, "after the refusals")
    finally:
        vm.destroy()


def test_votes_reached_exactly_missed_by_one_and_split_between_scans(hip, trajectory):
    """Three keyframes vote on the map of all six.  Voxel by voxel: one with exactly min_votes votes leaves and one with
    min_votes - 1 stays, for min_votes 1, 2 and 3; a voxel seen through by one scan and occupied in another has one vote,
    which min_votes = 1 takes and min_votes = 2 does not."""
    from quatro_amd import api
    kfs, clouds, normals, poses, _ = trajectory
    three = [0, 2, 4]
    f = CR.build_map(clouds, normals, poses, 1.0).fetch_all()
    c = CR.cfg_make(CR.Params(**GREEDY), 3, 1.0)
    votes = CR.carve_votes(c, [clouds[i] for i in three], poses[three], f[M.RECORDS][:, :3])
    through = (votes == CR.SEEN_THROUGH).sum(axis=1)
    split = (through == 1) & (votes == CR.OCCUPIED).any(axis=1)
    print(f"voxels by votes {np.bincount(through, minlength=4)}, seen through once and occupied elsewhere {int(split.sum())}")
    assert all((through == k).sum() > 0 for k in (0, 1, 2)) and split.sum() > 0
    keys = _keys(f[M.COORDS])
    for min_votes in (1, 2, 3):
        vm = api.build_map(hip, kfs, poses, voxel_size=1.0)
        try:
            got = vm.carve_keyframes([kfs[i] for i in three], poses[three], CR.Params(**GREEDY, min_votes=min_votes).to_lib())
            left = np.isin(keys, _keys(vm.fetch(M.COORDS)))
            assert not left[through == min_votes].any() and left[through == min_votes - 1].all(), min_votes
            assert np.array_equal(left, through < min_votes) and got["n_carved"] == int((through >= min_votes).sum())
            assert bool(left[split].all()) == (min_votes > 1) and bool(left[split].any()) == (min_votes > 1)
        finally:
            vm.destroy()


def test_build_map_and_odometry_with_carving(hip, trajectory):
    from quatro_amd import api
    kfs, clouds, normals, poses, fp = trajectory
    maps = []
    try:
        p = CR.Params(**GREEDY, min_votes=2)
        vm = api.build_map(hip, kfs, poses, voxel_size=1.0, carve=p.to_lib())
        maps.append(vm)
        ref = CR.build_map(clouds, normals, poses, 1.0, carve=p)
        plain = CR.build_map(clouds, normals, poses, 1.0)
        print(f"build_map: {len(plain)} voxels, {len(ref)} after the carve")
        assert 0 < len(ref) < len(plain)
        _same_map(vm, ref, "build_map(carve=)")
        with pytest.raises(ValueError):
            api.build_map(hip, kfs, poses, voxel_size=1.0, carve=CR.Params(min_votes=7).to_lib())
        with pytest.raises(ValueError):   # one scan votes per carve: refused before a keyframe or a map is made
            api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, carve=p.to_lib())
        p1 = CR.Params(**GREEDY)
        got, vm = api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, capacity=1 << 16, window_radius=40.0, carve=p1.to_lib())
        maps.append(vm)
        want, ref, results, carved = CR.odometry(clouds, normals, 1.0, 1 << 16, window_radius=40.0, carve=p1)
        print(f"odometry: carved per scan {[c['n_carved'] for c in carved]}")
        assert sum(c["n_carved"] for c in carved) > 0 and all(r["valid"] for r in results)
        assert np.array_equal(_bits(got), _bits(want))
        _same_map(vm, ref, "scan_to_map_odometry(carve=)")
        got0, vm0 = api.scan_to_map_odometry(hip, kfs, fp, voxel_size=1.0, capacity=1 << 16, carve=None)
        maps.append(vm0)
        want0, ref0, _ = M.odometry(clouds, normals, 1.0, 1 << 16)      # the restatement as it was
        assert np.array_equal(_bits(got0), _bits(want0))
        _same_map(vm0, ref0, "carve=None")
    finally:
        for m in maps:
            m.destroy()


def test_cpp_voxelmap_carve_demo_prints_what_the_python_calls_return(hip, hand, hand_scans, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "voxelmap_carve_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "voxelmap_carve_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath),
                           "-Wl,-rpath,/opt/rocm/lib"])
    _, clouds, poses = hand_scans
    p, n, pose = hand[0][1]
    scan = np.ascontiguousarray(clouds[1][np.isfinite(clouds[1]).all(axis=1)])
    args = [repr(K.SIDE)]
    for name, a in (("a", p), ("an", n), ("pa", pose), ("s", scan), ("ps", poses[1])):
        path = str(tmp_path / name)
        if a.shape == (4, 4):
            np.savetxt(path, a, fmt="%.17g")
        else:
            synth.save_kitti_bin(path, a)
        args.append(path)
    prm = CR.Params(rows=16, cols=64, fov_up_deg=75.0, fov_down_deg=-75.0, window=1, min_range=0.5)
    args += [str(prm.rows), str(prm.cols), repr(prm.fov_up_deg), repr(prm.fov_down_deg), str(prm.window)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    vm = hip.voxel_map(K.SIDE, 1 << 16)
    try:
        vm.insert(p, n, pose)
        i0 = vm.info()
        c = vm.carve(scan, poses[1], prm.to_lib())
        i1 = vm.info()
        assert c["n_carved"] > 0 and c["n_kept"] > 0

        def line(what, i):
            return f"{what}: voxels {i['n_voxels']} members {i['n_members']} inserts {i['n_inserts']}"
        assert out[0] == line("map", i0), out[0]
        assert out[1] == f"carve: kept {c['n_kept']} carved {c['n_carved']} tested {c['n_tested']} members {c['n_members_carved']}", out[1]
        assert out[2] == line("carved", i1), out[2]
        x = np.bitwise_xor.reduce(vm.fetch(M.SUMS).reshape(-1).view(np.uint64))
        assert out[3] == f"sums {int(x):016x} cloud {i1['n_voxels']}", out[3]
    finally:
        vm.destroy()
