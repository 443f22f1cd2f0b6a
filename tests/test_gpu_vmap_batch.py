"""The grouped map registration on the MI355X (qtr_voxel_map_register_batch, libquatro_ext.so): every item of every
named case bit-equal to the single call's restatement (vmap_restate.RefMap.register) and to the single calls on the same
slot, the group shapes, the blocked loop, repeatability and what a batch must leave untouched, relocalisation on top of it,
the refusals and the C++ demo.  Everything goes through the C ABI (quatro_amd.lib)."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import icp_restate as R
import vmap_batch_cases as BC
import vmap_restate as M

pytestmark = pytest.mark.gpu

ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")
SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


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


def _sections(vm):
    return {k: vm.fetch(k) for k in SECTIONS}


def _same_sections(a, b, what=""):
    assert all(a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])) for k in SECTIONS), what


def _prm(**kw):
    from quatro_amd import lib as ql
    return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)


def _fetched(vm, n_items, slot=0):
    from quatro_amd import lib as ql
    return [(vm.batch_fetch(i, ql.VMAP_BATCH_TRACE, slot), vm.batch_fetch(i, ql.VMAP_BATCH_CORR, slot)) for i in range(n_items)]


def _batch_against_ref(vm, ref, items, what, ref_items=None, slot=0, **icp):
    """One batch on the device against the restatement of every item alone: the record, the whole trace and the corr flags,
    bit for bit.  icp: RefMap.register's keywords (teps, feps, max_iter).  ref_items: the items as clouds where `items`
    holds keyframes or device tensors.  Returns (results, [(trace, corr)])."""
    names = {"teps": "transformation_epsilon", "feps": "euclidean_fitness_epsilon", "max_iter": "max_iterations"}
    got = vm.register_batch(items, _prm(**{names[k]: v for k, v in icp.items()}), slot)
    fetched = _fetched(vm, len(items), slot)
    assert len(got) == len(items)
    for i, (p, a, g) in enumerate(ref_items or items):
        o = ref.register(p, a, g, **icp)
        _same_icp(got[i], o, f"{what}, item {i}")
        trace, corr = fetched[i]
        assert trace.shape == o["trace"].shape and np.array_equal(_bits(trace), _bits(o["trace"])), (what, i)
        assert np.array_equal(corr, o["corr"]), (what, i)
    return got, fetched


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
def hand(hip):
    vm, ref = BC.hand_map(hip.voxel_map), BC.hand_map(M.RefMap)
    yield vm, ref
    vm.destroy()


@pytest.fixture(scope="module")
def room(hip):
    vm, ref = BC.room_map(hip.voxel_map), BC.room_map(M.RefMap)
    _, (q, qa), hyp = BC.room()
    yield vm, ref, q, qa, hyp
    vm.destroy()


@pytest.fixture(scope="module")
def traj(hip):
    """kitti64_trajectory(0, n_scans=6): keyframes of the six scans and of the revisit, their fetched clouds, the map and the
    place index of scans 0 - 5 under the scene's poses, and the restated map."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    scans, gt = synth.kitti64_trajectory(0, n_scans=6)
    fp = ql.default_frontend_params()
    kfs = [hip.keyframe(s, fp) for s in scans[:7]]
    clouds = [(k.fetch(ql.KF_VOX), k.fetch(ql.KF_NORMALS)) for k in kfs]
    vm, ref = hip.voxel_map(1.0, 1 << 16), M.RefMap(1.0, 1 << 16)
    index = hip.place_index(16)
    for k in range(6):
        vm.insert_keyframe(kfs[k], gt[k])
        ref.insert(clouds[k][0], clouds[k][1], gt[k])
        index.add(kfs[k])
    yield {"kfs": kfs, "clouds": clouds, "gt": np.asarray(gt), "vm": vm, "ref": ref, "index": index}
    index.close()
    vm.destroy()
    for k in kfs:
        k.close()


@pytest.mark.parametrize("case", sorted(BC.CASES) + ["room"])
def test_every_item_is_bit_equal_to_the_restatement_and_to_the_single_call(hip, hand, room, case):
    from quatro_amd import lib as ql
    if case == "room":
        vm, ref, q, qa, hyp = room
        items, icp = [(q, qa, g) for g in hyp], {}
    else:
        vm, ref = hand
        items, icp = BC.CASES[case]()
    for k in range(1, 9):  # the loop cut after k updates, as test_gpu_vmap's _register_both does for the single call
        _batch_against_ref(vm, ref, items, f"{case}, {k} iterations", teps=0.0, feps=0.0, max_iter=k)
    got, fetched = _batch_against_ref(vm, ref, items, f"{case}, defaults", **icp)
    print(f"{case}: iterations {[r['iterations'] for r in got]} stop {[r['stop_reason'] for r in got]} n_corr {[r['n_corr'] for r in got]}")
    # ... and the single calls on the same slot
    prm = _prm(transformation_epsilon=icp["teps"]) if icp else _prm()
    for i, (p, a, g) in enumerate(items):
        one = vm.register(p, a, g, prm)
        _same_icp(got[i], one, f"{case}, item {i}: the single call")
        assert np.array_equal(_bits(hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)), _bits(fetched[i][0])), (case, i)
        assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_CORR, np.int32), fetched[i][1]), (case, i)


def test_group_shapes_one_and_sixty_four(hip, hand):
    vm, ref = hand
    p, a = BC.plane_cloud(300, 31)
    _batch_against_ref(vm, ref, [(p, a, BC.small(3))], "B = 1")
    clouds = [BC.plane_cloud(n, 200 + j) for j, n in enumerate((120, 255, 256, 257, 300, 511, 513, 700))]
    items = [(c[0], c[1], BC.small(60 + g)) for c in clouds for g in range(8)]
    assert len(items) == 64
    got, _ = _batch_against_ref(vm, ref, items, "B = 64", max_iter=12)
    assert sum(r["valid"] for r in got) == 64


def test_keyframe_host_and_device_items_in_one_call(hip, traj):
    import torch
    vm, ref, kfs, clouds, gt = traj["vm"], traj["ref"], traj["kfs"], traj["clouds"], traj["gt"]
    off = [R.rigid(R.rot(0.004 * j, -0.003, 0.01 * j), [0.1 * j, -0.15, 0.02]) for j in range(6)]
    dev = [torch.from_numpy(x).cuda() for x in clouds[4]]
    items = [(kfs[1], gt[1] @ off[0]), (clouds[2][0], clouds[2][1], gt[2] @ off[1]), (dev[0], dev[1], gt[4] @ off[2]),
             (kfs[1], gt[1] @ off[3]), (dev[0], dev[1], gt[4] @ off[4]), (kfs[3], gt[3] @ off[5])]
    as_clouds = [clouds[k] + (items[i][-1],) for i, k in enumerate((1, 2, 4, 1, 4, 3))]
    got, _ = _batch_against_ref(vm, ref, items, "mixed items", ref_items=as_clouds, max_iter=10)
    assert all(r["valid"] and r["iterations"] >= 2 for r in got)
    # the single keyframe call on the same slot
    _same_icp(got[3], vm.register_keyframe(kfs[1], items[3][1], _prm(max_iterations=10)), "register_keyframe")


def test_sixty_five_items_are_a_batch_of_64_and_a_batch_of_1(hip, hand):
    from quatro_amd import lib as ql
    vm, ref = hand
    clouds = [BC.plane_cloud(200 + 13 * j, 300 + j) for j in range(5)]
    items = [(clouds[j % 5][0], clouds[j % 5][1], BC.small(400 + j)) for j in range(65)]
    prm = _prm(max_iterations=6)
    whole = vm.register_batch(items, prm)
    last_trace = vm.batch_fetch(0, ql.VMAP_BATCH_TRACE)
    with pytest.raises(ql.QuatroHipError):
        vm.batch_fetch(1, ql.VMAP_BATCH_TRACE)  # (the slot's last batch had one item)
    a = vm.register_batch(items[:64], prm)
    assert vm.batch_fetch(63, ql.VMAP_BATCH_CORR).shape[0] == items[63][0].shape[0]
    b = vm.register_batch(items[64:], prm)
    assert len(whole) == 65 and len(a) == 64 and len(b) == 1
    for i, (x, y) in enumerate(zip(whole, a + b)):
        _same_icp(x, y, f"item {i}")
    assert np.array_equal(_bits(last_trace), _bits(vm.batch_fetch(0, ql.VMAP_BATCH_TRACE)))
    _same_icp(whole[64], ref.register(*items[64], max_iter=6), "the 65th")


def _handle(n_slots, **env):
    """A handle created under these environment variables (the handle reads them once, when it is made)."""
    from quatro_amd import lib as ql
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ql.Handle(0, n_slots=n_slots)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_blocked_loop_equals_the_unblocked_loop(hip, hand):
    """QTR_ICP_BLOCK = 4 against all launches at once on the frozen case: 10 fixed updates are the blocks 4 + 4 + 2, the last
    one short; under transformation_epsilon = 1e-2 the first item stops inside the second block and the last one later
    (test_vmap_batch_cpu shows both with the restatement), so the host leaves the loop at a later read-back than the first
    stop."""
    vm, ref = hand
    items, icp = BC.CASES["frozen"]()
    blocked = _handle(1, QTR_ICP_BLOCK="4")
    bm = None
    try:
        bm = BC.hand_map(blocked.voxel_map)
        for kw in (dict(teps=0.0, feps=0.0, max_iter=10), dict(teps=1e-2, feps=0.0)):
            g0, f0 = _batch_against_ref(vm, ref, items, f"unblocked {kw}", **kw)
            g1, f1 = _batch_against_ref(bm, ref, items, f"blocked {kw}", **kw)
            print(f"{kw}: iterations {[r['iterations'] for r in g0]} / {[r['iterations'] for r in g1]}")
            for i in range(len(items)):
                _same_icp(g1[i], g0[i], f"{kw}, item {i}: blocked against unblocked")
                assert np.array_equal(_bits(f1[i][0]), _bits(f0[i][0])) and np.array_equal(f1[i][1], f0[i][1]), (kw, i)
        assert len({r["iterations"] for r in g0}) >= 3
    finally:
        if bm is not None:
            bm.destroy()
        blocked.close()


def test_repeatable_and_leaves_the_map_and_the_single_call_state_alone(hip, hand):
    from quatro_amd import lib as ql
    vm, ref = hand
    items, _ = BC.CASES["sizes"]()
    eight, _ = BC.CASES["one_cloud_eight_guesses"]()
    before = _sections(vm)
    info = vm.info()
    # a single call, a batch, and the slot's single-call debug sections are still the single call's
    p, a, g = eight[5]
    one = vm.register(p, a, g)
    trace1 = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    corr1 = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
    first = vm.register_batch(items)
    f_first = _fetched(vm, len(items))
    assert np.array_equal(_bits(hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)), _bits(trace1))
    assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_CORR, np.int32), corr1)
    assert trace1.shape[0] == one["iterations"] and corr1.shape[0] == 300
    _same_icp(vm.register(p, a, g), one, "the single call after the batch")
    # twice the same bits
    second = vm.register_batch(items)
    f_second = _fetched(vm, len(items))
    for i in range(len(items)):
        _same_icp(first[i], second[i], f"twice, item {i}")
        assert np.array_equal(_bits(f_first[i][0]), _bits(f_second[i][0])) and np.array_equal(f_first[i][1], f_second[i][1]), i
    times = vm.batch_fetch(0, ql.VMAP_BATCH_TIMES)
    assert times.shape == (2,) and times.dtype == np.float32 and np.all(times >= 0) and times[1] > 0
    # two slots batching against the one map from two threads: the sequential results
    want = [vm.register_batch(items, slot=0), vm.register_batch(eight, slot=0)]
    got, err = [None, None], []

    def work(k, its):
        try:
            for _ in range(3):
                got[k] = vm.register_batch(its, slot=k)
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(0, items)), threading.Thread(target=work, args=(1, eight))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k in range(2):
        for i, (x, y) in enumerate(zip(got[k], want[k])):
            _same_icp(x, y, f"thread {k}, item {i}")
    assert vm.batch_fetch(7, ql.VMAP_BATCH_TRACE, slot=1).shape[0] == want[1][7]["iterations"]
    # the map: its five sections and its counts as before
    _same_sections(_sections(vm), before, "the map after the batches")
    assert vm.info() == info


def _single(h, vm, item):
    """The single call on slot 0 with its trace and corr sections (the slot's debug sections)."""
    from quatro_amd import lib as ql
    r = vm.register(*item)
    return r, h.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18), h.debug_fetch(ql.DBG_ICP_CORR, np.int32)


def _same_as_single(h, vm, items, got, fetched, what):
    for i, item in enumerate(items):
        r, trace, corr = _single(h, vm, item)
        _same_icp(got[i], r, f"{what}, item {i}")
        assert fetched[i][0].shape == trace.shape and np.array_equal(_bits(fetched[i][0]), _bits(trace)), (what, i)
        assert np.array_equal(fetched[i][1], corr), (what, i)


def test_host_items_of_the_same_arrays_share_a_staged_copy_and_a_copy_of_them_does_not_matter(hip, hand):
    """Three host items of 257 points (two chunks): items 0 and 2 are the same arrays under two guesses (one staged copy),
    item 1 is a copy of them under item 0's guess (a staged copy of its own)."""
    vm, _ = hand
    p, a = BC.plane_cloud(257, 35)
    items = [(p, a, BC.small(80)), (p.copy(), a.copy(), BC.small(80)), (p, a, BC.small(81))]
    got = vm.register_batch(items)
    fetched = _fetched(vm, 3)
    _same_icp(got[1], got[0], "the copy against the arrays")
    assert np.array_equal(_bits(fetched[1][0]), _bits(fetched[0][0])) and np.array_equal(fetched[1][1], fetched[0][1])
    _same_as_single(hip, vm, items, got, fetched, "shared staging")


def test_the_arena_follows_a_small_a_large_and_a_small_call_on_a_fresh_handle():
    """B = 1 with n = 1, then B = 3 with n = 513, then B = 1 with n = 1 on a handle's first batches: the arena is made, grown
    and reused; every call is the single calls', and the fetch after the third serves the third."""
    from quatro_amd import lib as ql
    h = ql.Handle(0)
    vm = None
    try:
        vm = BC.hand_map(h.voxel_map)
        for k, sizes in enumerate(((1,), (513, 513, 513), (1,))):
            items = [BC.plane_cloud(n, 90 + 3 * k + j) + (BC.small(90 + 3 * k + j),) for j, n in enumerate(sizes)]
            got = vm.register_batch(items)
            _same_as_single(h, vm, items, got, _fetched(vm, len(items)), f"call {k}")
        assert vm.batch_fetch(0, ql.VMAP_BATCH_CORR).shape == (1,)
        with pytest.raises(ql.QuatroHipError):
            vm.batch_fetch(1, ql.VMAP_BATCH_CORR)  # (the slot's last batch had one item)
    finally:
        if vm is not None:
            vm.destroy()
        h.close()


def test_relocalize_on_the_room_returns_the_restatement_s_winner(hip, room):
    from quatro_amd import api
    vm, ref, q, qa, hyp = room
    out = api.relocalize(hip, vm, (q, qa), hyp)
    want = [ref.register(q, qa, g) for g in hyp]
    for i in range(27):
        _same_icp(out["results"][i], want[i], f"room, hypothesis {i}")
    best = api.best_hypothesis(want)
    assert out["best"] == best and best >= 0 and np.array_equal(_bits(out["T"]), _bits(want[best]["T"]))
    end = float(np.linalg.norm(out["T"][:3, 3] - BC.ROOM_TRUE[:3, 3]))
    assert end < 0.5 * BC.ROOM_SIDE


def test_relocalize_and_relocalize_in_map_on_the_trajectory(hip, traj):
    from quatro_amd import api
    vm, ref, kfs, clouds, gt, index = (traj[k] for k in ("vm", "ref", "kfs", "clouds", "gt", "index"))
    qv, qn = clouds[6]
    out = api.relocalize_in_map(hip, index, gt[:6], vm, kfs[6], 3, yaws=(-0.03, 0.0, 0.03),
                                offsets=((0.0, 0.0), (0.5, 0.0), (0.0, 0.5)))
    assert len(out["matches"]) == 3 and out["guesses"].shape == (27, 4, 4) and len(out["results"]) == 27
    assert out["candidate"] == [c for c in range(3) for _ in range(9)]
    m0 = out["matches"][0]
    assert np.array_equal(_bits(out["guesses"][4]), _bits(api.pose_hypothesis(gt[m0["id"]], float(m0["yaw"]) + 0.0, 0.5, 0.0)))
    want = [ref.register(qv, qn, g) for g in out["guesses"]]
    for i in range(27):
        _same_icp(out["results"][i], want[i], f"trajectory, hypothesis {i}")
    best = api.best_hypothesis(want)
    assert out["best"] == best
    assert out["best_id"] == (out["matches"][out["candidate"][best]]["id"] if best >= 0 else -1)
    if best >= 0:
        assert np.array_equal(_bits(out["T"]), _bits(want[best]["T"]))
    # relocalize alone, from the same guesses
    again = api.relocalize(hip, vm, kfs[6], out["guesses"])
    assert again["best"] == best and all(_f64bits(x["rmse"]) == _f64bits(y["rmse"]) for x, y in zip(again["results"], want))
    # what the restatement shows (not asserted, as in section 15)
    terr = [float(np.linalg.norm(r["T"][:3, 3] - gt[6][:3, 3])) for r in want]
    rerr = [R.rot_err_deg(r["T"], gt[6]) for r in want]
    start = [float(np.linalg.norm(g[:3, 3] - gt[6][:3, 3])) for g in out["guesses"]]
    print(f"relocalize_in_map (restatement): matches {[(m['id'], round(m['yaw'], 3)) for m in out['matches']]}; winner {best}: "
          f"{terr[best]:.3f} m, {rerr[best]:.3f} deg from the scene's pose (n_corr {want[best]['n_corr']} of {qv.shape[0]}); "
          f"hypotheses start {min(start):.3f} .. {max(start):.3f} m away and end {min(terr):.3f} .. {max(terr):.3f} m away; "
          f"valid {sum(r['valid'] for r in want)} of 27; iterations {[r['iterations'] for r in want]}")


def test_every_refusal_leaves_not_run_records_and_the_map_unchanged(hip, hand, traj):
    from quatro_amd import lib as ql
    vm, ref = hand
    blib = ql.load_ext()
    items, _ = BC.CASES["invalid_beside_good"]()
    p, a, g = items[0]
    before = _sections(vm)
    good = vm.register_batch(items)
    other = ql.Handle(0)
    foreign_map = foreign_kf = None

    def refused(code, word, its, prm=None, via=None):
        rc, res = (vm if via is None else via).register_batch_raw(its, prm)  # (an empty map is falsy: no `or`)
        assert rc == code and word in hip.last_error(), (word, rc, hip.last_error())
        assert all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(len(its))), word
        assert all(res[i].iterations == 0 and res[i].valid == 0 for i in range(len(its))), word

    try:
        rc, _ = vm.register_batch_raw([])
        assert rc == ql.QTR_OK  # B = 0
        refused(ql.QTR_ERR_BAD_ARG, "B=65", [(p, a, g)] * 65)
        for mth in (0, 1, 2):
            refused(ql.QTR_ERR_BAD_ARG, "QTR_ICP_VOXEL_PLANE_TO_PLANE", items, ql.default_icp_params(method=mth))
        refused(ql.QTR_ERR_BAD_ARG, "invalid ICP parameter", items, _prm(max_iterations=0))
        for bad_value in (np.nan, np.inf, -np.inf):
            bad = np.array(g)
            bad[2, 1] = bad_value
            refused(ql.QTR_ERR_BAD_ARG, "non-finite", [items[0], (p, a, bad), items[2]])
        refused(ql.QTR_ERR_BAD_ARG, "item 1", [items[0], (p, None, g)])  # no normals
        big = np.zeros((hip.limits.max_points + 1, 4), np.float32)
        refused(ql.QTR_ERR_CAPACITY, "max_points", [items[0], items[2], (big, big, g)])
        foreign_map = other.voxel_map(1.0, 64)
        stolen = ql.VoxelMap(hip, foreign_map._m.value)  # the other handle's map through this handle
        refused(ql.QTR_ERR_BAD_ARG, "another handle", items, via=stolen)
        stolen._m = None  # (not this wrapper's to destroy)
        foreign_kf = other.keyframe(traj["clouds"][0][0])
        refused(ql.QTR_ERR_BAD_ARG, "another handle", [items[0], (foreign_kf, g)])
        # the whole texts: the single call's words behind the item's prefix, for items 0, 1 and 2
        nan, mp = np.array(g), hip.limits.max_points
        nan[0, 3] = np.nan
        no_normals = "voxel map register: src_normals4 is NULL (the cloud entries do not compute normals)"
        for code, text, its in (
                (ql.QTR_ERR_BAD_ARG, "batch item 0: " + no_normals, [(p, None, g), items[1]]),
                (ql.QTR_ERR_BAD_ARG, "batch item 1: " + no_normals, [items[0], (p, None, g)]),
                (ql.QTR_ERR_CAPACITY, f"batch item 2: voxel map register: n={mp + 1} exceeds max_points={mp}",
                 [items[0], items[2], (big, big, g)]),
                (ql.QTR_ERR_BAD_ARG, "batch item 1: voxel map register: the guess has a non-finite entry in rows 0 - 2",
                 [items[0], (p, a, nan), items[2]]),
                (ql.QTR_ERR_BAD_ARG, "batch item 2: voxel map register: the guess has a non-finite entry in rows 0 - 2",
                 [items[0], items[1], (traj["kfs"][0], nan)]),
                (ql.QTR_ERR_BAD_ARG, "batch item 1: keyframe belongs to another handle", [items[0], (foreign_kf, g)])):
            refused(code, text, its)
            assert hip.last_error() == text, (hip.last_error(), text)
        # two faults in one item: the cloud's checks come first, in the single call's order, then the guess
        refused(ql.QTR_ERR_CAPACITY, "max_points", [items[0], (big, big, nan)])
        refused(ql.QTR_ERR_BAD_ARG, "src_normals4", [items[0], (big, None, nan)])
        # ... and the single calls judge the pose or guess before the cloud's size
        for call, word in ((lambda: vm.insert(big, big, nan), "voxel map insert: the pose has a non-finite entry in rows 0 - 2"),
                           (lambda: vm.register(big, big, nan), "voxel map register: the guess has a non-finite entry in rows 0 - 2")):
            with pytest.raises(ql.QuatroHipError) as e:
                call()
            assert e.value.code == ql.QTR_ERR_BAD_ARG and hip.last_error() == word, (e.value.code, hip.last_error())
        # NULL pointers and a negative count, through the C ABI as it stands
        arr, keep = vm._batch_items(items)
        res = (ql.IcpResult * 3)()
        prm = _prm()
        h, m = hip._h, vm._m
        assert blib.qtr_voxel_map_register_batch(h, 0, m, arr, -1, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        assert blib.qtr_voxel_map_register_batch(h, 0, m, None, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        assert all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(3))
        assert blib.qtr_voxel_map_register_batch(h, 0, m, arr, 3, None, res) == ql.QTR_ERR_BAD_ARG
        assert all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(3))
        assert blib.qtr_voxel_map_register_batch(h, 0, m, arr, 3, ctypes.byref(prm), None) == ql.QTR_ERR_BAD_ARG
        assert blib.qtr_voxel_map_register_batch(h, 0, None, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        assert all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(3))
        assert blib.qtr_voxel_map_register_batch(h, 7, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG  # no such slot
        arr[1].mem = 5
        assert blib.qtr_voxel_map_register_batch(h, 0, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        arr[1].mem = 7
        assert blib.qtr_voxel_map_register_batch(h, 0, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        assert hip.last_error() == "batch item 1: bad voxel map register arguments"
        arr[1].mem, arr[1].n = ql.MEM_HOST, -2
        assert blib.qtr_voxel_map_register_batch(h, 0, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        assert all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(3))
        del keep
        assert blib.qtr_voxel_map_batch_fetch(h, 0, 0, 9, None, 0) == -1 and blib.qtr_voxel_map_batch_fetch(h, 0, 64, 1, None, 0) == -1
        # nothing ran and nothing broke: the slot's last batch is still the good one, the next batch gives the same bits
        assert vm.batch_fetch(0, ql.VMAP_BATCH_TRACE).shape[0] == good[0]["iterations"]
        for i, (x, y) in enumerate(zip(vm.register_batch(items), good)):
            _same_icp(x, y, f"after the refusals, item {i}")
        _same_sections(_sections(vm), before, "the map after the refusals")
    finally:
        if foreign_kf is not None:
            foreign_kf.close()
        if foreign_map is not None:
            foreign_map.destroy()
        other.close()


def test_cpp_voxelmap_batch_demo_prints_what_the_python_calls_return(hip, tmp_path):
    from quatro_amd import api, synth
    from quatro_amd import build as qbuild
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "voxelmap_batch_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "voxelmap_batch_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath),
                           "-Wl,-rpath,/opt/rocm/lib"])
    inserts, (q, qa), _ = BC.room()
    pts, nrm, pose = inserts[0]
    base = api.pose_hypothesis(BC.ROOM_TRUE, 0.03, 0.2, -0.15)
    args = [repr(BC.ROOM_SIDE)]
    for name, x in (("a", pts), ("an", nrm), ("pa", pose), ("q", q), ("qn", qa), ("base", base)):
        path = str(tmp_path / name)
        if x.shape == (4, 4):
            np.savetxt(path, x, fmt="%.17g")
        else:
            synth.save_kitti_bin(path, x)
        args.append(path)
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    vm = hip.voxel_map(BC.ROOM_SIDE, 1 << 16)
    try:
        vm.insert(pts, nrm, pose)
        hyp = api.pose_hypotheses(base, (-0.1, 0.0, 0.1), ((0.0, 0.0), (BC.ROOM_SIDE, 0.0), (0.0, BC.ROOM_SIDE)))
        res = vm.register_batch([(q, qa, g) for g in hyp])
        for i, r in enumerate(res):
            want = (f"item {i}: iterations {r['iterations']} stop {r['stop_reason']} corr {r['n_corr']} valid {int(r['valid'])} "
                    f"rmse {int(_f64bits(r['rmse'])):016x}")
            assert out[i] == want, (out[i], want)
        best = api.best_hypothesis(res)
        assert out[9] == f"best {best}" and best >= 0
        words = np.array([int(x, 16) for ln in out[10:14] for x in ln.split()], dtype=np.uint64).view(np.float64)
        assert np.array_equal(_bits(words), _bits(res[best]["T"].reshape(16)))
    finally:
        vm.destroy()
