"""The evaluation of poses against the voxel map on the MI355X (qtr_voxel_map_evaluate*, libquatro_ext.so): every
named case bit-equal to the restatement (tests/vmap_eval_restate.py) through the cloud entry with host and device memory,
the keyframe entry and the batch; batch = single; the largest group; mixed items; repeatability; what an evaluation must
leave untouched; two slots; relocalize(keep=); the corridor; localisation -> evaluation -> pose-graph edge end to end; the
refusals and the C++ demo.  Everything goes through the C ABI (quatro_amd.lib)."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import icp_restate as R
import vmap_batch_cases as BC
import vmap_eval_cases as EC
import vmap_eval_restate as E
import vmap_restate as M

pytestmark = pytest.mark.gpu

SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)
ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same(got, want, what=""):
    assert got.get("status", 0) == 0, what
    bad = E.same_bits(got, want)
    assert not bad, (what, bad, [(k, got[k], want[k]) for k in bad[:2]])


def _same_icp(a, b, what=""):
    assert a.get("status", 0) == b.get("status", 0), what
    assert np.array_equal(_bits(a["T"]), _bits(b["T"])), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _same_points(vm, i, want, what="", slot=0):
    from quatro_amd import lib as ql
    corr, point = vm.eval_fetch(i, ql.VMAP_EVAL_CORR, slot), vm.eval_fetch(i, ql.VMAP_EVAL_POINT, slot)
    assert np.array_equal(corr, want["corr"]), what
    assert point.shape == want["point"].shape and np.array_equal(_bits(point), _bits(want["point"])), what


def _sections(vm):
    return {k: vm.fetch(k) for k in SECTIONS}


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
def maps(hip):
    """Per case: the device map, the items and the restatement's evaluations (computed once, shared, left unchanged)."""
    made, out = {}, {}
    for name, fn in EC.CASES.items():
        build, items = fn()
        if build not in made:
            vm = build(hip.voxel_map)
            made[build] = (vm, E.sections(build(M.RefMap)))
        vm, sec = made[build]
        out[name] = (vm, items, [E.evaluate(sec, p, a, T) for p, a, T in items], sec)
    yield out
    for vm, _ in made.values():
        vm.destroy()


@pytest.fixture(scope="module")
def traj(hip):
    """kitti64_trajectory(0, n_scans=6): keyframes of the six scans and of the revisit, their fetched clouds, and the map of
    scans 0 - 5 under the scene's poses with its restated sections."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    scans, gt = synth.kitti64_trajectory(0, n_scans=6)
    fp = ql.default_frontend_params()
    kfs = [hip.keyframe(s, fp) for s in scans[:7]]
    clouds = [(k.fetch(ql.KF_VOX), k.fetch(ql.KF_NORMALS)) for k in kfs]
    vm = hip.voxel_map(1.0, 1 << 16)
    for k in range(6):
        vm.insert_keyframe(kfs[k], gt[k])
    yield {"kfs": kfs, "clouds": clouds, "gt": np.asarray(gt), "vm": vm, "sec": E.sections(vm)}
    vm.destroy()
    for k in kfs:
        k.close()


@pytest.mark.parametrize("case", sorted(EC.CASES))
def test_device_equals_the_restatement_through_every_entry(hip, maps, case):
    import torch
    vm, items, want, _ = maps[case]
    if case == "room":  # (27 poses of one cloud: the batch below holds them all; the single entries take three of them)
        singles = (0, 13, 27)
    else:
        singles = range(len(items))
    for i in singles:
        p, a, T = items[i]
        _same(vm.evaluate(p, a, T, per_point=True), want[i], f"{case}, item {i}: host cloud")
        _same_points(vm, 0, want[i], f"{case}, item {i}: host cloud")
        if p.shape[0] > 0:  # (an empty torch tensor has no device pointer to hand over)
            dp, da = torch.from_numpy(p).cuda(), torch.from_numpy(a).cuda()
            _same(vm.evaluate(dp, da, T, per_point=True), want[i], f"{case}, item {i}: device cloud")
            _same_points(vm, 0, want[i], f"{case}, item {i}: device cloud")
        _same(vm.evaluate(p, a, T), want[i], f"{case}, item {i}: without per-point output")
    got = vm.evaluate_batch(items, per_point=True)
    assert len(got) == len(items)
    for i in range(len(items)):
        _same(got[i], want[i], f"{case}, batch item {i}")
        _same_points(vm, i, want[i], f"{case}, batch item {i}")
    for i, g in enumerate(vm.evaluate_batch(items)):
        _same(g, want[i], f"{case}, batch item {i} without per-point output")
    print(f"{case}: n_source {[w['n_source'] for w in want][:8]} n_corr {[w['n_corr'] for w in want][:8]}")


def test_keyframe_entry_and_mixed_items_in_one_call(hip, traj):
    import torch
    vm, sec, kfs, clouds, gt = traj["vm"], traj["sec"], traj["kfs"], traj["clouds"], traj["gt"]
    off = [R.rigid(R.rot(0.004 * j, -0.003, 0.01 * j), [0.1 * j, -0.15, 0.02]) for j in range(6)]
    dev = [torch.from_numpy(x).cuda() for x in clouds[4]]
    items = [(kfs[1], gt[1] @ off[0]), (clouds[2][0], clouds[2][1], gt[2] @ off[1]), (dev[0], dev[1], gt[4] @ off[2]),
             (kfs[1], gt[1] @ off[3]), (dev[0], dev[1], gt[4] @ off[4]), (kfs[3], gt[3] @ off[5]),
             (clouds[2][0], clouds[2][1], gt[2] @ off[2])]
    want = [E.evaluate(sec, clouds[k][0], clouds[k][1], items[i][-1]) for i, k in enumerate((1, 2, 4, 1, 4, 3, 2))]
    got = vm.evaluate_batch(items, per_point=True)
    for i in range(len(items)):
        _same(got[i], want[i], f"mixed item {i}")
        _same_points(vm, i, want[i], f"mixed item {i}")
    assert all(w["valid"] for w in want)
    print("mixed items: overlap", [round(w["overlap"], 3) for w in want])
    _same(vm.evaluate_keyframe(kfs[1], items[3][1], per_point=True), want[3], "evaluate_keyframe")
    _same_points(vm, 0, want[3], "evaluate_keyframe")
    _same(vm.evaluate_keyframe(kfs[3], items[5][1]), want[5], "evaluate_keyframe without per-point output")


def test_batch_equals_single_at_one_sixty_four_and_sixty_five(hip, maps):
    from quatro_amd import lib as ql
    vm, _, _, sec = maps["sizes"]
    clouds = [BC.plane_cloud(n, 200 + j) for j, n in enumerate((120, 255, 256, 257, 300, 511, 513, 700))]
    items = [(clouds[j % 8][0], clouds[j % 8][1], BC.small(60 + j)) for j in range(65)]
    single = [vm.evaluate(p, a, T) for p, a, T in items]
    for i in (0, 5, 64):
        _same(single[i], E.evaluate(sec, *items[i]), f"single {i}")
    for B in (1, 64, 65):
        for i, g in enumerate(vm.evaluate_batch(items[:B])):
            _same(g, single[i], f"B = {B}, item {i}")
    got = vm.evaluate_batch(items[:64], per_point=True)
    for i in range(64):
        _same(got[i], single[i], f"B = 64 with per-point output, item {i}")
    # 65 with per-point output: refused by the C call, two chunks through evaluate_batch
    rc, res = vm.evaluate_batch_raw(items, per_point=True)
    assert rc == ql.QTR_ERR_BAD_ARG and "B=65" in hip.last_error() and all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(65))
    got = vm.evaluate_batch(items, per_point=True)
    assert len(got) == 65 and vm.eval_fetch(0, ql.VMAP_EVAL_CORR).shape[0] == items[64][0].shape[0]
    with pytest.raises(ql.QuatroHipError):
        vm.eval_fetch(1, ql.VMAP_EVAL_CORR)  # (the slot's last call had one item)
    for i in range(65):
        _same(got[i], single[i], f"65 in two chunks, item {i}")
    rc, res = vm.evaluate_batch_raw(items)  # without: one group of 65
    assert rc == ql.QTR_OK and all(res[i].status == ql.QTR_OK for i in range(65))


def test_largest_group_of_1024_poses(hip, maps):
    from quatro_amd import api
    from quatro_amd import lib as ql
    vm, _, _, sec = maps["sizes"]
    p, a = BC.plane_cloud(300, 31)
    offs = [(0.05 * (i - 3.5), 0.07 * (j - 1.5)) for i in range(8) for j in range(4)]
    hyp = api.pose_hypotheses(BC.small(2), [0.01 * (k - 16) for k in range(32)], offs)
    assert hyp.shape == (1024, 4, 4)
    sc = api.score_hypotheses(hip, vm, (p, a), hyp)
    want = [E.evaluate(sec, p, a, g) for g in hyp]
    for i in range(1024):
        _same(sc["evaluations"][i], want[i], f"pose {i}")
    assert sc["order"] == api.evaluation_order(want) and sc["best"] == api.best_evaluation(want) == sc["order"][0]
    assert len({w["n_corr"] for w in want}) > 10
    items = [(p, a, g) for g in hyp] + [(p, a, np.eye(4))]
    rc, res = vm.evaluate_batch_raw(items)
    assert rc == ql.QTR_ERR_BAD_ARG and "B=1025" in hip.last_error()
    assert all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(1025))
    got = vm.evaluate_batch(items)  # chunked: 1024 + 1
    assert len(got) == 1025
    _same(got[1024], E.evaluate(sec, p, a, np.eye(4)), "the 1025th")
    _same(got[77], want[77], "item 77 of the chunked call")


def test_repeatable_map_unchanged_other_arenas_untouched_and_two_slots(hip, maps):
    from quatro_amd import lib as ql
    vm, items, want, _ = maps["sizes"]
    before, info = _sections(vm), vm.info()
    # a single registration, a registration batch and a pair evaluation on slot 0, then evaluations, then their fetches
    p, a = BC.plane_cloud(300, 31)
    g = BC.small(25)
    one = vm.register(p, a, g)
    trace1 = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    corr1 = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
    eight, _ = BC.CASES["one_cloud_eight_guesses"]()
    batch = vm.register_batch(eight)
    btrace = [vm.batch_fetch(i, ql.VMAP_BATCH_TRACE) for i in range(8)]
    q, qa = BC.plane_cloud(257, 33)
    pair = hip.evaluate(p, q, g)
    ecorr = hip.debug_fetch(ql.DBG_EVAL_CORR, np.int32)
    first = vm.evaluate_batch(items, per_point=True)
    f_first = [(vm.eval_fetch(i, ql.VMAP_EVAL_CORR), vm.eval_fetch(i, ql.VMAP_EVAL_POINT)) for i in range(len(items))]
    second = vm.evaluate_batch(items, per_point=True)
    for i in range(len(items)):  # twice the same bits
        _same(first[i], want[i], f"first, item {i}")
        _same(second[i], first[i], f"twice, item {i}")
        assert np.array_equal(vm.eval_fetch(i, ql.VMAP_EVAL_CORR), f_first[i][0])
        assert np.array_equal(_bits(vm.eval_fetch(i, ql.VMAP_EVAL_POINT)), _bits(f_first[i][1]))
    times = vm.eval_fetch(0, ql.VMAP_EVAL_TIMES)
    assert times.shape == (1,) and times.dtype == np.float32 and times[0] > 0
    assert np.array_equal(_bits(hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)), _bits(trace1))
    assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_CORR, np.int32), corr1)
    assert all(np.array_equal(_bits(vm.batch_fetch(i, ql.VMAP_BATCH_TRACE)), _bits(btrace[i])) for i in range(8))
    assert np.array_equal(hip.debug_fetch(ql.DBG_EVAL_CORR, np.int32), ecorr)
    _same_icp(vm.register(p, a, g), one, "the single registration after the evaluations")
    for x, y in zip(vm.register_batch(eight), batch):
        _same_icp(x, y, "the registration batch after the evaluations")
    again = hip.evaluate(p, q, g)
    assert all(np.array_equal(_bits(np.asarray(again[k], np.float64)), _bits(np.asarray(pair[k], np.float64)))
               for k in ("overlap", "sum_d2", "inlier_rmse", "information"))
    # a call without per-point output serves no per-point section
    vm.evaluate_batch(items)
    with pytest.raises(ql.QuatroHipError):
        vm.eval_fetch(2, ql.VMAP_EVAL_CORR)
    assert vm.eval_fetch(0, ql.VMAP_EVAL_TIMES).shape == (1,)
    # two slots evaluating against the one map from two threads: the sequential results
    other = [(p, a, BC.small(70 + j)) for j in range(8)]
    seq = [vm.evaluate_batch(items, slot=0), vm.evaluate_batch(other, slot=0)]
    got, err = [None, None], []

    def work(k, its):
        try:
            for _ in range(3):
                got[k] = vm.evaluate_batch(its, per_point=True, slot=k)
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(0, items)), threading.Thread(target=work, args=(1, other))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k in range(2):
        for i, (x, y) in enumerate(zip(got[k], seq[k])):
            _same(x, y, f"thread {k}, item {i}")
    assert vm.eval_fetch(7, ql.VMAP_EVAL_CORR, slot=1).shape[0] == 300
    # the map: its five sections and its counts as before
    after = _sections(vm)
    assert all(after[k].shape == before[k].shape and np.array_equal(_bits(after[k]), _bits(before[k])) for k in SECTIONS)
    assert vm.info() == info


def _same_as_single(vm, items, got, what):
    """A per-point batch that has just run against the single calls: records and both per-point sections, bit for bit."""
    from quatro_amd import lib as ql
    fetched = [(vm.eval_fetch(i, ql.VMAP_EVAL_CORR), vm.eval_fetch(i, ql.VMAP_EVAL_POINT)) for i in range(len(items))]
    for i, item in enumerate(items):
        _same(got[i], vm.evaluate(*item, per_point=True), f"{what}, item {i}")
        assert np.array_equal(fetched[i][0], vm.eval_fetch(0, ql.VMAP_EVAL_CORR)), (what, i)
        assert np.array_equal(_bits(fetched[i][1]), _bits(vm.eval_fetch(0, ql.VMAP_EVAL_POINT))), (what, i)
    return fetched


def test_host_items_of_the_same_arrays_share_a_staged_copy_and_a_copy_of_them_does_not_matter(hip, maps):
    """Three host items of 257 points (two chunks) with per-point output: items 0 and 2 are the same arrays under two poses
    (one staged copy), item 1 is a copy of them under item 0's pose (a staged copy of its own)."""
    vm, _, _, sec = maps["sizes"]
    p, a = BC.plane_cloud(257, 35)
    items = [(p, a, BC.small(80)), (p.copy(), a.copy(), BC.small(80)), (p, a, BC.small(81))]
    got = vm.evaluate_batch(items, per_point=True)
    fetched = _same_as_single(vm, items, got, "shared staging")
    _same(got[1], got[0], "the copy against the arrays")
    assert np.array_equal(fetched[1][0], fetched[0][0]) and np.array_equal(_bits(fetched[1][1]), _bits(fetched[0][1]))
    for i in range(3):
        _same(got[i], E.evaluate(sec, *items[i]), f"shared staging against the restatement, item {i}")


def test_the_arena_follows_a_small_a_large_and_a_small_call_on_a_fresh_handle():
    """B = 1 with n = 1, then B = 3 with n = 513, then B = 1 with n = 1 on a handle's first evaluations: the arena is made,
    grown and reused; every call is the single calls', and the fetch after the third serves the third."""
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    vm = None
    try:
        vm = BC.hand_map(h.voxel_map)
        for k, sizes in enumerate(((1,), (513, 513, 513), (1,))):
            items = [BC.plane_cloud(n, 90 + 3 * k + j) + (BC.small(90 + 3 * k + j),) for j, n in enumerate(sizes)]
            got = vm.evaluate_batch(items, per_point=True, slot=1)
            fetched = [(vm.eval_fetch(i, ql.VMAP_EVAL_CORR, 1), vm.eval_fetch(i, ql.VMAP_EVAL_POINT, 1)) for i in range(len(items))]
            for i, item in enumerate(items):  # (the single calls on slot 0: slot 1's arena sees only the three groups)
                _same(got[i], vm.evaluate(*item, per_point=True), f"call {k}, item {i}")
                assert np.array_equal(fetched[i][0], vm.eval_fetch(0, ql.VMAP_EVAL_CORR)), (k, i)
                assert np.array_equal(_bits(fetched[i][1]), _bits(vm.eval_fetch(0, ql.VMAP_EVAL_POINT))), (k, i)
        assert vm.eval_fetch(0, ql.VMAP_EVAL_CORR, 1).shape == (1,)
        with pytest.raises(ql.QuatroHipError):
            vm.eval_fetch(1, ql.VMAP_EVAL_CORR, 1)  # (the slot's last evaluation had one item)
    finally:
        if vm is not None:
            vm.destroy()
        h.close()


def test_relocalize_keep_returns_the_full_batch_s_winner_on_the_room(hip, maps):
    from quatro_amd import api
    vm, items, want, _ = maps["room"]
    q, qa = items[0][0], items[0][1]
    hyp = np.stack([T for _, _, T in items[:27]])
    full = api.relocalize(hip, vm, (q, qa), hyp)
    assert "scores" not in full and all(r is not None for r in full["results"])
    again = api.relocalize(hip, vm, (q, qa), hyp, keep=None)  # today's output
    assert again["best"] == full["best"] and sorted(again) == sorted(full) == ["T", "best", "results"]
    for x, y in zip(again["results"], full["results"]):
        _same_icp(x, y, "keep=None")
    kept = api.relocalize(hip, vm, (q, qa), hyp, keep=EC.ROOM_KEEP)
    assert kept["best"] == full["best"] and np.array_equal(_bits(kept["T"]), _bits(full["T"]))
    chosen = [i for i, r in enumerate(kept["results"]) if r is not None]
    assert len(chosen) == EC.ROOM_KEEP and sorted(kept["scores"]["order"][:EC.ROOM_KEEP]) == chosen
    for i in chosen:
        _same_icp(kept["results"][i], full["results"][i], f"kept item {i}")
    for i in range(27):
        _same(kept["scores"]["evaluations"][i], want[i], f"score {i}")
    assert kept["scores"]["order"].index(full["best"]) + 1 == EC.ROOM_RANK


def test_corridor_degeneracy_inputs_are_the_restatement_s(hip, maps):
    from quatro_amd import api
    vm, items, want, _ = maps["corridor"]
    got = vm.evaluate(*items[0])
    _same(got, want[0], "corridor")
    d, dw = api.degeneracy(got), api.degeneracy(want[0])
    assert all(np.array_equal(_bits(d[k]), _bits(dw[k])) for k in ("eigenvalues", "weakest_translation", "translation_eigenvalues"))
    assert abs(d["weakest_translation"][0]) > np.cos(np.radians(5.0))
    assert d["translation_eigenvalues"][0] < 0.1 * d["translation_eigenvalues"][1]


def test_localise_evaluate_and_optimise_end_to_end(hip, traj):
    from quatro_amd import api
    vm, sec, kfs, clouds, gt = traj["vm"], traj["sec"], traj["kfs"], traj["clouds"], traj["gt"]
    guess = gt[6] @ R.rigid(R.rot(0.0, 0.0, 0.01), [0.2, -0.1, 0.0])
    loc = api.localize(hip, vm, kfs[6], guess)
    assert loc["valid"]
    ev = vm.evaluate_keyframe(kfs[6], loc["T"])
    _same(ev, E.evaluate(sec, clouds[6][0], clouds[6][1], loc["T"]), "the revisit scan at its localised pose")
    assert ev["valid"]
    g = api.PoseGraph()
    m = g.add_map_node()
    n = g.add_node(R.rigid(R.rot(0.01, -0.01, 0.03), [0.4, -0.3, 0.1]) @ loc["T"])  # a drifted start
    g.add_localization(n, m, loc, ev)
    res = g.optimize(hip)
    assert res["valid"]
    end = g.poses[n]
    print(f"end to end: n_corr {ev['n_corr']} overlap {ev['overlap']:.3f}; the node ends "
          f"{np.linalg.norm(end[:3, 3] - loc['T'][:3, 3]):.2e} m from the registration's pose; condition {api.degeneracy(ev)['condition']:.3g}")
    assert np.linalg.norm(end[:3, 3] - loc["T"][:3, 3]) < 0.01 and np.array_equal(g.poses[m], np.eye(4))


def test_every_refusal_leaves_not_run_records(hip, maps, traj):
    from quatro_amd import lib as ql
    vm, items, want, _ = maps["sizes"]
    elib = ql.load_ext()
    its = items[2:5]
    p, a, T = its[0]
    before = _sections(vm)
    good = vm.evaluate_batch(its, per_point=True)
    other = ql.Handle(0)
    foreign_map = foreign_kf = None

    def refused(code, word, bad_items, via=None):
        rc, res = (vm if via is None else via).evaluate_batch_raw(bad_items)
        assert rc == code and word in hip.last_error(), (word, rc, hip.last_error())
        assert all(res[i].status == ql.QTR_ERR_NOT_RUN and res[i].valid == 0 and res[i].n_source == 0 for i in range(len(bad_items))), word

    try:
        rc, _ = vm.evaluate_batch_raw([])
        assert rc == ql.QTR_OK  # B = 0
        for bad_value in (np.nan, np.inf, -np.inf):
            bad = np.array(T)
            bad[2, 1] = bad_value
            refused(ql.QTR_ERR_BAD_ARG, "item 1", [its[0], (p, a, bad), its[2]])
            assert "non-finite" in hip.last_error()
        refused(ql.QTR_ERR_BAD_ARG, "item 1", [its[0], (p, None, T)])  # no normals
        big = np.zeros((hip.limits.max_points + 1, 4), np.float32)
        refused(ql.QTR_ERR_CAPACITY, "max_points", [its[0], its[2], (big, big, T)])
        assert "item 2" in hip.last_error()
        foreign_map = other.voxel_map(1.0, 64)
        stolen = ql.VoxelMap(hip, foreign_map._m.value)  # the other handle's map through this handle
        refused(ql.QTR_ERR_BAD_ARG, "another handle", its, via=stolen)
        stolen._m = None  # (not this wrapper's to destroy)
        foreign_kf = other.keyframe(traj["clouds"][0][0])
        refused(ql.QTR_ERR_BAD_ARG, "another handle", [its[0], (foreign_kf, T)])
        # the whole texts: the single call's words behind the item's prefix, for items 0, 1 and 2
        nan, mp = np.array(T), hip.limits.max_points
        nan[0, 3] = np.nan
        no_normals = "voxel map evaluate: src_normals4 is NULL (the cloud entries do not compute normals)"
        for code, text, bad_items in (
                (ql.QTR_ERR_BAD_ARG, "evaluate item 0: " + no_normals, [(p, None, T), its[1]]),
                (ql.QTR_ERR_BAD_ARG, "evaluate item 1: " + no_normals, [its[0], (p, None, T)]),
                (ql.QTR_ERR_CAPACITY, f"evaluate item 2: voxel map evaluate: n={mp + 1} exceeds max_points={mp}",
                 [its[0], its[2], (big, big, T)]),
                (ql.QTR_ERR_BAD_ARG, "evaluate item 1: voxel map evaluate: the pose has a non-finite entry in rows 0 - 2",
                 [its[0], (p, a, nan), its[2]]),
                (ql.QTR_ERR_BAD_ARG, "evaluate item 2: voxel map evaluate: the pose has a non-finite entry in rows 0 - 2",
                 [its[0], its[1], (traj["kfs"][0], nan)]),
                (ql.QTR_ERR_BAD_ARG, "evaluate item 1: keyframe belongs to another handle", [its[0], (foreign_kf, T)])):
            refused(code, text, bad_items)
            assert hip.last_error() == text, (hip.last_error(), text)
        # two faults in one item: the cloud's checks come first, in the single call's order, then the pose
        refused(ql.QTR_ERR_CAPACITY, "max_points", [its[0], (big, big, nan)])
        refused(ql.QTR_ERR_BAD_ARG, "src_normals4", [its[0], (big, None, nan)])
        # NULL pointers, a negative count and a bad mem, through the C ABI as it stands
        arr, keep = vm._batch_items(its)
        res = (ql.VmapEvalResult * 3)()
        one = ql.VmapEvalResult()
        prm = ql.default_vmap_eval_params()
        h, m = hip._h, vm._m
        not_run = lambda: all(res[i].status == ql.QTR_ERR_NOT_RUN for i in range(3))
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, arr, -1, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, None, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG and not_run()
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, arr, 3, None, res) == ql.QTR_ERR_BAD_ARG and not_run()
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, arr, 3, ctypes.byref(prm), None) == ql.QTR_ERR_BAD_ARG
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, None, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG and not_run()
        assert elib.qtr_voxel_map_evaluate_batch(h, 7, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG  # no such slot
        arr[1].mem = 5
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG and not_run()
        arr[1].mem = 7
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG and not_run()
        assert hip.last_error() == "evaluate item 1: bad voxel map evaluate arguments"
        arr[1].mem, arr[1].n = ql.MEM_HOST, -2
        assert elib.qtr_voxel_map_evaluate_batch(h, 0, m, arr, 3, ctypes.byref(prm), res) == ql.QTR_ERR_BAD_ARG and not_run()
        del keep
        T16 = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))
        assert elib.qtr_voxel_map_evaluate(h, 0, m, p.ctypes.data, a.ctypes.data, p.shape[0], ql.MEM_HOST, None, ctypes.byref(prm),
                                           ctypes.byref(one)) == ql.QTR_ERR_BAD_ARG and one.status == ql.QTR_ERR_NOT_RUN
        assert elib.qtr_voxel_map_evaluate(h, 0, m, p.ctypes.data, None, p.shape[0], ql.MEM_HOST, T16.ctypes.data, ctypes.byref(prm),
                                           ctypes.byref(one)) == ql.QTR_ERR_BAD_ARG and one.status == ql.QTR_ERR_NOT_RUN
        assert elib.qtr_voxel_map_evaluate_keyframe(h, 0, m, None, T16.ctypes.data, ctypes.byref(prm),
                                                    ctypes.byref(one)) == ql.QTR_ERR_BAD_ARG and one.status == ql.QTR_ERR_NOT_RUN
        assert elib.qtr_voxel_map_eval_fetch(h, 0, 0, 9, None, 0) == -1 and elib.qtr_voxel_map_eval_fetch(h, 0, 3, 1, None, 0) == -1
        assert elib.qtr_voxel_map_eval_fetch(h, 1, 0, ql.VMAP_EVAL_TIMES, None, 0) in (-1, 4)  # (slot 1: whether it has evaluated yet)
        assert elib.qtr_voxel_map_eval_fetch(h, 7, 0, ql.VMAP_EVAL_TIMES, None, 0) == -1
        # nothing ran and nothing broke: the slot's last evaluation is still the good one, the next gives the same bits
        for i in range(3):
            _same_points(vm, i, want[2 + i], f"after the refusals, item {i}")
        for i, g in enumerate(vm.evaluate_batch(its, per_point=True)):
            _same(g, good[i], f"after the refusals, item {i}")
        after = _sections(vm)
        assert all(np.array_equal(_bits(after[k]), _bits(before[k])) for k in SECTIONS)
    finally:
        if foreign_kf is not None:
            foreign_kf.close()
        if foreign_map is not None:
            foreign_map.destroy()
        other.close()


def test_fetch_before_the_slot_s_first_evaluation_is_refused():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quatro_amd import lib as ql
    h = ql.Handle(0)
    try:
        assert ql.load_ext().qtr_voxel_map_eval_fetch(h._h, 0, 0, ql.VMAP_EVAL_TIMES, None, 0) == -1
    finally:
        h.close()


def test_cpp_voxelmap_eval_demo_prints_what_the_python_calls_return(hip, tmp_path):
    from quatro_amd import api, synth
    from quatro_amd import build as qbuild
    libpath = qbuild.build_ext(force=False, verbose=False)
    exe = str(tmp_path / "voxelmap_eval_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "voxelmap_eval_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
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
        sc = api.score_hypotheses(hip, vm, (q, qa), hyp)
        for i, r in enumerate(sc["evaluations"]):
            want = (f"item {i}: source {r['n_source']} corr {r['n_corr']} valid {int(r['valid'])} "
                    f"overlap {int(_f64bits(r['overlap'])):016x} rmse {int(_f64bits(r['rmse'])):016x}")
            assert out[i] == want, (out[i], want)
        best = sc["best"]
        assert out[9] == f"best {best}" and best >= 0
        words = np.array([int(x, 16) for ln in out[10:16] for x in ln.split()], dtype=np.uint64).view(np.float64)
        assert np.array_equal(_bits(words), _bits(sc["evaluations"][best]["information"].reshape(36)))
    finally:
        vm.destroy()
