"""The front end's rare branches on every path that has them — a cloud that passes through the voxel grid (pcl::VoxelGrid's
int32 overflow), a cloud whose neighbour lists exceed QTR_KMAX on a handle that has not met one yet, the capacity
refusals behind the voxel stage — on the pair path (qtr_register_pair / _corr), the one-cloud path (keyframes) and the
grouped path (batch lanes).  Every case compares one path of the library against another, bit for bit; the oracle only
confirms on the CPU that the inputs are what the case needs."""
import numpy as np
import pytest

from quatro_amd import lib as ql
from quatro_amd import synth

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=65536, max_voxels=16384, max_corr=8192)
SMALL = dict(max_points=65536, max_voxels=1024, max_corr=8192)  # the handle that refuses: max_voxels below every big cloud
PASS_LEAF, LONG_LEAF = 0.001, 0.01
KMAX = 256  # QTR_KMAX (quatro_amd/csrc/frontend.h)


def _moved(p, yaw, t, seed, sigma):
    q = p.copy()
    q[:, :3] = (p[:, :3].astype(np.float64) @ synth.yaw_matrix(yaw).T + np.asarray(t)).astype(np.float32)
    q[:, :3] += np.random.default_rng(seed).normal(0, sigma, (q.shape[0], 3)).astype(np.float32)
    return q


def _neighbours(p, r):
    d = np.linalg.norm(p[:, None, :3].astype(np.float64) - p[None, :, :3].astype(np.float64), axis=2)
    return (d <= r).sum(1) - 1


@pytest.fixture(scope="module")
def data(qo):
    """normal: a lidar pair (10 k voxels at 0.3 m); small: its points within 20 m (a normal pair of a few hundred voxels);
    passing: 2000 points on a 5 m patch — at leaf 0.001 the grid overflows int32 and the cloud passes through; long: 600
    points in a 0.5 m cube — at leaf 0.01 every point has more than QTR_KMAX neighbours inside the FPFH radius."""
    fp = ql.default_frontend_params(seed=1)
    s, t, _ = synth.kitti64_pair(1)
    near = lambda p: np.ascontiguousarray(p[np.linalg.norm(p[:, :3], axis=1) < 20.0])
    g = np.random.default_rng(3)
    a = np.zeros((2000, 4), dtype=np.float32)
    a[:, 0], a[:, 1] = g.uniform(0, 5.0, 2000), g.uniform(0, 5.0, 2000)
    a[:, 2] = 0.15 * np.sin(1.3 * a[:, 0]) * np.cos(0.9 * a[:, 1]) + g.normal(0, 0.01, 2000)
    b = _moved(a, 0.3, (0.4, -0.2, 0.05), 9, 0.002)
    c = np.zeros((600, 4), dtype=np.float32)
    c[:, :3] = np.random.default_rng(5).uniform(0, 0.5, (600, 3))
    d = _moved(c, 0.2, (0.05, -0.03, 0.01), 11, 0.0005)
    e = np.zeros((250, 4), dtype=np.float32)  # tiny: 250 points on a 0.8 m patch — a grid that fits int32 even at leaf 0.001
    e[:, 0], e[:, 1] = g.uniform(0, 0.8, 250), g.uniform(0, 0.8, 250)
    e[:, 2] = 0.1 * np.sin(5.0 * e[:, 0]) * np.cos(4.0 * e[:, 1]) + g.normal(0, 0.002, 250)
    f = _moved(e, 0.2, (0.05, -0.03, 0.01), 13, 0.0005)
    d = {"normal": (s, t), "small": (near(s), near(t)), "passing": (a, b), "long": (c, d), "tiny": (e, f)}
    for p in d["tiny"]:  # voxelised for real at both small leaves (sorted by voxel, not handed back), and no long list (249 others)
        assert not np.array_equal(qo.voxelize(p, PASS_LEAF), p) and not np.array_equal(qo.voxelize(p, LONG_LEAF), p)
    for p in d["passing"]:  # pcl::VoxelGrid hands the cloud back as it is, and no list of it is a long one
        assert np.array_equal(qo.voxelize(p, PASS_LEAF), p)
        assert _neighbours(p, fp.fpfh_radius).max() < KMAX
    for p in d["long"]:
        assert _neighbours(qo.voxelize(p, LONG_LEAF), fp.fpfh_radius).min() > KMAX
    for p, q in zip(d["normal"], d["small"]):
        assert qo.voxelize(p, fp.voxel_size).shape[0] > SMALL["max_voxels"] >= qo.voxelize(q, fp.voxel_size).shape[0]
    assert min(p.shape[0] for p in d["passing"]) > SMALL["max_voxels"]
    return d


def _fp(kind):
    return ql.default_frontend_params(seed=2, voxel_size={"passing": PASS_LEAF, "long": LONG_LEAF}.get(kind, 0.3))


@pytest.fixture(scope="module")
def seq(data):
    """register_pair of every pair kind on one slot, one after the other: what the other paths must reproduce.  (The long
    pair goes last: it turns the handle's long lists on.)"""
    h = ql.Handle(0, **LIMITS)
    try:
        return {k: h.register_pair(*data[k], _fp(k)) for k in ("normal", "small", "passing", "long")}
    finally:
        h.close()


def _same(got, want, lists=True):
    assert (got["status"], got["valid"], got["n_src"], got["n_tgt"], got["L"]) == \
        (want["status"], want["valid"], want["n_src"], want["n_tgt"], want["L"])
    assert np.array_equal(got["T"], want["T"])
    assert got["n_rot_inliers"] == want["n_rot_inliers"]
    if lists:
        assert np.array_equal(got["clique"], want["clique"]) and np.array_equal(got["final_inliers"], want["final_inliers"])


def _dev_items(pairs, fp, corr=None):
    import torch
    dev = torch.device("cuda", 0)
    items = []
    for i, (s, t) in enumerate(pairs):
        it = {"src": torch.from_numpy(s).to(dev), "tgt": torch.from_numpy(t).to(dev), "fp": fp}
        if corr is not None:
            it["cs"], it["ct"] = torch.from_numpy(corr[0]).to(dev), torch.from_numpy(corr[1]).to(dev)
        items.append(it)
    torch.cuda.synchronize()
    return items


def _refusal(h, call):
    """(status code, the whole qtr_last_error text) of a call that must be refused"""
    with pytest.raises(ql.QuatroHipError) as e:
        call()
    return e.value.code, h.last_error()


def _corr300():
    return synth.correspondences(300, 0.1, seed=7, noise=0.1)[:2]


def test_keyframes_of_a_pass_through_pair_equal_register_pair(data, seq):
    s, t = data["passing"]
    fp = _fp("passing")
    h = ql.Handle(0, **LIMITS)
    try:
        with h.keyframe(s, fp) as ks, h.keyframe(t, fp) as kt:
            for kf, p in ((ks, s), (kt, t)):
                assert kf.info["passed_through"] == 1 and kf.info["n_voxels"] == p.shape[0]
                assert np.array_equal(kf.fetch(ql.KF_VOX), p)
            got = h.register_keyframes(ks, kt, fp)
    finally:
        h.close()
    assert (got["n_src"], got["n_tgt"]) == (s.shape[0], t.shape[0])
    _same(got, seq["passing"])


@pytest.mark.parametrize("host_mem", [True, False])
def test_batch_with_a_pass_through_pair_between_normal_pairs_equals_three_calls(data, seq, host_mem):
    """One leaf for the whole batch: the normal pairs are the tiny pair, whose grid fits int32 at 0.001 m."""
    fp = _fp("passing")
    kinds = ("tiny", "passing", "tiny")
    h = ql.Handle(0, n_slots=4, **LIMITS)
    try:
        want = [h.register_pair(*data[k], fp) for k in kinds]
        if host_mem:
            got = h.register_batch([(*data[k], 2) for k in kinds], fp)
        else:
            got = h.register_batch_dev(_dev_items([data[k] for k in kinds], fp), ql.demo_params(), fp)
    finally:
        h.close()
    _same(want[1], seq["passing"])
    for g, w in zip(got, want):
        _same(g, w, lists=host_mem)


def test_keyframe_of_a_long_list_cloud_on_a_fresh_handle(data, seq, qo):
    c, d = data["long"]
    fp = _fp("long")
    fresh, warm = ql.Handle(0, **LIMITS), ql.Handle(0, **LIMITS)
    try:
        _same(warm.register_pair(c, d, fp), seq["long"])  # (the warm handle's first call: its chains now carry long lists)
        with fresh.keyframe(c, fp) as ka, warm.keyframe(c, fp) as kb:  # ka: the chain starts without k2_neighbors_big
            assert ka.info == kb.info and ka.info["passed_through"] == 0
            for what in (ql.KF_VOX, ql.KF_NORMALS, ql.KF_FPFH, ql.KF_MEAN):
                assert np.array_equal(ka.fetch(what).view(np.uint32), kb.fetch(what).view(np.uint32))
            with fresh.keyframe(d, fp) as kd:
                _same(fresh.register_keyframes(ka, kd, fp), seq["long"])
    finally:
        fresh.close()
        warm.close()
    h = ql.Handle(0, max_long_neighbors=4096, **LIMITS)  # every list of the cloud is a long one: ~350 k entries
    try:
        with pytest.raises(ql.QuatroHipError, match="max_long_neighbors") as e:
            h.keyframe(c, fp)
        assert e.value.code == ql.QTR_ERR_CAPACITY
        # the whole text, on every path: the longest list of a cloud is its point with the most voxels inside the FPFH radius
        # (the point itself included)
        longest = [int(_neighbours(qo.voxelize(p, LONG_LEAF), fp.fpfh_radius).max()) + 1 for p in (c, d)]
        text = "radius-neighbour lists longer than %d entries (longest %s) exceed the long-list arena: " \
               "qtr_limits.max_long_neighbors is 4096"
        assert _refusal(h, lambda: h.keyframe(c, fp)) == (ql.QTR_ERR_CAPACITY, text % (KMAX, "%d" % longest[0]))
        assert _refusal(h, lambda: h.keyframe(d, fp)) == (ql.QTR_ERR_CAPACITY, text % (KMAX, "%d" % longest[1]))
        both = (ql.QTR_ERR_CAPACITY, text % (KMAX, "%d / %d" % tuple(longest)))
        assert _refusal(h, lambda: h.register_pair(c, d, fp)) == both
        assert _refusal(h, lambda: h.register_pair_corr(c, d, *_corr300(), fp)) == both
        _same(h.register_pair(*data["small"], _fp("small")), seq["small"])
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["passing", "normal"])
def test_capacity_refusals_on_every_path(data, seq, kind):
    """passing: a pass-through cloud of more than max_voxels points; normal: a grid with more than max_voxels voxels."""
    s, t = data[kind]
    fp = _fp(kind)
    # the pair that is not refused, at the refused pair's leaf, on a handle with room for everything
    fits = data["tiny" if kind == "passing" else "small"]
    hw = ql.Handle(0, **LIMITS)
    try:
        ok = hw.register_pair(*fits, fp)
    finally:
        hw.close()
    h = ql.Handle(0, n_slots=4, **SMALL)
    try:
        with pytest.raises(ql.QuatroHipError) as e:
            h.register_pair(s, t, fp)
        assert e.value.code == ql.QTR_ERR_CAPACITY and "max_voxels" in str(e.value)
        _same(h.register_pair(*fits, fp), ok)
        with pytest.raises(ql.QuatroHipError) as e:
            h.keyframe(s, fp)
        assert e.value.code == ql.QTR_ERR_CAPACITY and "max_voxels" in str(e.value)
        # the whole text on every path: the counts of both clouds for a pair, of the one cloud for a keyframe
        if kind == "passing":
            text = "voxel grid would overflow int32 (leaf too small): the cloud passes through as it is (pcl::VoxelGrid), " \
                   "and its %s points exceed max_voxels=1024"
            pair, one = "%d / %d" % (s.shape[0], t.shape[0]), ["%d" % p.shape[0] for p in (s, t)]
        else:
            text = "voxel count %s exceeds max_voxels=1024"
            n = (seq[kind]["n_src"], seq[kind]["n_tgt"])
            pair, one = "(%d,%d)" % n, ["%d" % k for k in n]
        assert _refusal(h, lambda: h.register_pair(s, t, fp)) == (ql.QTR_ERR_CAPACITY, text % pair)
        assert _refusal(h, lambda: h.register_pair_corr(s, t, *_corr300(), fp)) == (ql.QTR_ERR_CAPACITY, text % pair)
        assert _refusal(h, lambda: h.keyframe(s, fp)) == (ql.QTR_ERR_CAPACITY, text % one[0])
        assert _refusal(h, lambda: h.keyframe(t, fp)) == (ql.QTR_ERR_CAPACITY, text % one[1])
        with h.keyframe(fits[0], fp) as ks, h.keyframe(fits[1], fp) as kt:
            _same(h.register_keyframes(ks, kt, fp), ok)
        got = h.register_batch([(*fits, 2), (s, t, 2), (*fits, 2)], fp)
        assert got[1]["status"] == ql.QTR_ERR_CAPACITY and not got[1]["valid"]
        _same(got[0], ok)
        _same(got[2], ok)
        _same(h.register_batch([(*fits, 2)], fp)[0], ok)  # the lane and its slots after the refusal
    finally:
        h.close()


def test_refusals_in_front_of_the_first_launch_on_every_path(data):
    """max_points, an empty cloud, normal_radius > fpfh_radius: the same status and the same text from qtr_register_pair,
    qtr_register_pair_corr and qtr_keyframe_create — in that order when a pair has more than one reason — and the slot
    goes on as before."""
    s, t = data["normal"]
    small = data["tiny"]
    fp = _fp("normal")
    hw = ql.Handle(0, **LIMITS)
    try:
        ok = hw.register_pair(*small, fp)
    finally:
        hw.close()
    bad = ql.default_frontend_params(seed=2, normal_radius=2.0, fpfh_radius=1.0)
    empty = np.zeros((0, 4), dtype=np.float32)
    corr = _corr300()
    lim = dict(max_points=4096, max_voxels=1024, max_corr=8192)
    assert min(s.shape[0], t.shape[0]) > lim["max_points"] >= max(p.shape[0] for p in small)
    h = ql.Handle(0, **lim)
    try:
        points = (ql.QTR_ERR_CAPACITY, "cloud exceeds max_points=4096")
        nothing = (ql.QTR_ERR_BAD_ARG, "Invalid or empty point cloud dataset given!")
        radius = (ql.QTR_ERR_BAD_ARG, "[FPFHManager]: Normal should be lower than fpfh_radius!!!!")
        for a, b in ((s, t), (small[0], t), (s, small[1])):  # either cloud of a pair
            assert _refusal(h, lambda: h.register_pair(a, b, fp)) == points
            assert _refusal(h, lambda: h.register_pair_corr(a, b, *corr, fp)) == points
        assert _refusal(h, lambda: h.keyframe(s, fp)) == points
        for a, b in ((empty, empty), (empty, small[1]), (small[0], empty), (empty, t), (s, empty)):  # empty before max_points
            assert _refusal(h, lambda: h.register_pair(a, b, fp)) == nothing
            assert _refusal(h, lambda: h.register_pair_corr(a, b, *corr, fp)) == nothing
        assert _refusal(h, lambda: h.keyframe(empty, fp)) == nothing
        for a, b in ((small[0], small[1]), (empty, small[1]), (s, t)):  # the radii before everything else
            assert _refusal(h, lambda: h.register_pair(a, b, bad)) == radius
            assert _refusal(h, lambda: h.register_pair_corr(a, b, *corr, bad)) == radius
        for a in (small[0], empty, s):
            assert _refusal(h, lambda: h.keyframe(a, bad)) == radius
        _same(h.register_pair(*small, fp), ok)
    finally:
        h.close()


@pytest.mark.parametrize("host_mem", [True, False])
def test_register_pair_corr_equals_a_batch_of_scans_with_given_correspondences(data, seq, host_mem):
    """A long-list pair and a normal (tiny) pair, both with 1500 given correspondences, on a fresh handle: the long-list pair takes
    the batch's per-pair fallback, which is qtr_register_pair_corr's path.  The batch's record has no field for the
    matcher's own count: n_matched of the single call is compared with the matcher's count of qtr_register_pair."""
    corr = synth.correspondences(1500, 0.1, seed=3, noise=0.1)[:2]
    fp = _fp("long")
    kinds = ("long", "tiny")
    ref = ql.Handle(0, **LIMITS)
    try:
        matched = {k: ref.register_pair(*data[k], fp)["L"] for k in kinds}
        assert matched["long"] == seq["long"]["L"]
        want = {k: ref.register_pair_corr(*data[k], corr[0], corr[1], fp) for k in kinds}
        back = ref.solve(corr[0], corr[1])
    finally:
        ref.close()
    for k in kinds:
        assert want[k]["n_matched"] == matched[k] and want[k]["L"] == 1500
        assert np.array_equal(want[k]["T"], back["T"]) and np.array_equal(want[k]["clique"], back["clique"])
    h = ql.Handle(0, n_slots=4, **LIMITS)  # fresh: its first grouped chain runs without the long-list launch
    try:
        if host_mem:
            got = h.register_batch([(*data[k], 2, corr[0], corr[1]) for k in kinds], fp)
        else:
            items = _dev_items([data[k] for k in kinds], fp, corr)
            got = h.register_batch_dev(items, ql.demo_params(), fp, corr=True)
            res = ql.Result()  # the single call on device scans and device correspondences, after the batch
            it = items[0]
            rc = h.register_pair_corr_dev(it["src"].data_ptr(), it["src"].shape[0], it["tgt"].data_ptr(), it["tgt"].shape[0],
                                          fp, it["cs"].data_ptr(), it["ct"].data_ptr(), 1500, ql.demo_params(), res)
            assert rc == want["long"]["status"]
            assert (res.n_src, res.n_tgt, res.n_corr) == (want["long"]["n_src"], want["long"]["n_tgt"], 1500)
            assert np.array_equal(np.array(res.T[:]).reshape(4, 4), want["long"]["T"])
    finally:
        h.close()
    for g, k in zip(got, kinds):
        _same(g, want[k], lists=host_mem)
