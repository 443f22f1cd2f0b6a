"""No-GPU checks of the submap keyframes: include/qtr_submap_math.h compiled for the host equals the numpy restatement
(tests/submap_restate.py) bit for bit; qtr_keyframe_merge is exported, bound and refuses its arguments before it touches a
device; api.make_submap / api.close_loop pick the windows and the relative poses the contract states; and
synth.kitti64_trajectory is deterministic, consistent with its poses, and leaves the older generators' bytes alone."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import submap_restate as sr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from quatro_amd import build as qbuild
    qbuild.build(force=False, verbose=False)
    from quatro_amd import lib as ql
    return ql.load()


# ---- the contract header ----------------------------------------------------------------------------------------------
def _random_pose(rng, scale=50.0):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-scale, scale, 3)
    return T


def test_header_compiled_for_the_host_equals_the_float64_restatement():
    src = r'''
#include "qtr_submap_math.h"
extern "C" {
void move(const double* T, const float* in, int n, float* out) {
  for (int i = 0; i < n; ++i) {
    qtr_submap_point(T, in[4 * i], in[4 * i + 1], in[4 * i + 2], out + 4 * i, out + 4 * i + 1, out + 4 * i + 2);
    out[4 * i + 3] = in[4 * i + 3];
  }
}
int pose_ok(const double* T) { return qtr_submap_pose_finite(T); }
}
'''
    rng = np.random.default_rng(12)
    n = 20000
    # magnitudes 1e-3 .. 1e3 of either sign, w = arbitrary bit patterns that are not NaNs (a NaN's payload is the one thing a
    # float assignment on the host may touch; the kernel copies the 128-bit record)
    pts = (10.0 ** rng.uniform(-3, 3, (n, 4)) * rng.choice([-1.0, 1.0], (n, 4))).astype(np.float32)
    pts[:, 3] = rng.integers(0, 0x7f800000, n, dtype=np.uint32).view(np.float32)
    poses = [("identity", np.eye(4))] + [(f"random {k}", _random_pose(rng)) for k in range(6)]
    skew = rng.standard_normal((4, 4)) * 10.0 ** rng.uniform(-2, 2, (4, 4))  # (not rigid: the contract does not ask for it)
    poses.append(("general", skew))
    # products that cancel catastrophically: T[0] x + T[1] y with x ~ y leaves the last bits of two 1e11-sized products
    cancel = np.eye(4)
    cancel[0] = [1.0e8, -1.0e8, 1.0, 0.5]
    cancel[1] = [-(1.0 + 2.0 ** -30) * 3.0e7, 3.0e7, -3.0e7 * 2.0 ** -30, 1.0e-3]
    poses.append(("cancelling", cancel))
    near = pts.copy()
    near[:, 1] = near[:, 0] * (1.0 + rng.integers(-3, 4, n) * np.float32(2.0 ** -23))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, so = os.path.join(tmp, "m.cpp"), os.path.join(tmp, "m.so")
        open(cpp, "w").write(src)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), cpp,
                               "-o", so])
        m = C.CDLL(so)
        for name, T in poses:
            T16 = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
            for cloud in (pts, near):
                got = np.zeros_like(cloud)
                m.move(T16.ctypes.data_as(C.c_void_p), cloud.ctypes.data_as(C.c_void_p), n, got.ctypes.data_as(C.c_void_p))
                assert np.array_equal(bits32(got), bits32(sr.transform(T, cloud))), name
                if name == "identity":  # the record comes back as it went in, w included
                    assert np.array_equal(bits32(got), bits32(cloud))
        # (the cancelling pose is not vacuous: most of its x coordinates lost more than 20 bits to the subtraction)
        x = sr.transform(cancel, near)[:, 0].astype(np.float64)
        assert np.median(np.abs(x) / (1.0e8 * np.abs(near[:, 0].astype(np.float64)))) < 2.0 ** -20
        ok = np.eye(4).reshape(16)
        assert m.pose_ok(ok.ctypes.data_as(C.c_void_p)) == 1
        for k in range(16):
            for v in (np.nan, np.inf, -np.inf):
                bad = ok.copy()
                bad[k] = v
                assert m.pose_ok(bad.ctypes.data_as(C.c_void_p)) == (0 if k < 12 else 1), (k, v)  # row 3 is ignored


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_merge_is_exported_and_bound(lib):
    from quatro_amd import lib as ql
    assert "qtr_keyframe_merge" in ql.EXPORTS and hasattr(lib, "qtr_keyframe_merge")
    assert lib.qtr_keyframe_merge.argtypes is not None and len(lib.qtr_keyframe_merge.argtypes) == 7
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    assert "#define QTR_SUBMAP_MAX_KEYFRAMES 64" in hdr and ql.SUBMAP_MAX_KEYFRAMES == 64


def test_merge_refuses_its_arguments_without_a_device(lib):
    from quatro_amd import lib as ql
    fp, bad = ql.default_frontend_params(), ql.QTR_ERR_BAD_ARG
    members = (C.c_void_p * 65)()
    poses = np.tile(np.eye(4).reshape(16), (65, 1))
    for K in (0, 1, 65):
        out = C.c_void_p(1234)
        assert lib.qtr_keyframe_merge(None, 0, members, poses.ctypes.data, K, C.byref(fp), C.byref(out)) == bad, K
        assert not out, K  # *out = NULL on every failure
        assert lib.qtr_keyframe_merge(None, 0, members, None, K, C.byref(fp), None) == bad, K
        assert lib.qtr_keyframe_merge(None, 0, None, None, K, None, C.byref(out)) == bad, K


# ---- make_submap / close_loop against a handle that records its calls --------------------------------------------------------
class FakeKf:
    def __init__(self, name):
        self.name, self.closed = name, 0

    def close(self):
        self.closed += 1


class FakeHandle:
    def __init__(self):
        self.merges, self.made, self.pairs = [], [], None

    def merge_keyframes(self, kfs, poses=None, fp=None, slot=0):
        self.merges.append((list(kfs), np.array(poses), fp, slot))
        self.made.append(FakeKf(f"submap{len(self.made)}"))
        return self.made[-1]

    def register_batch_keyframes(self, pairs, fp, params, icp):
        self.pairs = pairs
        out = [{"valid": True, "n_final": 10 + 5 * (k == 1)} for k in range(len(pairs))]
        return out if icp is None else (out, [{"status": 0}] * len(pairs))


class FakeIndex:
    def __init__(self, ids, size):
        self.ids, self.size = ids, size

    def __len__(self):
        return self.size

    def query(self, kf, k, id_lo, id_hi):
        self.args = (kf, k, id_lo, id_hi)
        return [{"id": i, "shift": 0, "distance": 0.1 * n, "yaw": 0.0} for n, i in enumerate(self.ids[:k])]


def _poses(n, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([_random_pose(rng) for _ in range(n)])


def test_make_submap_clips_its_window_and_moves_the_members_into_the_centre_frame():
    from quatro_amd import api
    kfs, P = [f"kf{i}" for i in range(12)], _poses(12)
    cases = [  # (centre, half width, id_lo, id_hi) -> member ids
        ((5, 2, 0, None), [3, 4, 5, 6, 7]),
        ((1, 3, 0, None), [0, 1, 2, 3, 4]),        # clipped at the low end
        ((10, 3, 0, None), [7, 8, 9, 10, 11]),     # ... at the high end (len(keyframes))
        ((5, 4, 3, 8), [3, 4, 5, 6, 7]),           # ... by id_lo / id_hi
        ((7, 2, 0, 8), [5, 6, 7]),
        ((4, 0, 0, None), [4]),
        ((0, 25, 0, None), list(range(12))),
    ]
    for (c, w, lo, hi), want in cases:
        h = FakeHandle()
        fp = object()
        got = api.make_submap(h, kfs, P, c, w, fp, lo, hi, slot=1)
        (members, rel, fp_seen, slot), = h.merges
        assert got is h.made[0] and members == [f"kf{i}" for i in want] and fp_seen is fp and slot == 1, (c, w, lo, hi)
        assert rel.dtype == np.float64 and rel.shape == (len(want), 4, 4)
        inv_c = np.linalg.inv(P[c])
        for r, i in zip(rel, want):
            assert np.array_equal(r, inv_c @ P[i]), (c, i)  # float64 equality
    with pytest.raises(ValueError):
        api.make_submap(FakeHandle(), kfs, P, 9, 2, None, 0, 8)  # the centre itself is outside the range


def test_close_loop_defaults_make_the_calls_they_made_before():
    from quatro_amd import api
    from quatro_amd import lib as ql
    h, ix = FakeHandle(), FakeIndex([4, 9, 2, 7], 12)
    kfs = [f"kf{i}" for i in range(12)]
    fp = ql.FrontendParams(0.3, 0.5, 0.75, 0.95, 1, 1, 5)
    r = api.close_loop(h, ix, kfs, "q", 3, id_lo=1, id_hi=10, fp=fp)
    assert ix.args == ("q", 3, 1, 10) and h.merges == []
    assert h.pairs == [("q", "kf4", 5), ("q", "kf9", 5), ("q", "kf2", 5)]
    assert (r["best"], r["best_id"]) == (1, 9) and "refined" not in r
    r = api.close_loop(h, ix, kfs, "q", 3, 1, 10, fp, None, None, poses=_poses(12), submap_half_width=0)
    assert h.merges == [] and h.pairs == [("q", "kf4", 5), ("q", "kf9", 5), ("q", "kf2", 5)]


def test_close_loop_registers_submaps_clipped_to_the_searched_range_and_destroys_them():
    from quatro_amd import api
    from quatro_amd import lib as ql
    kfs, P = [f"kf{i}" for i in range(12)], _poses(12)
    fp = ql.FrontendParams(0.3, 0.5, 0.75, 0.95, 1, 1, 5)
    with pytest.raises(ValueError):
        api.close_loop(FakeHandle(), FakeIndex([4], 12), kfs, "q", 3, fp=fp, submap_half_width=2)
    h, ix = FakeHandle(), FakeIndex([4, 8, 1], 12)
    r = api.close_loop(h, ix, kfs, "q", 3, id_lo=1, id_hi=10, fp=fp, icp=object(), poses=P, submap_half_width=2)
    assert [[m for m in mem] for mem, _, _, _ in h.merges] == [[f"kf{i}" for i in ids] for ids in ([2, 3, 4, 5, 6], [6, 7, 8, 9],
                                                                                                 [1, 2, 3])]
    for (_, rel, fp_seen, _), (c, ids) in zip(h.merges, ((4, [2, 3, 4, 5, 6]), (8, [6, 7, 8, 9]), (1, [1, 2, 3]))):
        assert fp_seen is fp and all(np.array_equal(x, np.linalg.inv(P[c]) @ P[i]) for x, i in zip(rel, ids))
    assert h.pairs == [("q", h.made[0], 5), ("q", h.made[1], 5), ("q", h.made[2], 5)]
    assert [k.closed for k in h.made] == [1, 1, 1]
    assert (r["best"], r["best_id"]) == (1, 8) and len(r["refined"]) == 3
    # id_hi = None: the searched range ends with the index — keyframes beyond it (the query's neighbourhood) are not fused
    h, ix = FakeHandle(), FakeIndex([7], 9)
    api.close_loop(h, ix, kfs, "q", 1, fp=fp, poses=P, submap_half_width=3)
    assert h.merges[0][0] == [f"kf{i}" for i in (4, 5, 6, 7, 8)] and h.made[0].closed == 1

    class Failing(FakeHandle):
        def register_batch_keyframes(self, *a):
            raise RuntimeError("job failed")

    h = Failing()
    with pytest.raises(RuntimeError):
        api.close_loop(h, FakeIndex([4, 5], 12), kfs, "q", 2, fp=fp, poses=P, submap_half_width=1)
    assert [k.closed for k in h.made] == [1, 1]  # (temporary submaps do not outlive a failed job)


# ---- the synthetic trajectory ----------------------------------------------------------------------------------------------
def test_older_generators_produce_the_bytes_they_produced_before():
    """sha256 over source, target and ground truth of kitti64_pair(0), taken on the commit before kitti64_trajectory existed."""
    from quatro_amd import synth
    s, t, T = synth.kitti64_pair(0)
    assert hashlib.sha256(s.tobytes() + t.tobytes() + T.tobytes()).hexdigest() == \
        "69f82c34ed2d676783e08aeaa125e0fe5a7f21aa74c7ec215b4fd9718e52b648"


def test_trajectory_is_deterministic_and_its_poses_put_the_scans_on_one_scene(qo):
    """Consecutive scans are `step` apart; moved by their poses they occupy the same cells of the oracle's voxel grid (0.5 m),
    unmoved they do not.  The bounds: two sweeps of one static scene taken 1 m apart see the same surfaces but for what each
    occludes and for cells the 2 cm range noise splits, so most occupied cells are shared (0.7 asked; 0.88 - 0.91 seen);
    unmoved, a 1 m shift is two cells, and the overlap is what chance and surfaces parallel to the motion leave (at most half
    of the moved figure asked; 0.05 - 0.24 seen)."""
    from quatro_amd import synth
    scans, poses = synth.kitti64_trajectory(0, 7, 1.0)
    again, poses2 = synth.kitti64_trajectory(0, 7, 1.0)
    other, _ = synth.kitti64_trajectory(1, 7, 1.0)
    assert len(scans) == 8 and poses.shape == (8, 4, 4) and poses.dtype == np.float64
    assert all(np.array_equal(bits32(a), bits32(b)) for a, b in zip(scans, again)) and np.array_equal(poses, poses2)
    assert other[0].shape != scans[0].shape or not np.array_equal(other[0], scans[0])
    assert all(s.dtype == np.float32 and s.shape[1] == 4 and s.shape[0] > 20000 for s in scans)
    for i in range(6):
        assert abs(np.linalg.norm(poses[i + 1][:3, 3] - poses[i][:3, 3]) - 1.0) < 1e-9
        R = poses[i][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.array_equal(poses[i][3], [0, 0, 0, 1])
    assert np.array_equal(poses[3][:3, 3], np.zeros(3)) and np.linalg.norm(poses[7][:2, 3]) <= 0.4

    def cells(cloud, leaf=0.5):
        v = qo.voxelize(cloud, leaf)
        return set(map(tuple, np.floor(v[:, :3] / leaf).astype(np.int64)))

    def overlap(a, b):
        ka, kb = cells(a), cells(b)
        return len(ka & kb) / min(len(ka), len(kb))

    for i, j in [(k, k + 1) for k in range(6)] + [(3, 7)]:
        moved = overlap(sr.transform(poses[i], scans[i]), sr.transform(poses[j], scans[j]))
        raw = overlap(scans[i], scans[j])
        print(f"scans {i}, {j}: overlap under the poses {moved:.3f}, without {raw:.3f}")
        assert moved >= 0.7 and raw <= 0.5 * moved, (i, j, moved, raw)
