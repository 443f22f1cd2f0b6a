"""The continuous-time registration's contract (include/qtr_vmap_ct_math.h) on the host: the restated loop
(tests/vmap_ct_ref/vmap_ct_ref.cpp over a RefMap) against an independent restatement in Python floats, the anchor — all times
at t_end IS the rigid map registration, bit for bit —, the Jacobian's stated bound, the header's two entry points and layout, the
glue of quatro_amd.api, and the accuracy of the method against today's path, computed by the restatements."""
import ctypes
import types

import numpy as np
import pytest

import deskew_cases as DC
import deskew_restate as D
import ext_abi
import icp_restate as R
import vmap_ct_cases as K
import vmap_ct_restate as CT
import vmap_restate as M

TWO = {"qtr_voxel_map_register_ct", "qtr_voxel_map_ct_pose_at"}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def small():
    pts, nrm, pose = K.small_map()
    ref = M.RefMap(K.SIDE, 1 << 14)
    ref.insert(pts, nrm, pose)
    assert 100 < len(ref) < 1000
    return ref


def test_per_point_pose_and_terms_equal_the_python_restatement_bit_for_bit(small):
    """Interval, pose, q, lever, s, key and all 32 terms of every point of the 513-point edge cloud (its first rows sit on
    the named times: t_end, t_begin, the float32 just inside and outside each, far outside, NaN, inf), under two iterates."""
    s, sn, t, _, _ = K.edge_cloud(513)
    f = small.fetch_all()
    rec_of = {M.key(*c): (r, int(n)) for c, r, n in zip(f[M.COORDS], f[M.RECORDS], f[M.COUNT])}
    matched = flagged = 0
    for E in (K.GUESS_END, K.BEGIN @ R.rigid(R.rot(0.2, -0.3, 0.5), [0.5, 0.2, -0.1])):
        ok, iv = CT.py_interval(K.T_BEGIN, K.T_END, K.BEGIN, E)
        assert ok
        for i in range(s.shape[0]):
            probe = CT.point(K.T_BEGIN, K.T_END, K.BEGIN, E, s[i, :3], sn[i, :3], t[i], K.SIDE)
            rec, n = rec_of.get(probe["key"], (None, 0)) if probe["ok"] else (None, 0)
            got = CT.point(K.T_BEGIN, K.T_END, K.BEGIN, E, s[i, :3], sn[i, :3], t[i], K.SIDE, rec, n)
            want = CT.py_point(iv, s[i, :3], sn[i, :3], t[i], K.SIDE, rec, n)
            assert got["admitted"] and got["flags"] == want["flags"] and got["ok"] == want["ok"], i
            flat = np.concatenate([[iv["tau"], iv["div"]], iv["R"], iv["c"], iv["dc"], iv["w"]])
            assert np.array_equal(_bits(got["iv"]), _bits(flat)), i
            if want["flags"] == CT.SKIPPED:
                assert not got["ok"]
                flagged += 1
                continue
            for k in ("T", "q", "r", "terms"):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (i, k)
            assert _bits([got["s"]])[0] == _bits([want["s"]])[0] and got["key"] == want["key"], i
            matched += rec is not None
    assert matched > 500 and flagged == 12
    # the named times say what they are named for
    for (tt, sk, ex), i in zip(K.named_times(), range(len(K.named_times()))):
        fl = CT.point(K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, s[i, :3], sn[i, :3], tt, K.SIDE)["flags"]
        assert fl == (CT.SKIPPED if sk else CT.EXTRAPOLATED if ex else 0), (i, tt)
    on_end = CT.point(K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, s[0, :3], sn[0, :3], np.float32(K.T_END), K.SIDE)
    on_begin = CT.point(K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, s[0, :3], sn[0, :3], np.float32(K.T_BEGIN), K.SIDE)
    assert on_end["s"] == 1.0 and on_begin["s"] == 0.0
    assert np.array_equal(_bits(on_end["T"]), _bits(K.GUESS_END.reshape(16)[:12]))  # u = 0: the point moves by exactly E
    assert np.abs(on_begin["T"] - K.BEGIN.reshape(16)[:12]).max() < 1e-14            # u = 1: by B, up to the Log / Exp round trip


def test_pose_at_follows_the_rule_and_refuses_what_the_interval_refuses():
    B, E = K.BEGIN, K.GUESS_END
    assert np.array_equal(_bits(CT.pose_at(K.T_BEGIN, K.T_END, B, E, K.T_END)), _bits(E))
    assert np.abs(CT.pose_at(K.T_BEGIN, K.T_END, B, E, K.T_BEGIN) - B).max() < 1e-14
    mid = CT.pose_at(K.T_BEGIN, K.T_END, B, E, 0.5 * (K.T_BEGIN + K.T_END))
    kt, kp = np.array([K.T_BEGIN, K.T_END]), np.stack([B, E])
    assert np.abs(mid - D.model_pose_at(kt, kp, 0.5 * (K.T_BEGIN + K.T_END))).max() < 1e-13  # (numpy's sin / cos model)
    far = B @ R.rigid(R.rot(0.0, 0.0, np.radians(100.0)), [0.0, 0.0, 0.0])
    assert CT.pose_at(K.T_BEGIN, K.T_END, B, far, K.T_END) is None
    assert CT.pose_at(K.T_BEGIN, K.T_END, B, B @ R.rigid(R.rot(0.0, 0.0, np.radians(89.0)), [0, 0, 0]), K.T_END) is not None


@pytest.mark.parametrize("n", [1, 257, 513])
def test_all_times_at_t_end_is_the_rigid_registration_bit_for_bit(small, n):
    """The anchor, for three unrelated begin poses: T, iterations, stop reason and every trace row."""
    s, sn, _, _, _ = K.edge_cloud(n)
    te = np.full(n, np.float32(K.T_END))
    assert float(te[0]) == K.T_END  # (a binary32 value: the time sits ON the end)
    for kw in (dict(teps=0.0, feps=0.0, max_iter=8), dict(max_iter=30)):
        want = small.register(s, sn, K.GUESS_END, **kw)
        for B in K.ANCHOR_BEGINS:
            got = CT.register_ct(small, s, sn, te, K.T_BEGIN, K.T_END, B, K.GUESS_END, **kw)
            assert np.array_equal(_bits(got["T"]), _bits(want["T"]))
            assert (got["iterations"], got["stop_reason"], got["n_corr"], got["valid"]) == \
                   (want["iterations"], want["stop_reason"], want["n_corr"], want["valid"])
            assert np.array_equal(_bits(got["trace"]), _bits(want["trace"])) and np.array_equal(got["corr"], want["corr"])
            assert _bits([got["fitness"], got["rmse"]]).tolist() == _bits([want["fitness"], want["rmse"]]).tolist()
            assert got["info"] == {"n_points": n, "n_skipped": 4 if n >= 255 else 0, "n_extrapolated": 0}  # (points, normals)
    if n == 513:
        assert want["iterations"] >= 3 and want["valid"]


def test_the_loop_counts_skips_and_extrapolations_and_stops_where_it_must(small):
    s, sn, t, n_skip, n_extra = K.edge_cloud(513)
    r = CT.register_ct(small, s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, teps=0.0, feps=0.0, max_iter=6)
    assert r["info"] == {"n_points": 513, "n_skipped": n_skip, "n_extrapolated": n_extra} and (n_skip, n_extra) == (6, 5)
    assert r["iterations"] == 6 and r["valid"] and r["stop_reason"] == CT.STOP_MAX_ITERATIONS
    named = K.named_times()
    for i, (tt, sk, ex) in enumerate(named):
        assert r["corr"][i] == (-1 if sk else 0), (i, tt)  # an extrapolated point is still matched
    k = len(named)
    assert (r["corr"][k:k + 4] == -1).all() and (r["corr"][k + 4:k + 9] == -1).all()
    assert r["n_corr"] == int((r["corr"] == 0).sum())
    # no voxel anywhere: too few correspondences, T stays the guess
    away = s.copy()
    away[:, :3] += np.float32(500.0)
    e = CT.register_ct(small, away, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END)
    assert e["stop_reason"] == CT.STOP_TOO_FEW and not e["valid"] and e["n_corr"] == 0 and e["iterations"] == 0
    assert np.array_equal(_bits(e["T"]), _bits(K.GUESS_END))
    # an iterate the interval refuses gives no point a correspondence: the same stop
    far = K.BEGIN @ R.rigid(R.rot(0.0, 0.0, np.radians(120.0)), [0.0, 0.0, 0.0])
    e = CT.register_ct(small, s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, far)
    assert e["stop_reason"] == CT.STOP_TOO_FEW and e["n_corr"] == 0 and (e["corr"] == -1).all()
    one = CT.register_ct(small, s, sn, t, K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, max_iter=1)
    assert one["iterations"] == 1 and one["stop_reason"] == CT.STOP_MAX_ITERATIONS
    assert np.array_equal(_bits(one["trace"][0]), _bits(r["trace"][0]))


def test_the_jacobian_is_within_the_bound_the_header_states():
    """Central differences of q under a left increment on E against s [-[r]x | I], on a sweep that turns by 3 degrees.  The
    header's bound: |gap|_2 <= u |p| ((1 - u) |w| / 2 + |w|^2) in the rotation block, nothing in the translation block.  The
    differences themselves are good to about 25 eps |q| / h (rounding; truncation h^2 |q| is far below): 1e-7 at h = 1e-6."""
    B = K.BEGIN
    E = B @ R.rigid(DC.rot([0.3, -0.5, 1.0], np.radians(3.0)), [0.9, 0.1, -0.05])
    ok, iv = CT.py_interval(K.T_BEGIN, K.T_END, B, E)
    w = float(np.linalg.norm(iv["w"]))
    assert ok and abs(np.degrees(w) - 3.0) < 1e-9
    h, fd_tol = 1e-6, 1e-7
    rng = np.random.default_rng(3)
    worst = 0.0
    for u in (0.0, 0.25, 0.5, 0.75, 1.0):
        t = np.float32(K.T_END + u * (K.T_BEGIN - K.T_END))  # (the ends and the quarter points are float32 values)
        for _ in range(4):
            p = rng.normal(size=3) * 12.0
            a = np.array([0.0, 0.0, 1.0])
            base = CT.point(K.T_BEGIN, K.T_END, B, E, p, a, t, K.SIDE)
            assert base["s"] == 1.0 - u
            r, s = base["r"], base["s"]
            Ja = s * np.hstack([-D.hat(r), np.eye(3)])
            Jfd = np.zeros((3, 6))
            for k in range(6):
                q = []
                for sign in (1.0, -1.0):
                    d = np.zeros(6)
                    d[k] = sign * h
                    inc = R.rigid(D.model_exp(d[:3]), d[3:])
                    q.append(CT.point(K.T_BEGIN, K.T_END, B, inc @ E, p, a, t, K.SIDE)["q"])
                Jfd[:, k] = (q[0] - q[1]) / (2 * h)
            lever = float(np.linalg.norm(np.float32(p).astype(np.float64)))
            gap = float(np.linalg.norm(Jfd[:, :3] - Ja[:, :3], 2))
            bound = u * lever * ((1.0 - u) * w / 2.0 + w * w)
            worst = max(worst, gap / lever)
            assert gap <= bound + fd_tol, (u, gap, bound)
            assert np.linalg.norm(Jfd[:, 3:] - Ja[:, 3:], 2) <= fd_tol, u
            if u == 0.0:
                assert gap <= fd_tol  # the rigid Jacobian
    print(f"Jacobian: worst gap over the lever {worst:.3e} (the first-order term allows {w / 8:.3e} at u = 1/2)")
    assert 0.1 * w / 8 < worst <= w / 8 + w * w  # (the gap is there, and of the size the first-order term says)


def test_the_extension_library_exports_the_headers_two_names_and_pose_at_is_the_restatement():
    from quatro_amd import lib as ql
    assert ext_abi.check_header("quatro_voxelmap_ct.h") == TWO  # declared, listed, exported by libquatro_ext.so alone
    hip, _ = ext_abi.libraries()
    assert set(ql.VMAP_CT_EXPORTS) == TWO
    assert not (ext_abi.table(hip) & TWO) and not (set(ql.EXPORTS) & TWO)
    # the ctypes mirror against sizeof / offsetof of the compiled header
    got = np.zeros(4, np.int32)
    CT.load().vmap_ct_ref_layout(got.ctypes.data)
    I = ql.VmapCtInfo
    assert list(got) == [ctypes.sizeof(I), I.n_points.offset, I.n_skipped.offset, I.n_extrapolated.offset] == [12, 0, 4, 8]
    # the host-only entry point runs without a device and is the restatement's
    T = ql.ct_pose_at(K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, 0.3)
    assert np.array_equal(_bits(T), _bits(CT.pose_at(K.T_BEGIN, K.T_END, K.BEGIN, K.GUESS_END, 0.3)))
    with pytest.raises(ValueError):
        ql.ct_pose_at(K.T_END, K.T_BEGIN, K.BEGIN, K.GUESS_END, 0.3)
    with pytest.raises(ValueError):
        ql.ct_pose_at(K.T_BEGIN, K.T_END, K.BEGIN, K.BEGIN @ R.rigid(R.rot(0, 0, 2.0), [0, 0, 0]), 0.3)


def test_sample_sweep_takes_the_first_raw_point_of_every_voxel():
    from quatro_amd import api
    raw = np.array([[0.1, 0.1, 0.1, 7.0], [0.2, 0.2, 0.2, 8.0], [np.nan, 0.0, 0.0, 1.0], [-0.1, 0.1, 0.1, 2.0],
                    [1.3, 0.0, 0.0, 3.0], [0.0, np.inf, 0.0, 4.0], [-0.4, 0.4, 0.4, 5.0], [0.49, 0.49, 0.49, 6.0],
                    [0.5, 0.0, 0.0, 9.0]], np.float32)
    times = (np.arange(9, dtype=np.float32) + np.float32(0.1)) / np.float32(7.0)
    pts, ts = api.sample_sweep(raw, times, 0.5)
    assert np.array_equal(pts.view(np.uint32), raw[[0, 3, 4, 8]].view(np.uint32))  # raw points, never centroids
    assert np.array_equal(ts.view(np.uint32), times[[0, 3, 4, 8]].view(np.uint32))  # ... and their times, unaltered
    assert pts.dtype == np.float32 and ts.dtype == np.float32
    e, et = api.sample_sweep(raw[[2, 5]], times[[2, 5]], 0.5)
    assert e.shape == (0, 4) and et.shape == (0,)
    with pytest.raises(ValueError):
        api.sample_sweep(raw, times[:3], 0.5)
    rng = np.random.default_rng(1)
    big = rng.uniform(-20, 20, (5000, 4)).astype(np.float32)
    bt = rng.random(5000).astype(np.float32)
    pts, ts = api.sample_sweep(big, bt, 1.0)
    vox = np.floor(big[:, :3].astype(np.float64))
    seen, keep = set(), []
    for i, v in enumerate(map(tuple, vox)):
        if v not in seen:
            seen.add(v)
            keep.append(i)
    assert np.array_equal(pts, big[keep]) and np.array_equal(ts, bt[keep])


class FakeKf:
    def __init__(self, log, **kw):
        self.kw, self.log = kw, log

    def close(self):
        self.log.append(("close",))


class FakeMap:
    def __init__(self, log, valid):
        self.log, self.valid, self.n = log, valid, 0

    def register_ct(self, pts, normals, ts, t_begin, t_end, begin, guess, icp):
        self.log.append(("register_ct", pts.shape[0], ts.copy(), t_begin, t_end, np.array(begin), np.array(guess), icp))
        ok = self.valid[self.n]
        self.n += 1
        return {"valid": ok, "T": np.array(guess) @ R.rigid(R.rot(0.0, 0.0, 0.01), [0.05, 0.0, 0.0])}

    def insert_keyframe(self, kf, pose):
        self.log.append(("insert", kf, np.array(pose)))

    def evict(self, centre, radius):
        self.log.append(("evict", np.array(centre), radius))

    def destroy(self):
        self.log.append(("destroy",))


class FakeHandle:
    def __init__(self, valid):
        self.log, self.map = [], None
        self.valid = valid

    def voxel_map(self, voxel_size, capacity):
        self.map = FakeMap(self.log, self.valid)
        return self.map

    def fpfh(self, pts, r_normal, r_fpfh):
        self.log.append(("fpfh", pts.shape[0], r_normal, r_fpfh))
        return np.zeros_like(pts), None

    def keyframe(self, raw, fp, times=None, knot_times=None, knot_poses=None, t_ref=None):
        self.log.append(("keyframe", np.array(knot_times), np.array(knot_poses), t_ref))
        return FakeKf(self.log, times=times)


def test_continuous_time_odometry_over_a_fake_handle():
    from quatro_amd import api
    rng = np.random.default_rng(5)
    scans = [rng.uniform(-10, 10, (400, 4)).astype(np.float32) for _ in range(4)]
    times = [rng.uniform(0, 0.1, 400).astype(np.float32) for _ in range(4)]
    fp = types.SimpleNamespace(voxel_size=2.0, normal_radius=0.5, fpfh_radius=0.7)
    with pytest.raises(ValueError, match="continuous_time needs times"):
        api.scan_to_map_odometry(FakeHandle([]), scans, fp, continuous_time=True)
    with pytest.raises(ValueError, match="sweep_period"):
        api.scan_to_map_odometry(FakeHandle([]), scans, fp, times=times, continuous_time=True)
    h = FakeHandle([True, False, True])
    poses, vm = api.scan_to_map_odometry(h, scans, fp, voxel_size=1.0, times=times, sweep_period=0.1, window_radius=30.0,
                                         continuous_time=True, icp="the icp params")
    assert vm is h.map and poses.shape == (4, 4, 4)
    step = R.rigid(R.rot(0.0, 0.0, 0.01), [0.05, 0.0, 0.0])
    regs = [e for e in h.log if e[0] == "register_ct"]
    kfs = [e for e in h.log if e[0] == "keyframe"]
    ins = [e for e in h.log if e[0] == "insert"]
    assert len(regs) == 3 and len(kfs) == 4 and len(ins) == 4 and sum(e[0] == "close" for e in h.log) == 4
    ends = [np.eye(4)]  # E_0: the end of an identity motion
    for k in range(1, 4):
        begin = ends[-1]
        guess = api.constant_velocity_guess(poses[k - 1], begin)
        _, n, ts, t0, t1, B, G, icp = regs[k - 1]
        want_pts, want_ts = api.sample_sweep(scans[k], times[k], 2.0)
        assert n == want_pts.shape[0] and np.array_equal(ts, want_ts) and (t0, t1) == (0.0, 0.1) and icp == "the icp params"
        assert np.array_equal(B, begin) and np.array_equal(G, guess)
        ends.append(guess @ step if h.valid[k - 1] else guess)  # an invalid registration keeps its guess
    for k in range(4):
        begin = np.eye(4) if k == 0 else ends[k - 1]
        assert np.array_equal(poses[k], begin)  # the returned poses are the sweep starts
        assert np.array_equal(kfs[k][1], [0.0, 0.1]) and kfs[k][3] == 0.0
        assert np.array_equal(kfs[k][2][0], begin) and np.array_equal(kfs[k][2][1], ends[k])  # deskewed under (B_k, E_k)
        assert np.array_equal(ins[k][2], begin)  # inserted under B_k
    assert np.array_equal(regs[0][6], np.eye(4))  # sweep 1 starts from the identity motion
    assert [e[1:] for e in h.log if e[0] == "fpfh"] == [(r[1], 0.5, 0.7) for r in regs]
    assert sum(e[0] == "evict" for e in h.log) == 4 and ("destroy",) not in h.log


@pytest.fixture(scope="module")
def accuracy():
    """The three end poses of both accuracy cases, computed once: (a) register_ct from the wrong guess, (b) today's path —
    the sweep deskewed under the WRONG constant-velocity knots, registered rigidly, its end pose the result times the guessed
    motion —, (c) the same under the TRUE knots: the floor."""
    out = {}
    for case in K.ACC_CASES:
        sc = K.accuracy_scene(case)
        m = M.RefMap(1.0, 1 << 16)
        m.insert(sc["world"], sc["world_normals"], None)
        B, Mt, Mg = sc["begin"], sc["true_motion"], sc["guess_motion"]
        want = B @ Mt
        a = CT.register_ct(m, sc["raw"], sc["normals"], sc["times"], 0.0, K.PERIOD, B, B @ Mg)
        errs = {"a": K.pose_error(a["T"], want), "guess": K.pose_error(B @ Mg, want)}
        for name, motion in (("b", Mg), ("c", Mt)):
            kt, kp = DC.two_knots(motion, K.PERIOD)
            flat, _ = D.deskew(sc["raw"], sc["times"], kt, kp, 0.0)
            r = m.register(flat, sc["normals"], B)
            assert r["valid"]
            errs[name] = K.pose_error(r["T"] @ motion, want)
        assert a["valid"] and a["info"] == {"n_points": sc["raw"].shape[0], "n_skipped": 0, "n_extrapolated": 0}
        out[sc["name"]] = errs
    return out


@pytest.mark.parametrize("name", [c[0] for c in K.ACC_CASES])
def test_the_end_pose_beats_todays_path_and_stays_near_the_floor(accuracy, name):
    """End-pose errors (metres, degrees) measured by the restatements, as written into DESIGN.md section 22:
      speed change     guess 0.4000 / 0.000   (a) 0.0111 / 0.109   (b) 0.2362 / 1.008   (c) 0.0075 / 0.082
      yaw-rate change  guess 0.0000 / 2.000   (a) 0.0157 / 0.180   (b) 0.0264 / 0.371   (c) 0.0076 / 0.082
    (a) must beat (b) strictly in both.  Against the floor (c) the margin is twice (c)'s own error, (a) <= 3 (c): the end pose
    is seen through the weights s^2 of the points, whose mean over a sweep is 1/3, so it carries a third of the information the
    rigid fit has of its pose and the same noise moves it sqrt(3) times as far; the rest of the margin is for the source
    normals, which are the begin frame's and up to the sweep's own rotation off for late points — (c)'s cloud does not have
    that, and the yaw case shows it."""
    e = accuracy[name]
    print(f"{name}: guess {e['guess']}, (a) {e['a']}, (b) {e['b']}, (c) {e['c']}")
    assert e["a"][0] < e["b"][0] and e["a"][1] < e["b"][1]
    assert e["a"][0] <= 3.0 * e["c"][0] and e["a"][1] <= 3.0 * e["c"][1]
