"""Sweep deskew without a GPU: include/qtr_deskew_math.h (through the g++ restatement, tests/deskew_ref/deskew_ref.cpp, and
through qtr_deskew_pose_at of libquatro_ext.so, which is host code) against a second model in numpy that shares nothing
with the header (deskew_restate.model_*: numpy's sin, cos and arctan2, 2 sin^2(th/2)/th^2 for the second Rodrigues
coefficient); the interval, skip and identity rules; every refusal; the round trip through the skew synthesiser; and the
header's entry points in the extension library's symbol table.

The asserted differences are ten times what was measured when the test was written (the project's convention); every test
prints what it measures."""
import numpy as np
import pytest

import deskew_cases as K
import deskew_restate as D

# measured -> asserted (x 10)
TOL_LOG_REL = 7.0e-15    # |Log_header - Log_model| / angle, angles 1e-12 .. pi/2: measured 6.97e-16
TOL_EXP = 8.9e-15        # entries of Exp_header - Exp_model, angles up to pi: measured 8.88e-16
TOL_ATAN_REL = 6.6e-15   # 2 atan(tan(th/2)) against th over (0, pi/2], relative: measured 6.56e-16
TOL_POSE_R = 4.5e-15     # entries of R(t), s in [-1, 2]: measured 4.44e-16
TOL_POSE_C = 0.0         # entries of c(t): measured 0 (c_j + s dc_j is the same three operations on both sides)
TOL_POINT_F64 = 5.7e-13  # output coordinates before their rounding, metres, clouds of up to 105 m: measured 5.68e-14


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _half_ulp32(x):
    """Half a float32 ulp at |x| (of the binade |x| lies in; normal numbers)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 24)


ANGLES = np.concatenate([np.logspace(-12, np.log10(K.ROTATION_LIMIT), 400), [K.ROTATION_LIMIT * (1 - 1e-12), 1.0, 0.5]])


def test_log_and_exp_against_the_numpy_model():
    rng = np.random.default_rng(1)
    worst_log = worst_exp = 0.0
    for th in ANGLES:
        axis = rng.normal(size=3)
        axis /= np.sqrt(axis @ axis)
        M = D.model_exp(axis * th)
        w = D.log(M)
        assert w is not None, th
        worst_log = max(worst_log, np.abs(w - D.model_log(M)).max() / th)
        assert np.abs(w - axis * th).max() / th < 1e-3 or th < 1e-7  # (and it is the rotation vector it was made from)
        for s in (1.0, 0.37, -1.0, 2.0):  # s in [-1, 2]: angles up to pi
            worst_exp = max(worst_exp, np.abs(D.exp(s * th * axis) - D.model_exp(s * th * axis)).max())
    print(f"Log: worst relative difference {worst_log:.3g}; Exp: worst entry difference {worst_exp:.3g}")
    assert worst_log <= TOL_LOG_REL and worst_exp <= TOL_EXP
    assert np.array_equal(D.exp([0.0, 0.0, 0.0]), np.eye(3)) and np.array_equal(D.log(np.eye(3)), np.zeros(3))


def test_the_arctangent_on_its_whole_range():
    """The angle of the issue's check: 2 atan(tan(th / 2)) over (0, pi/2], relative."""
    th = np.linspace(1e-9, np.pi / 2, 4001)
    got = np.array([2.0 * D.atan(np.sin(t / 2) / np.cos(t / 2)) for t in th])
    worst = (np.abs(got - th) / th).max()
    print(f"arctangent: worst relative error of the angle {worst:.3g}")
    assert worst <= TOL_ATAN_REL


def test_pose_at_against_the_numpy_model_and_through_the_library():
    from quatro_amd import lib as ql
    worst_R = worst_c = 0.0
    for Kn, seed, ang in ((2, 0, 0.05), (3, 1, 1.5), (17, 2, 0.3), (256, 3, 0.05)):
        kt, kp = K.smooth_knots(Kn, seed, max_angle=ang)
        # inside the knots, and outside by up to one interval's length (s in [-1, 2]: what the series are cut for)
        rng = np.random.default_rng(seed)
        ts = np.concatenate([rng.uniform(kt[0], kt[-1], 40), rng.uniform(2 * kt[0] - kt[1], kt[0], 10),
                             rng.uniform(kt[-1], 2 * kt[-1] - kt[-2], 10), kt])
        for t in ts:
            T, _ = D.pose_at(kt, kp, t)
            Tm = D.model_pose_at(kt, kp, t)
            worst_R = max(worst_R, np.abs(T[:3, :3] - Tm[:3, :3]).max())
            worst_c = max(worst_c, np.abs(T[:3, 3] - Tm[:3, 3]).max())
            assert np.array_equal(_bits(ql.deskew_pose_at(kt, kp, t)), _bits(T))  # the library's host entry: the same bits
    print(f"pose_at: worst entry difference R {worst_R:.3g}, c {worst_c:.3g}")
    assert worst_R <= TOL_POSE_R and worst_c <= TOL_POSE_C


@pytest.mark.parametrize("Kn,seed,ang", [(2, 0, 0.05), (3, 1, 1.5), (256, 3, 0.05)])
def test_output_points_against_the_numpy_model(Kn, seed, ang):
    """The header's points before their rounding (qtr_deskew_point_f64) against the numpy model: the binary64 difference of
    the two is measured and held; out is that point rounded to float32 once (numpy's cast is the reference)."""
    kt, kp = K.smooth_knots(Kn, seed, max_angle=ang)
    cloud, times = K.random_cloud(3000, seed), K.random_times(3000, kt, seed)
    t_ref = float(kt[0] + 0.25 * (kt[-1] - kt[0]))
    out, info = D.deskew(cloud, times, kt, kp, t_ref)
    want = D.model_deskew(cloud, times, kt, kp, t_ref)
    assert info == {"n_points": 3000, "n_skipped": 0, "n_extrapolated": 0}
    assert np.array_equal(_bits(out[:, 3]), _bits(cloud[:, 3]))
    q = D.deskew_f64(cloud, times, kt, kp, t_ref)
    worst = np.abs(q - want).max()
    print(f"K={Kn}: worst |q_header - q_model| {worst:.3g} m on coordinates up to {np.abs(want).max():.0f} m")
    assert worst <= TOL_POINT_F64
    assert np.array_equal(_bits(out[:, :3]), _bits(q.astype(np.float32)))
    assert np.abs(out[:, :3] - cloud[:, :3]).max() > 1e-3  # (something was moved)


def test_interval_rule_on_and_around_every_knot():
    kt, kp = K.smooth_knots(5, 4)
    edges = K.edge_times(kt)
    for t, j, extra in edges:
        got_j, s = D.interval(kt, kp, float(t))
        _, got_extra = D.pose_at(kt, kp, float(t))
        assert (got_j, got_extra) == (j, extra), (float(t), got_j, s, got_extra, j, extra)
        assert (s < 0.0 or s > 1.0) == extra
    j, s = D.interval(kt, kp, kt[-1])
    assert j == 3 and s == 1.0  # the last knot: s == 1 on the last interval, not extrapolated
    j, s = D.interval(kt, kp, kt[2])
    assert j == 2 and s == 0.0
    cloud = K.random_cloud(len(edges), 6)
    times = np.array([t for t, _, _ in edges], np.float32)
    out, info = D.deskew(cloud, times, kt, kp, float(kt[0]))
    assert info == {"n_points": len(edges), "n_skipped": 0, "n_extrapolated": sum(e for _, _, e in edges)}
    want = D.model_deskew(cloud, times, kt, kp, float(kt[0]))
    assert np.abs(out[:, :3] - want).max() < 1e-5
    # t_ref may extrapolate as well; it is not counted
    out, info = D.deskew(cloud[:1], np.array([kt[1]], np.float32), kt, kp, float(kt[-1] + 1.0))
    assert info["n_extrapolated"] == 0


def test_skipped_points_keep_their_bits():
    cloud, times, n_skip = K.skipped_cloud()
    kt, kp = K.smooth_knots(3, 7)
    out, info = D.deskew(cloud, times, kt, kp, 0.0)
    assert info == {"n_points": 12, "n_skipped": n_skip, "n_extrapolated": 0}
    bad = ~(np.isfinite(cloud[:, :3]).all(axis=1) & np.isfinite(times))
    assert bad.sum() == n_skip
    assert np.array_equal(_bits(out[bad]), _bits(cloud[bad]))
    assert np.array_equal(_bits(out[:, 3]), _bits(cloud[:, 3]))  # the fourth float, NaN and inf included, everywhere
    assert np.all(out[~bad, :3] != cloud[~bad, :3])


def test_identity_knots_reproduce_every_value():
    cloud = K.random_cloud(2000, 8)
    cloud[0, :3] = (0.0, -0.0, 1e-30)
    cloud[1, :3] = (3.0e38, -3.0e38, 1e-45)
    for Kn in (2, 7):
        kt, kp = K.identity_knots(Kn)
        times = np.random.default_rng(Kn).uniform(-0.05, 0.15, 2000).astype(np.float32)  # (extrapolating, too)
        out, info = D.deskew(cloud, times, kt, kp, 0.04)
        assert np.array_equal(out, cloud) and info["n_skipped"] == 0 and info["n_extrapolated"] > 0


def _rotation_pair(angle):
    return np.array([0.0, 0.1]), np.stack([K.pose(K.rot([1, 2, 3], 0.3)), K.pose(K.rot([1, 2, 3], 0.3) @ K.rot([0.3, -1, 0.5], angle))])


REFUSALS = {
    "one knot": (lambda: (np.array([0.0]), np.eye(4)[None], 0.0), D.BAD_K),
    "257 knots": (lambda: K.identity_knots(257) + (0.0,), D.BAD_K),
    "a knot time that is NaN": (lambda: (np.array([0.0, np.nan, 0.2]), np.stack([np.eye(4)] * 3), 0.0), D.BAD_TIME),
    "a knot time that is infinite": (lambda: (np.array([0.0, 0.1, np.inf]), np.stack([np.eye(4)] * 3), 0.0), D.BAD_TIME),
    "equal knot times": (lambda: (np.array([0.0, 0.1, 0.1]), np.stack([np.eye(4)] * 3), 0.0), D.BAD_TIME),
    "decreasing knot times": (lambda: (np.array([0.0, 0.2, 0.1]), np.stack([np.eye(4)] * 3), 0.0), D.BAD_TIME),
    "a NaN in a rotation": (lambda: (np.array([0.0, 0.1]), np.stack([np.eye(4), K.pose(np.full((3, 3), np.nan))]), 0.0), D.BAD_POSE),
    "an infinite translation": (lambda: (np.array([0.0, 0.1]), np.stack([K.pose(c=(0, np.inf, 0)), np.eye(4)]), 0.0), D.BAD_POSE),
    "a rotation just above the limit": (lambda: _rotation_pair(K.ROTATION_LIMIT * (1 + 1e-9)) + (0.0,), D.BAD_ROTATION),
    "a half turn": (lambda: _rotation_pair(np.pi) + (0.0,), D.BAD_ROTATION),
    "t_ref NaN": (lambda: K.identity_knots(2) + (np.nan,), D.BAD_TREF),
    "t_ref infinite": (lambda: K.identity_knots(2) + (np.inf,), D.BAD_TREF),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(name):
    """The restatement names the reason; the library's host entry, qtr_deskew_pose_at, answers QTR_ERR_BAD_ARG to each."""
    from quatro_amd import lib as ql
    make, why = REFUSALS[name]
    kt, kp, t_ref = make()
    with pytest.raises(D.Refused) as ei:
        D.deskew(K.random_cloud(4), np.zeros(4, np.float32), kt, kp, t_ref)
    assert ei.value.why == why
    with pytest.raises(ql.QuatroHipError) as ei:
        ql.deskew_pose_at(kt, kp, t_ref)
    assert ei.value.code == ql.QTR_ERR_BAD_ARG


def test_a_rotation_just_under_the_limit_is_admitted():
    from quatro_amd import lib as ql
    kt, kp = _rotation_pair(K.ROTATION_LIMIT * (1 - 1e-9))
    out, info = D.deskew(K.random_cloud(4), np.full(4, 0.05, np.float32), kt, kp, 0.0)
    assert info["n_points"] == 4
    T = ql.deskew_pose_at(kt, kp, 0.1)
    assert np.abs(T - kp[1]).max() < 1e-14
    # a last row that is not 0 0 0 1 is not read
    kp2 = kp.copy()
    kp2[:, 3, :] = np.nan
    assert np.array_equal(_bits(ql.deskew_pose_at(kt, kp2, 0.03)), _bits(ql.deskew_pose_at(kt, kp, 0.03)))


def test_round_trip_through_the_synthesiser():
    """skew() carries a scan into what a moving sensor records, in numpy float64, and rounds to float32; deskew with the same
    knots and t_ref = 0 must recover the scan.  The bound, per point in Euclidean distance:
      * the skewed point is stored as float32: an error vector of at most half an ulp per axis, h = half a float32 ulp at the
        largest |coordinate| of the skewed cloud, so at most sqrt(3) h long; the deskew rotates it (its length stays) into the
        output frame;
      * the output is rounded to float32 once: at most half an ulp per axis at the largest |coordinate| of the result, again
        at most sqrt(3) h' long;
      * the times are the same float32 values on both sides: no error;
      * the header's and the numpy model's binary64 arithmetic differ by at most TOL_POINT_F64 per axis (measured
        above on clouds of the same extent, x 10): sqrt(3) of it.
    Hence |q_i - scan_i| <= sqrt(3) (h + h' + TOL_POINT_F64)."""
    from quatro_amd import synth
    scan = synth.kitti64_pair(0)[0]
    M = K.pose(K.rot([0.1, -0.2, 1.0], 0.04), (1.0, 0.05, -0.02))  # a metre and 0.04 rad per sweep
    kt, kp = K.two_knots(M)
    skewed, times = K.skew(scan, kt, kp)
    warp = np.sqrt(((skewed[:, :3] - scan[:, :3]).astype(np.float64) ** 2).sum(axis=1)).max()
    out, info = D.deskew(skewed, times, kt, kp, 0.0)
    assert info == {"n_points": scan.shape[0], "n_skipped": 0, "n_extrapolated": 0}
    err = np.sqrt(((out[:, :3].astype(np.float64) - scan[:, :3].astype(np.float64)) ** 2).sum(axis=1)).max()
    h_in, h_out = _half_ulp32(np.abs(skewed[:, :3]).max()), _half_ulp32(np.abs(scan[:, :3]).max())
    bound = np.sqrt(3.0) * (h_in + h_out + TOL_POINT_F64)
    print(f"round trip: {scan.shape[0]} points, the sweep was warped by up to {warp:.3f} m, recovered within {err:.3g} m "
          f"(bound {bound:.3g} m)")
    assert warp > 0.5 and err <= bound
    assert np.array_equal(_bits(out[:, 3]), _bits(scan[:, 3]))


def test_constant_velocity_knots():
    from quatro_amd import api
    A, B = K.pose(K.rot([0, 0, 1], 0.3), (1, 2, 0.1)), K.pose(K.rot([0.1, 0, 1], 0.35), (2, 2.2, 0.1))
    kt, kp = api.constant_velocity_knots(A, B, 0.1)
    assert np.array_equal(kt, [0.0, 0.1]) and np.array_equal(kp[0], np.eye(4))
    assert np.abs(kp[1] - np.linalg.inv(A) @ B).max() < 1e-15
    # the guess of the next pose is the previous pose moved by that motion: the same fixed-order arithmetic
    assert np.abs(B @ kp[1] - api.constant_velocity_guess(A, B)).max() < 1e-15


def test_the_three_entry_points_are_declared_exported_and_bound():
    """The entry points of include/quatro_deskew.h are three of libquatro_ext.so's exports, they have their ctypes
    signatures, libquatro_hip.so exports none of them, and the info struct is its ctypes mirror."""
    import ctypes
    import os
    import subprocess
    import tempfile
    import ext_abi
    from quatro_amd import lib as ql
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    assert ext_abi.check_header("quatro_deskew.h") == {"qtr_deskew", "qtr_keyframe_create_deskewed", "qtr_deskew_pose_at"}
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "quatro_deskew.h"
#include "qtr_deskew_math.h"
int main(void){printf("%zu %zu %zu %zu %d %d\n", sizeof(qtr_deskew_info), offsetof(qtr_deskew_info, n_points),
  offsetof(qtr_deskew_info, n_skipped), offsetof(qtr_deskew_info, n_extrapolated), QTR_DESKEW_KNOTS_MAX, QTR_DESKEW_MAX_KNOTS); return 0;}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.cpp")
        open(c, "w").write(src)
        subprocess.check_call(["g++", "-I", os.path.join(root, "include"), c, "-o", os.path.join(d, "s")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    E = ql.DeskewInfo
    assert got == [ctypes.sizeof(E), E.n_points.offset, E.n_skipped.offset, E.n_extrapolated.offset, ql.DESKEW_MAX_KNOTS,
                   D.MAX_KNOTS] == [12, 0, 4, 8, 256, 256]
