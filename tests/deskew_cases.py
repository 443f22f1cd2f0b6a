"""Named inputs of the deskew tests (CPU and GPU) and the skew synthesiser.  Everything here is numpy: nothing is shared with
include/qtr_deskew_math.h, rotations come from deskew_restate's numpy model."""
import numpy as np

import deskew_restate as D

PERIOD = 0.1  # seconds per sweep (a 10 Hz spinning LiDAR)
ROTATION_LIMIT = np.pi / 2  # the largest relative rotation of two consecutive knots


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    return D.model_exp(a / np.sqrt(a @ a) * float(angle))


def pose(R=None, c=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = c
    return T


def identity_knots(K=2, t0=0.0, t1=PERIOD):
    return np.linspace(t0, t1, K), np.stack([np.eye(4)] * K)


def smooth_knots(K, seed=0, t0=0.0, t1=PERIOD, max_angle=0.05, max_step=0.2):
    """K knots of a wandering sensor: times on a grid of float32-representable values (multiples of 2^-13 s from t0, unevenly
    spaced), each knot a rotation of up to max_angle rad about a random axis and up to max_step m away from the one before."""
    rng = np.random.default_rng(9100 + 31 * seed + K)
    ticks = np.sort(rng.choice(np.arange(1, 4 * K + 8), size=K - 1, replace=False))
    scale = 2.0 ** np.floor(np.log2((t1 - t0) / ticks[-1]))
    kt = np.concatenate([[t0], t0 + ticks * scale])
    T = [pose(rot(rng.normal(size=3), rng.uniform(0, 0.3)), rng.uniform(-1, 1, 3))]
    for _ in range(K - 1):
        step = pose(rot(rng.normal(size=3), rng.uniform(0, max_angle)), rng.uniform(-max_step, max_step, 3))
        T.append(T[-1] @ step)
    assert np.all(kt.astype(np.float32).astype(np.float64) == kt)
    return kt, np.stack(T)


def random_cloud(n, seed=0, extent=80.0):
    """[n, 4] float32: x, y in [-extent, extent], z in [-3, 5], an arbitrary fourth float."""
    rng = np.random.default_rng(7700 + seed)
    c = np.zeros((n, 4), np.float32)
    c[:, 0] = rng.uniform(-extent, extent, n)
    c[:, 1] = rng.uniform(-extent, extent, n)
    c[:, 2] = rng.uniform(-3, 5, n)
    c[:, 3] = rng.uniform(0, 1, n)
    return c


def random_times(n, kt, seed=0):
    """float32 times inside the knots' span, in no order."""
    rng = np.random.default_rng(7800 + seed)
    return rng.uniform(kt[0], kt[-1], n).astype(np.float32)


def edge_times(kt):
    """The float32 times the interval rule is tested at, with what the rule says of each: (time, j, extrapolated).  The knot
    times must be float32 values.  On every knot; one float32 below and above every knot; well before the first and after the
    last knot."""
    kt = np.asarray(kt, np.float64)
    K = kt.shape[0]
    out = []
    for k, t in enumerate(kt):
        f = np.float32(t)
        assert float(f) == t
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        out.append((f, min(k, K - 2), False))                        # on the knot (the last one: s == 1, not extrapolated)
        out.append((lo, min(max(k - 1, 0), K - 2), k == 0))          # just below: the interval before (none: extrapolated)
        out.append((hi, min(k, K - 2), k == K - 1))                  # just above
    span = kt[-1] - kt[0]
    out.append((np.float32(kt[0] - 0.5 * span), 0, True))
    out.append((np.float32(kt[-1] + 0.5 * span), K - 2, True))
    return out


def skipped_cloud():
    """8 points: NaN or an infinity in x, y, z and in the time, one each, (cloud, times, number skipped)."""
    c = random_cloud(12, seed=5)
    t = np.full(12, 0.03, np.float32)
    c[1, 0], c[2, 1], c[3, 2], t[4] = np.nan, np.nan, np.nan, np.nan
    c[6, 0], c[7, 1], c[8, 2], t[9] = np.inf, -np.inf, np.inf, -np.inf
    c[1, 3] = np.float32(np.nan)  # (the fourth float is not looked at ...)
    c[10, 3] = np.float32(np.inf)  # (... on a point that is deskewed either)
    return c, t, 8


# ---- the skew synthesiser ------------------------------------------------------------------------------------------------
def azimuth_times(scan, period=PERIOD):
    """times[i] = float32(period (atan2(y, x) mod 2 pi) / 2 pi): one revolution per sweep, starting at the +x axis."""
    s = np.asarray(scan, np.float32).astype(np.float64)
    return (period * (np.mod(np.arctan2(s[:, 1], s[:, 0]), 2 * np.pi) / (2 * np.pi))).astype(np.float32)


def skew(scan, knot_times, knot_poses, period=PERIOD):
    """What a sensor records of the scene that `scan` is at time 0 while it moves as the knots say (the numpy model's pose
    rule: deskew_restate.model_poses_at; a knot pose is sensor frame -> a fixed frame).  Returns (skewed [P, 4] float32,
    times [P] float32): skewed_i = T(t_i)^-1 T(0) scan_i in float64, cast to float32; the fourth float travels unchanged."""
    scan = np.asarray(scan, np.float32)
    times = azimuth_times(scan, period)
    T0 = D.model_pose_at(knot_times, knot_poses, 0.0)
    world = scan[:, :3].astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]
    R, c = D.model_poses_at(knot_times, knot_poses, times.astype(np.float64))
    out = scan.copy()
    out[:, :3] = np.einsum("nji,nj->ni", R, world - c).astype(np.float32)
    return out, times


def two_knots(M, period=PERIOD):
    """The knots of the motion from the identity at 0 to M at `period`."""
    return np.array([0.0, period]), np.stack([np.eye(4), np.asarray(M, np.float64)])
