"""Inputs the continuous-time registration tests share (CPU and GPU): the small edge scene with its named times, the anchor's
three begin poses, and the accuracy scenes — a sweep skewed under a true motion that differs from the constant-velocity guess.
Everything here is numpy; the skew comes from deskew_cases (numpy's sin / cos), nothing is shared with the headers."""
import numpy as np

import deskew_cases as DC
import icp_restate as R

SIDE = 1.0
# float32-representable sweep ends, so that a time can sit exactly ON either end (the anchor needs t == t_end)
T_BEGIN, T_END = 0.25, 0.375
SIZES = (0, 1, 255, 256, 257, 513)
# three unrelated begin poses for the anchor (the result must not depend on them at all)
ANCHOR_BEGINS = (np.eye(4), R.rigid(R.rot(0.3, -0.2, 1.1), [5.0, -2.5, 0.7]), R.rigid(R.rot(-0.05, 0.6, -0.4), [-30.0, 12.0, 3.0]))


def f32_next(x, up=True):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def named_times():
    """(time, skipped, extrapolated): on either end, the float32 just inside and just outside each, far outside, NaN, inf."""
    b, e = np.float32(T_BEGIN), np.float32(T_END)
    return [(e, 0, 0), (b, 0, 0), (f32_next(e, False), 0, 0), (f32_next(e, True), 0, 1), (f32_next(b, True), 0, 0),
            (f32_next(b, False), 0, 1), (np.float32(T_END + 0.5), 0, 1), (np.float32(T_BEGIN - 0.5), 0, 1),
            (np.float32(np.nan), 1, 0), (np.float32(np.inf), 1, 0)]


def small_map():
    """(points, normals, pose) of the edge scene's map: the box scene at 40 points per face under a pose, a few hundred
    voxels at SIDE."""
    pts, nrm = R.box_scene(40, seed=6)
    return pts, nrm, R.rigid(R.rot(0.02, -0.03, 0.4), [0.377, -1.291, 0.613])


BEGIN = R.rigid(R.rot(0.02, -0.03, 0.4), [0.377, -1.291, 0.613]) @ R.rigid(R.rot(0.004, -0.006, 0.01), [0.08, -0.05, 0.02])
GUESS_END = BEGIN @ R.rigid(R.rot(-0.003, 0.005, 0.03), [0.35, 0.06, -0.01])


def edge_cloud(n, seed=0):
    """n sources of the edge scene with their normals and times: map points seen from about BEGIN, times spread over the
    sweep in no order.  From n >= 255 on the first rows carry the named times, then a NaN point, an infinite point, a zero
    normal, a NaN normal and points that fall into no voxel.  Returns (src4, normals4, times, n_skipped, n_extrapolated)."""
    rng = np.random.default_rng(500 + seed)
    pts, nrm, pose = small_map()
    sel = rng.choice(pts.shape[0], n, replace=True)
    Bi = np.linalg.inv(BEGIN) @ pose
    s = pts[sel, :3].astype(np.float64) @ Bi[:3, :3].T + Bi[:3, 3] + rng.normal(scale=0.02, size=(n, 3))
    sn = nrm[sel, :3].astype(np.float64) @ Bi[:3, :3].T + rng.normal(scale=0.05, size=(n, 3))
    t = rng.uniform(T_BEGIN, T_END, n).astype(np.float32)
    skipped = extra = 0
    if n >= 255:
        named = named_times()
        for k, (tt, sk, ex) in enumerate(named):
            t[k] = tt
            skipped, extra = skipped + sk, extra + ex
        k = len(named)
        s[k] = [np.nan, 1.0, 1.0]
        s[k + 1] = [1.0, np.inf, 1.0]
        sn[k + 2] = 0.0
        sn[k + 3] = [np.nan, 1.0, 0.0]
        skipped += 4
        s[k + 4:k + 9] = rng.random((5, 3)) * 5.0 + 60.0  # no voxel there: they take part and find nothing
        t[k + 4] = f32_next(T_END, True)  # (extrapolated and without a voxel: counted all the same)
        extra += 1
        t[k + 2] = np.float32(T_END + 1.0)  # (skipped for its normal: NOT counted as extrapolated)
    return R.f4(s), R.f4(sn), t, skipped, extra


# ---- the accuracy scenes ------------------------------------------------------------------------------------------------------
PERIOD = DC.PERIOD
ACC_BEGIN = R.rigid(R.rot(0.01, -0.015, 0.25), [1.2, -0.8, 0.3])
# (name, the sensor's true motion over the sweep in its own frame at the sweep's start, what the constant-velocity guess says)
ACC_CASES = (
    ("speed change", R.rigid(R.rot(0.0, 0.0, 0.01), [1.0, 0.0, 0.0]), R.rigid(R.rot(0.0, 0.0, 0.01), [0.6, 0.0, 0.0])),
    ("yaw-rate change", R.rigid(R.rot(0.0, 0.0, np.radians(3.0)), [0.8, 0.0, 0.0]), R.rigid(R.rot(0.0, 0.0, np.radians(1.0)), [0.8, 0.0, 0.0])),
)


def accuracy_scene(case):
    """The box scene (300 points per face) as the map's world cloud, and what a sensor records of it over one sweep that
    begins at ACC_BEGIN and moves by the case's TRUE motion: dict(world, world_normals, raw, normals, times, begin, true_motion,
    guess_motion).  raw is the skewed sweep (deskew_cases.skew of the scene seen from the begin pose, 1 cm of noise), normals
    are the scene's in the begin frame."""
    name, M_true, M_guess = case
    world, wn = R.box_scene(300, seed=12)
    rng = np.random.default_rng(77)
    Bi = np.linalg.inv(ACC_BEGIN)
    scan = world.copy()
    scan[:, :3] = (world[:, :3].astype(np.float64) @ Bi[:3, :3].T + Bi[:3, 3] + rng.normal(scale=0.01, size=(world.shape[0], 3))).astype(np.float32)
    normals = R.f4(wn[:, :3].astype(np.float64) @ Bi[:3, :3].T)
    kt, kp = DC.two_knots(M_true, PERIOD)
    raw, times = DC.skew(scan, kt, kp, PERIOD)
    return {"name": name, "world": world, "world_normals": wn, "raw": R.f4(raw), "normals": normals, "times": times,
            "begin": ACC_BEGIN, "true_motion": M_true, "guess_motion": M_guess}


def pose_error(T, want):
    """(translation error in metres, rotation error in degrees)."""
    return float(np.linalg.norm(np.asarray(T)[:3, 3] - np.asarray(want)[:3, 3])), R.rot_err_deg(np.asarray(T), np.asarray(want))
