"""Inputs the visibility-carving tests share (CPU and GPU): raster scans made pixel by pixel, shell scans around the
hand-built map of vmap_cases, the named edge cases, and the eight-scan scene with a moving box of the quality test."""
import numpy as np

import icp_restate as R
import vmap_carve_restate as CR
import vmap_cases as K

# a small image that sees the hand-built map (|z| <= 3 at a few metres) from anywhere near it
WIDE = dict(rows=16, cols=64, fov_up_deg=75.0, fov_down_deg=-75.0, min_range=0.5, max_range=60.0)
TINY = dict(rows=4, cols=8, fov_up_deg=75.0, fov_down_deg=-75.0, min_range=0.5, max_range=60.0)


def raster_scan(p: CR.Params, seed, fill=0.8, r_lo=8.0, r_hi=30.0, per_pixel=1, smooth=False):
    """A scan made pixel by pixel: each pixel of p's image is filled with probability `fill` by per_pixel points in directions
    drawn inside the pixel (a tenth of a pixel away from its edges), at ranges drawn from [r_lo, r_hi] — or, smooth, on a
    surface whose range swings between r_lo and r_hi three times around the sensor, with 5 cm of noise, so that the pixels of
    a window agree; in random storage order, [n, 4] float32 in the scan's own frame."""
    rng = np.random.default_rng(seed)
    up, down = np.deg2rad(p.fov_up_deg), np.deg2rad(p.fov_down_deg)
    rows, cols = np.nonzero(rng.random((p.rows, p.cols)) < fill)
    rows, cols = np.repeat(rows, per_pixel), np.repeat(cols, per_pixel)
    n = rows.shape[0]
    el = up - (rows + 0.1 + 0.8 * rng.random(n)) * (up - down) / p.rows
    az = -np.pi + (cols + 0.1 + 0.8 * rng.random(n)) * 2 * np.pi / p.cols
    r = rng.uniform(r_lo, r_hi, n)
    if smooth:
        r = 0.5 * (r_lo + r_hi) + 0.5 * (r_hi - r_lo) * np.sin(3 * az + seed) + rng.normal(0.0, 0.05, n)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1)
    return R.f4(pts[rng.permutation(n)])


def shell_scan(n, seed, pose, radius=9.0, near_world=None, el_max_deg=70.0):
    """n points on a rough shell of `radius` around the sensor at `pose` (scan frame -> map frame), plus the world points
    near_world seen from there: what makes the voxels around them occupied.  [n + len(near_world), 4] float32, scan frame."""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(rng.uniform(-el_max_deg, el_max_deg, n))
    az = rng.uniform(-np.pi, np.pi, n)
    r = radius + rng.uniform(-0.5, 0.5, n)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1)
    if near_world is not None and len(near_world):
        Pi = np.linalg.inv(np.asarray(pose, np.float64))
        pts = np.concatenate([pts, np.asarray(near_world, np.float64) @ Pi[:3, :3].T + Pi[:3, 3]])
    return R.f4(pts[rng.permutation(pts.shape[0])])


SENSOR_POSES = (R.rigid(R.rot(0.02, -0.03, 0.4), [0.3, -0.2, 0.1]),
                R.rigid(R.rot(-0.05, 0.04, -2.0), [-0.6, 0.5, -0.2]),
                R.rigid(np.eye(3), [0.0, 0.0, 0.0]))


def hand_scans(sections_cloud, n_scans=3, n=1500, seed=0):
    """Shell scans of the hand-built map from SENSOR_POSES (cycled): each also sees a different quarter of the map's voxel means (one quarter is seen by none)
    (sections_cloud: the CLOUD section), so voxels are occupied in some scans and seen through in others.  Non-finite points
    and a point on the z axis are mixed in.  Returns (clouds, poses)."""
    mu = np.asarray(sections_cloud, np.float64)[:, :3]
    mu = mu[np.abs(mu).max(axis=1) < 100.0]
    clouds, poses = [], []
    for b in range(n_scans):
        P = SENSOR_POSES[b % len(SENSOR_POSES)] if b < len(SENSOR_POSES) else \
            R.rigid(R.rot(0.01 * b, -0.02 * b, 0.37 * b), [0.05 * (b % 7) - 0.2, 0.04 * (b % 5) - 0.1, 0.03 * (b % 3)])
        c = shell_scan(n, seed + 17 * b, P, near_world=mu[b % 3::4])
        c[3, :3] = [np.nan, 1.0, 1.0]
        c[5, :3] = [1.0, np.inf, 1.0]
        c[7, :3] = [0.0, 0.0, 4.0]      # on the z axis
        c[9, :3] = [1e-3, 0.0, 0.0]     # below min_range
        c[11, :3] = [3e4, 0.0, 0.0]     # above max_range
        clouds.append(c)
        poses.append(P)
    return clouds, np.stack(poses)


def random_map_cloud(n_voxels, side, seed, r_lo=3.0, r_hi=25.0, z_lo=-1.6, z_hi=0.4):
    """Points (and normals) of n_voxels distinct voxels in an annulus around the origin, low enough for the default image's
    field of view from a sensor near the origin: one to three members per voxel."""
    rng = np.random.default_rng(seed)
    got = set()
    while len(got) < n_voxels:
        r, a = np.sqrt(rng.uniform(r_lo ** 2, r_hi ** 2, n_voxels)), rng.uniform(-np.pi, np.pi, n_voxels)
        z = rng.uniform(z_lo, z_hi, n_voxels)
        for c in np.floor(np.stack([r * np.cos(a), r * np.sin(a), z], axis=1) / side).astype(int):
            if len(got) < n_voxels:
                got.add(tuple(int(x) for x in c))
    return K.cloud_of_voxels(sorted(got), side, seed=seed)


EDGE_IMAGE = dict(rows=8, cols=16, fov_up_deg=40.0, fov_down_deg=-40.0, window=1, margin_abs=2.5)


def edge_clouds():
    """The named edge cases as clouds for a map of 0.5 m voxels under the identity and EDGE_IMAGE: (name, map points, scan
    points, carved?) — each map has ONE voxel, whose mean is its single member exactly.
      limit / above   the voxel at (3, 4, 0) has r_v = 5 and limit 7.5; the return (4.5, 6, 0), same azimuth, has r = 7.5
                      exactly (kept); with y one float above 6 its float range is one float above 7.5 (carved)
      fold            the voxel at (-5, -1e-9, 0) lies in column 0; the return (-30, +0, 0) has az = pi, which folds to column
                      0 and fills the centre far behind the voxel (carved) ...
      wrap            ... unless a return in the LAST column, one row below, is near (kept): the window wraps
      empty           filled neighbours and no return in the centre pixel: no vote (kept)
      skipped         returns that have no pixel (non-finite, on the z axis, out of range, above the image) fill nothing (kept)
      first_row / last_row, _near, _other_end   the window clamped at the image's first and last row (below)"""
    f = np.float32
    el = np.deg2rad(-15.0)                                                  # row 5
    last = [-6 * np.cos(el), 0.01, 6 * np.sin(el)]                          # az just below pi: column 15
    up = np.nextafter(f(6.0), f(7.0))
    v34, v0 = [[3.0, 4.0, 0.0]], [[-5.0, -1e-9, 0.0]]
    cases = [("limit", v34, [[4.5, 6.0, 0.0]], False), ("above", v34, [[4.5, up, 0.0]], True),
             ("fold", v0, [[-30.0, 0.0, 0.0]], True), ("wrap", v0, [[-30.0, 0.0, 0.0], last], False),
             ("empty", v34, [[1.2, 4.0, 0.0], [4.0, 1.2, 0.0], [1.5, 2.0, 1.2]], False),
             ("skipped", v34, [[np.nan, 6.0, 0.0], [0.0, 0.0, 9.0], [450.0, 600.0, 0.0], [0.3, 0.4, 0.0], [4.5, 6.0, 30.0]], False)]
    # the window clamped at the first and the last row: the voxel a milliradian inside the image's edge, its centre filled
    # far behind it (carved); a near return one row inside and one column on (kept); a near return in the row a wrapped row
    # index would reach, at the other end of the image (still carved)
    def ray(el_deg, az_deg, r):
        e, a = np.deg2rad(el_deg), np.deg2rad(az_deg)
        return [r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e)]
    edge = np.rad2deg(1e-3)
    for name, sign in (("first_row", 1.0), ("last_row", -1.0)):
        v, far = [ray(sign * (40.0 - edge), 5.0, 5.0)], ray(sign * (40.0 - edge), 5.0, 40.0)
        cases += [(name, v, [far], True), (name + "_near", v, [far, ray(sign * 25.0, 30.0, 5.0)], False),
                  (name + "_other_end", v, [far, ray(-sign * 35.0, 5.0, 5.0)], True)]
    return [(name, R.f4(np.array(m, f)), R.f4(np.array(s, f)), carved) for name, m, s, carved in cases]


# (field, value, the header's refusal code) with the other fields at their defaults and two scans in the call
BAD_PARAMS = (("rows", 0, 1), ("rows", 257, 1), ("cols", 7, 2), ("cols", 4097, 2), ("fov_up_deg", -25.5, 3), ("fov_up_deg", np.nan, 3),
              ("fov_down_deg", 2.5, 3), ("fov_down_deg", -np.inf, 3), ("window", -1, 4), ("window", 4, 4), ("min_votes", 0, 5),
              ("min_votes", 3, 5), ("margin_abs", -1e-9, 6), ("margin_abs", np.inf, 6), ("margin_rel", -1.0, 6),
              ("margin_rel", np.nan, 6), ("min_range", 80.0, 7), ("min_range", np.nan, 7), ("max_range", 1.0, 7),
              ("max_range", np.inf, 7))


# ---- the quality scene -------------------------------------------------------------------------------------------------
BOX_SIZE = (4.0, 2.0, 1.5)


def moving_box_scans(vegetation: bool, n_scans=8, step=1.5, box_step=3.0, seed=0):
    """synth._scene at its defaults (with KITTI16K's vegetation or without), a 5 m disc around every pose and the lane
    2 < y < 7 cleared; n_scans poses `step` apart along x, scanned with the ground kept (_scan(..., ground=True)); a
    4 x 2 x 1.5 m box on the ground at y = 4.5 that moves box_step per scan.  Returns (scans [n, 4] float32 in their own
    frames, poses [n_scans, 4, 4], is_box: per scan a bool per point, True for returns from the box)."""
    from quatro_amd import synth
    rng = np.random.default_rng(synth.SEED_BASE + 7919 * (seed + 1))
    veg = dict(n_trees=synth.KITTI16K["n_trees"], n_hedges=synth.KITTI16K["n_hedges"], leaf_p=synth.KITTI16K["leaf_p"],
               crown=synth.KITTI16K["crown"]) if vegetation else {}
    sc = synth._scene(rng, 100, 60, 150, 300, **veg)
    lo, hi = sc[0], sc[1]
    porous = sc[2] if len(sc) > 2 else None
    xs = (np.arange(n_scans) - (n_scans - 1) / 2) * step
    keep = ~((hi[:, 1] > 2.0) & (lo[:, 1] < 7.0))
    for x in xs:
        dx = np.maximum(np.maximum(lo[:, 0] - x, x - hi[:, 0]), 0.0)
        dy = np.maximum(np.maximum(lo[:, 1], -hi[:, 1]), 0.0)
        keep &= np.hypot(dx, dy) > 5.0
    lo, hi = lo[keep], hi[keep]
    porous = porous[keep] if porous is not None else None
    bump_k, bump_ph = rng.normal(0.0, 2.0, size=(6, 3)), rng.uniform(0.0, 2 * np.pi, size=6)
    scans, poses, is_box = [], [], []
    for k, x in enumerate(xs):
        bx = -10.0 + box_step * k
        blo = np.array([[bx - BOX_SIZE[0] / 2, 4.5 - BOX_SIZE[1] / 2, -synth.SENSOR_HEIGHT]])
        bhi = np.array([[bx + BOX_SIZE[0] / 2, 4.5 + BOX_SIZE[1] / 2, -synth.SENSOR_HEIGHT + BOX_SIZE[2]]])
        origin = np.array([x, 0.0, 0.0])
        pts, _ = synth._scan(origin, 0.0, np.concatenate([lo, blo]), np.concatenate([hi, bhi]), rng, 0.02, bump_k, bump_ph, 0.0,
                             ground=True, porous=None if porous is None else np.concatenate([porous, [0.0]]))
        w = pts[:, :3].astype(np.float64) + origin
        is_box.append(((w > blo[0] + [-0.15, -0.15, 0.08]) & (w < bhi[0] + 0.15)).all(axis=1))
        T = np.eye(4)
        T[:3, 3] = origin
        scans.append(pts)
        poses.append(T)
    return scans, np.stack(poses), is_box
