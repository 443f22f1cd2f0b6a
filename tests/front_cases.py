"""Named clouds for the FPFH chain of quatro_amd/csrc/frontend.hip (k2_cell_* / k2_ranges, k2_neighbors, k2_neighbors_big,
k2_normals, k2_spfh, k2_fpfh) and for the voxel grid: degenerate geometry, list lengths on both sides of every sort and
staging switch, and pairs that only the margin of the neighbour grid's cell side keeps together.  A plain module:
deterministic numpy generators, no fixtures, no GPU work.  Used by tests/test_front_cases_cpu.py (the oracle against
independent references, the clouds against what they claim) and tests/test_gpu_front_cases.py (the device against the
oracle, bit for bit, along both forms of the neighbour grid).

    case(name) -> FrontCase(cloud, r_normal, r_fpfh, claims)

cloud is [n, 4] binary32 (n <= 700); the radii are binary32 values held as Python floats, so that the oracle (which takes
doubles) and the library (which takes floats) square the same number; claims says what the case is there for, and the
CPU test asserts every entry.  Also here, because both the CPU and the GPU tests need them: the brute-force neighbour
lists, the numpy voxel grid, the numpy mirror of the neighbour grid's cell arithmetic, and the inputs and the numpy mirror
of the SPFH angle-bin shortcut.
"""
from collections import namedtuple

import numpy as np

f32 = np.float32

# ---------------------------------------------------------------------------------------------- mirrored constants
QTR_KMAX = 256          # frontend.h: entries of a list's fixed slot; longer lists live in the long-list arena
FPFH_CHUNK = 32         # frontend.hip: entries of a list staged per round of k2_fpfh
FPFH_PB = 7             # points per workgroup of k2_fpfh
SPFH_PB = 32            # points per workgroup of k2_spfh
CELL_MARGIN = f32(1.001)  # cell side of the neighbour grid = r_fpfh * 1.001f
CELL_CLAMP = 255        # cell_of clamps every cell coordinate to 0 .. 255
QTR_CELL_CAP = 1 << 21  # frontend.h: the largest grid the dense cell table serves; above it the chain sorts packed keys
RANK_SORT_MAX = 64      # k2_neighbors: lists up to here are sorted by rank, longer ones by the bitonic network
BITONIC_MIN = 128       # ... whose size is 128 up to here and 256 above
CNT_BITS_SWITCH = 372   # k2_fpfh: 11 k needs 12 bits up to here (11 * 372 = 4092), 13 above

FrontCase = namedtuple("FrontCase", "cloud r_normal r_fpfh claims")

R_NORMAL, R_FPFH = 0.5, 0.75  # the demo's radii: both exact in binary32


def _r32(r):
    return float(f32(r))


def _pack(xyz):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    c = np.zeros((xyz.shape[0], 4), dtype=f32)
    c[:, :3] = xyz.astype(f32)
    return c


def _exact(xyz):
    """for hand-chosen coordinates: they are binary32 values already"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(xyz.astype(f32).astype(np.float64), xyz)
    return _pack(xyz)


def _lattice(nx, ny, nz, step, origin):
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1) * step + np.asarray(origin, dtype=np.float64)


def _seed(name):
    return [ord(c) for c in name]


# ---------------------------------------------------------------------------------------------- independent references
def brute_neighbors(cloud, radius):
    """Radius-neighbour lists by brute force in binary32, the operation order of FLANN's L2_Simple with the query first:
    d2 = ((dx dx) + dy dy) + dz dz, kept iff d2 < float(r r), sorted by (d2, index), the query included.
    -> (offsets int64 [n + 1], indices int32, d2 float32)"""
    p = np.ascontiguousarray(cloud[:, :3], dtype=f32)
    n = p.shape[0]
    r2 = f32(float(radius) * float(radius))
    off = np.zeros(n + 1, dtype=np.int64)
    idx, d2 = [], []
    for i in range(n):
        dx, dy, dz = p[i, 0] - p[:, 0], p[i, 1] - p[:, 1], p[i, 2] - p[:, 2]
        dd = ((dx * dx) + dy * dy) + dz * dz
        sel = np.nonzero(dd < r2)[0]
        order = sel[np.lexsort((sel, dd[sel]))]
        idx.append(order.astype(np.int32))
        d2.append(dd[order])
        off[i + 1] = off[i] + order.size
    return off, np.concatenate(idx) if n else np.zeros(0, np.int32), np.concatenate(d2) if n else np.zeros(0, f32)


def voxelize_numpy(pts, leaf):
    """pcl::VoxelGrid restated in numpy: binary32 voxel indices floor(p / leaf) - floor(min / leaf), centroids added up in
    ascending (voxel, point) order in binary32.  For grids that fit int32 -> centroids [m, 3] float32"""
    pts = np.ascontiguousarray(pts, dtype=f32)
    leaf = f32(leaf)
    inv = f32(1.0) / leaf
    mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
    minb = np.floor(mn * inv).astype(np.int64)
    maxb = np.floor(mx * inv).astype(np.int64)
    div = maxb - minb + 1
    ijk = (np.floor(pts[:, :3] * inv) - minb.astype(f32)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.lexsort((np.arange(len(idx)), idx))
    exp = []
    i = 0
    while i < len(order):
        j = i
        acc = np.zeros(3, dtype=f32)
        while j < len(order) and idx[order[j]] == idx[order[i]]:
            acc = acc + pts[order[j], :3]
            j += 1
        exp.append(acc / f32(j - i))
        i = j
    return np.array(exp, dtype=f32)


def cells_of(x, mn, cell):
    """cell_of of frontend.hip without the clamp, one axis: floorf((x - mn) / cell) in binary32"""
    x, mn, cell = np.asarray(x, dtype=f32), f32(mn), f32(cell)
    return np.floor((x - mn) / cell).astype(np.int64)


def grid_cells(cloud, r_fpfh):
    """cell_dims of frontend.hip over the cloud's bounding box: (nx, ny, nz) after the clamp, and the unclamped counts"""
    cell = f32(r_fpfh) * CELL_MARGIN
    mn, mx = cloud[:, :3].min(0), cloud[:, :3].max(0)
    raw = np.array([int(cells_of(mx[a], mn[a], cell)) + 1 for a in range(3)])
    return np.minimum(raw, CELL_CLAMP + 1), raw


# ---------------------------------------------------------------------------------------------- neighbour search
def _lattice3d():
    xyz = _lattice(6, 6, 3, 0.25, (-0.5, -0.75, -0.25))
    return FrontCase(_exact(xyz), R_NORMAL, R_FPFH, dict(
        d2_equal_rn2=True,         # pairs two steps apart: d2 = 0.25 = rn2 exactly, excluded from the normals by the strict <
        d2_equal_r2=True,          # pairs three steps apart: d2 = 0.5625 = r2 exactly, excluded from the lists
        d2_ties=1000,              # at least this many neighbouring list entries with equal d2 (ordered by index)
        nan_normal_finite_curv=1,  # at least one interior point: an isotropic neighbourhood, (NaN, NaN, NaN, finite)
        negative_coordinates=True))


STRADDLE_R = (0.7, 0.3, 1.1, 0.75)
STRADDLE_MN = f32(-57.3)
STRADDLE_ROWS = 18


def _ulps(x, k):
    return (x + f32(k) * np.spacing(x)).astype(f32)


def _straddle_candidates(rf, cell):
    """pairs (x1, x2) on one line: x1 within +-3 ulp of border 2 .. 249 of a grid of side `cell` whose origin is
    STRADDLE_MN, x2 = x1 +- (r - k ulp), k = 0 .. 5 (the second point above the first, and below it)"""
    ks = np.arange(2, 250)
    b = (np.float64(STRADDLE_MN) + ks * np.float64(cell)).astype(f32)
    x1 = np.stack([_ulps(b, j) for j in range(-3, 4)], axis=1).ravel()
    up, down = (x1 + rf).astype(f32), (x1 - rf).astype(f32)
    x2 = np.stack([_ulps(up, -k) for k in range(6)] + [_ulps(down, k) for k in range(6)], axis=1)
    x1 = np.repeat(x1[:, None], 12, axis=1)
    return x1.ravel(), x2.ravel()


def straddle_pairs(r):
    """-> (kept [m, 2], control [c, 2]) x coordinates.  kept: neighbours (d2 < r2 in binary32, the kernel's order of
    operations) whose cells under the UN-margined formula floor((x - mn) / r) are two apart — a grid of side r would
    never compare them; control: neighbours next to the borders of the margined grid."""
    rf = f32(r)
    r2 = f32(float(rf) * float(rf))

    def neighbours(x1, x2):
        d = x1 - x2
        return (f32(0) + d * d) + f32(0) + f32(0) < r2

    x1, x2 = _straddle_candidates(rf, rf)
    two = np.abs(cells_of(x2, STRADDLE_MN, rf) - cells_of(x1, STRADDLE_MN, rf)) == 2
    kept = np.unique(np.stack([x1, x2], axis=1)[neighbours(x1, x2) & two], axis=0)
    y1, y2 = _straddle_candidates(rf, rf * CELL_MARGIN)
    ctl = np.unique(np.stack([y1, y2], axis=1)[neighbours(y1, y2)], axis=0)
    return kept, ctl


def _straddle(r):
    """A control case for r = 0.75: the radius is exact in binary32 and so is every quotient at a border — no pair is
    kept, the cloud is the control pairs alone."""
    kept, ctl = straddle_pairs(r)
    n_kept_all = kept.shape[0]
    room = STRADDLE_ROWS * STRADDLE_ROWS
    n_ctl = min(36, ctl.shape[0])
    if kept.shape[0] > room - n_ctl:
        kept = kept[np.linspace(0, kept.shape[0] - 1, room - n_ctl).astype(int)]
    ctl = ctl[np.linspace(0, ctl.shape[0] - 1, n_ctl).astype(int)]
    pairs = np.concatenate([kept, ctl])
    step = np.ceil(3.2 * r * 4) / 4  # >= 3 r between the rows, a multiple of 0.25
    xyz = [(float(STRADDLE_MN), -step, -step)]  # the anchor: pins the box minimum at a value that is not round
    for t, (a, b) in enumerate(pairs):
        y, z = step * (t % STRADDLE_ROWS), step * (t // STRADDLE_ROWS)
        xyz += [(float(a), y, z), (float(b), y, z)]
    m = kept.shape[0]
    return FrontCase(_exact(xyz), _r32(r) / 2, _r32(r), dict(
        n_kept=m, n_kept_found=n_kept_all, pairs=1 + 2 * np.arange(pairs.shape[0]), kept=1 + 2 * np.arange(m), row_step=step))


BALL_M = (61, 63, 64, 65, 127, 128, 129, 255, 256, 257, 372, 373)


def _ball_points(m, rng, radius=0.37, centre=(1.0, -0.5, 0.25)):
    out = np.zeros((0, 3))
    while out.shape[0] < m:
        c = rng.uniform(-radius, radius, (4 * m, 3))
        c = np.round(c * 16384) / 16384
        out = np.unique(np.concatenate([out, c[np.linalg.norm(c, axis=1) < radius]]), axis=0)
    return rng.permutation(out)[:m] + np.asarray(centre)


def _ball(m):
    rng = np.random.default_rng(_seed("ball") + [m])
    return FrontCase(_exact(_ball_points(m, rng)), R_NORMAL, R_FPFH, dict(list_length=m))


def _ball_300_in_lattice():
    rng = np.random.default_rng(_seed("ball_300_in_lattice"))
    ball = _ball_points(300, rng)
    lat = _lattice(10, 10, 1, 0.5, (3.0, -2.0, 0.25))
    xyz, is_ball = [], []
    for t in range(100):  # three ball points, one lattice point: every SPFH block and most FPFH blocks hold both kinds
        xyz += [ball[3 * t], ball[3 * t + 1], ball[3 * t + 2], lat[t]]
        is_ball += [True, True, True, False]
    return FrontCase(_exact(xyz), R_NORMAL, R_FPFH, dict(is_ball=np.array(is_ball), long_length=300, short_max=9))


def _short_lists():
    xyz = [(7, 0, 0),                                                # alone: k = 1
           (5, 0, 0), (5.25, 0, 0),                                  # a pair: k = 2
           (3, 0, 0), (3.625, 0, 0), (3.3125, 0.5625, 0),            # a triple wider than r_normal: k = 3, one point for the normal
           (1, 0, 0.5), (1.25, 0, 0.5), (1, 0.25, 0.5)]              # a triple inside r_normal: a plane from three points
    return FrontCase(_exact(xyz), R_NORMAL, R_FPFH, dict(
        k_fpfh=[1, 2, 2, 3, 3, 3, 3, 3, 3], k_normal=[1, 2, 2, 1, 1, 1, 3, 3, 3]))


def _wide_extent():
    rng = np.random.default_rng(_seed("wide_extent"))
    a = rng.uniform((0, 0, 0), (1.5, 1.0, 0.25), (60, 3))
    b = rng.uniform((188.0, 0, 0), (200.0, 1.0, 0.25), (240, 3))  # across cell 254 | 255 | 256 ... of the unclamped grid
    xyz = np.round(np.concatenate([a, b]) * 1024) / 1024
    return FrontCase(_exact(rng.permutation(xyz)), R_NORMAL, R_FPFH, dict(route="dense", clamped_points=20))


# ---------------------------------------------------------------------------------------------- normals
PLANE_ORIGIN = (0.25, -1.0, 0.75)


def _plane_lattice(shift=(0, 0, 0)):
    return _lattice(8, 8, 1, 0.25, PLANE_ORIGIN) + np.asarray(shift, dtype=np.float64)


def _normal_cases(name):
    if name == "plane_lattice":
        # z = 0.75 > 0: the viewpoint flip turns every normal to (-0, -0, -1)
        return FrontCase(_exact(_plane_lattice()), R_NORMAL, R_FPFH, dict(quadratic_branch=True, normal_bits=(-0.0, -0.0, -1.0, 0.0)))
    if name == "plane_through_origin":
        return FrontCase(_exact(_lattice(9, 9, 1, 0.25, (-1.0, -1.0, 0.0))), R_NORMAL, R_FPFH, dict(
            cos_theta_zero=True, origin_index=4 * 9 + 4))
    if name == "collinear":
        t = np.arange(12)[:, None]
        return FrontCase(_exact(np.array([1.0, -1.0, 0.5]) + t * np.array([0.125, 0.0, 0.0])), R_NORMAL, R_FPFH, dict(
            pattern="nan3_curv0"))
    if name == "collinear_oblique":
        # off the axes the products of the covariance round: the rank-one matrix becomes some rank-two one, and the normal is
        # whatever direction across the line the rounding picks — finite, defined by the operation order alone
        t = np.arange(12)[:, None]
        return FrontCase(_exact(np.array([1.0, -1.0, 0.5]) + t * np.array([0.0625, 0.125, 0.25])), R_NORMAL, R_FPFH, dict(
            finite_normals=8))
    if name == "identical":
        xyz = [(1, 2, 0.5)] * 5 + [(3, 4, 1.5)] * 3
        return FrontCase(_exact(xyz), R_NORMAL, R_FPFH, dict(pattern="nan3_curv0", zero_rows=True, zero_d2_pairs=5 * 4 + 3 * 2))
    if name == "duplicates":
        lat = _lattice(4, 4, 2, 0.25, (0.5, -0.5, 0.5))
        return FrontCase(_exact(np.concatenate([lat, lat, lat])), R_NORMAL, R_FPFH, dict(
            zero_d2_pairs=2 * 96, blocks_below_100=True))
    if name == "octahedron":
        c = np.array([2.0, 1.0, 0.5])
        v = 0.125 * np.concatenate([np.eye(3), -np.eye(3)])
        return FrontCase(_exact(np.concatenate([c + v, c[None]])), R_NORMAL, R_FPFH, dict(curvature_third=True))
    if name == "cube":
        c = np.array([2.0, 1.0, 0.5])
        s = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
        return FrontCase(_exact(c + 0.125 * s), R_NORMAL, R_FPFH, dict(curvature_third=True))
    if name == "far_plane":
        return FrontCase(_exact(_plane_lattice((2000.0, -1500.0, 300.0))), R_NORMAL, R_FPFH, dict(nan_normals=1))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- SPFH and FPFH
def _two_planes(z0, z1):
    a = _lattice(8, 8, 1, 0.25, (0.5, -1.0, z0))
    b = _lattice(8, 8, 1, 0.25, (0.5, -1.0, z1))
    return _exact(np.concatenate([a, b]))


def _feature_cases(name):
    if name == "facing_planes":
        # 0.625 apart: outside r_normal, inside r_fpfh; the origin lies between them, so the normals face each other
        return FrontCase(_two_planes(0.25, -0.375), R_NORMAL, R_FPFH, dict(opposite_normals=True, blocks_below_100=True))
    if name == "stacked_planes":
        return FrontCase(_two_planes(0.5, 1.0), R_NORMAL, R_FPFH, dict(other_layer_at_rn=True, blocks_below_100=True))
    if name == "denormal_d2":
        lat = _lattice(4, 4, 2, 0.125, (0.125, -0.25, 0.125))
        tiny = np.array([[0, 0, 0], [float(f32(1e-20)), 0, 0], [0, float(f32(1e-19)), 0]])
        return FrontCase(_exact(np.concatenate([tiny, lat])), R_NORMAL, R_FPFH, dict(denormal_d2=True, nan_descriptors=1))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- voxel grid
VOXEL_LEAF = 0.25


def _voxel_borders():
    lat = _lattice(9, 9, 3, VOXEL_LEAF, (-1.0, -1.0, -0.25)).astype(f32)
    below = np.nextafter(lat, f32(-np.inf))
    xyz = np.empty((2 * lat.shape[0], 3), dtype=np.float64)
    xyz[0::2], xyz[1::2] = lat, below
    return FrontCase(_exact(xyz), R_NORMAL, R_FPFH, dict(leaf=VOXEL_LEAF, n_voxels=2 * 9 * 9 * 3 - 8 * 8 * 2))


# ---------------------------------------------------------------------------------------------- the table
NEIGHBOUR_NAMES = (("lattice3d",) + tuple(f"straddle_{r}" for r in STRADDLE_R) + tuple(f"ball_{m}" for m in BALL_M)
                   + ("ball_300_in_lattice", "short_lists", "wide_extent"))
NORMAL_NAMES = ("plane_lattice", "plane_through_origin", "collinear", "collinear_oblique", "identical", "duplicates", "octahedron", "cube", "far_plane")
FEATURE_NAMES = ("facing_planes", "stacked_planes", "denormal_d2")
FPFH_NAMES = NEIGHBOUR_NAMES + NORMAL_NAMES + FEATURE_NAMES
VOXEL_NAMES = ("voxel_borders",)
NAMES = FPFH_NAMES + VOXEL_NAMES
# neighbourhoods without an independent answer (coincident, collinear or isotropic points, cancelled covariances, fewer
# than three points): numpy's eigh is no judge there, the CPU test only records the oracle's pattern.  A fixed list
DEGENERATE = ("lattice3d", "collinear", "collinear_oblique", "identical", "octahedron", "cube", "far_plane", "denormal_d2") + tuple(
    f"straddle_{r}" for r in STRADDLE_R)
# cases whose lists exceed the slot: the keyframe route runs them on a fresh and on a warm handle
LONG_LIST_NAMES = tuple(f"ball_{m}" for m in BALL_M if m > QTR_KMAX) + ("ball_300_in_lattice",)


def _make(name):
    if name == "lattice3d":
        return _lattice3d()
    if name.startswith("straddle_"):
        return _straddle(float(name[9:]))
    if name == "ball_300_in_lattice":
        return _ball_300_in_lattice()
    if name.startswith("ball_"):
        return _ball(int(name[5:]))
    if name == "short_lists":
        return _short_lists()
    if name == "wide_extent":
        return _wide_extent()
    if name in NORMAL_NAMES:
        return _normal_cases(name)
    if name in FEATURE_NAMES:
        return _feature_cases(name)
    if name == "voxel_borders":
        return _voxel_borders()
    raise KeyError(name)


_cache = {}


def case(name):
    """(cached: the cloud is shared and read-only)"""
    if name not in _cache:
        c = _make(name)
        assert c.cloud.shape[0] <= 700 and c.cloud.dtype == f32
        c.cloud.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def keyframe_leaf(name):
    """The voxel leaf of the keyframe route.  2^-10 where every point then is a voxel of its own and the grid fits int32;
    where it does not fit (the wide clouds) pcl::VoxelGrid hands the cloud back as it is, which serves as well; 1e-6 for
    the clouds with coincident or nearly coincident points: their grid overflows and they pass through unmerged."""
    return 1e-6 if name in ("identical", "duplicates", "denormal_d2") else 2.0 ** -10


def same_bits(a, b):
    """bit for bit, NaN equal to NaN (whatever its payload): (bits equal) | (both NaN)"""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------- the SPFH angle bin
ANGLE_BIN_C = ((0.95949297361449748, 0.2817325568414295), (0.6548607339452851, 0.75574957435425827),
               (0.14231483827328512, 0.98982144188093268), (-0.41541501300188632, 0.90963199535451844),
               (-0.84125353283118109, 0.54064081745559778))
ANGLE_BIN_N = 400000
AngleBinInputs = namedtuple("AngleBinInputs", "y x uniform zero_y nonfinite out_of_guard")


def angle_bin_inputs():
    """(y, x) for the first SPFH block's bin, floor(11 (atan2f(y, x) + pi) / 2 pi): uniform directions, directions within
    4e-6 rad of every bin boundary (both sides, also of the cut at +-pi and of 0), y = +-0 with both signs of x,
    magnitudes from 1e-12 to 1e6, magnitudes around both guards of spfh_bin_of_angle (1e-31 .. 1e-29, 1e29 .. 1e31),
    denormals, +-inf and NaN.  The masks: `uniform` the uniform directions at ordinary magnitudes, `zero_y`, `nonfinite`
    and `out_of_guard` (|y| + |x| in binary32 not inside (1e-30f, 1e30f)) the inputs the shortcut must leave alone."""
    rng = np.random.default_rng(6)
    d_pi = float(f32(1.0) / (f32(2.0) * f32(np.pi)))
    T = np.array([k / (11 * d_pi) - np.pi for k in range(0, 12)])
    n = ANGLE_BIN_N
    phi = np.concatenate([rng.uniform(-np.pi, np.pi, n),
                          (T[rng.integers(0, 12, n)] + rng.uniform(-4e-6, 4e-6, n)),
                          rng.uniform(-4e-6, 4e-6, n // 4), np.pi - rng.uniform(0, 4e-6, n // 4), -np.pi + rng.uniform(0, 4e-6, n // 4)])
    r = np.exp(rng.uniform(np.log(1e-12), np.log(1e6), phi.size))
    y, x = (r * np.sin(phi)).astype(f32), (r * np.cos(phi)).astype(f32)
    y[:2000:4], y[1:2000:4] = f32(0.0), f32(-0.0)                      # atan2f(-0, x < 0) = -pi rounds below -pi: bin 0
    uniform = np.zeros(y.size, dtype=bool)
    uniform[2000:n] = True
    g = np.random.default_rng(7)
    ys, xs = [y], [x]
    for lo, hi in ((1e-31, 1e-29), (1e29, 1e31), (1e-45, 1.2e-38)):   # both guards, denormals
        m = 20000
        ph = np.concatenate([g.uniform(-np.pi, np.pi, m // 2), T[g.integers(0, 12, m // 2)] + g.uniform(-4e-6, 4e-6, m // 2)])
        rr = np.exp(g.uniform(np.log(lo), np.log(hi), m))
        with np.errstate(under="ignore"):
            ys.append((rr * np.sin(ph)).astype(f32))
            xs.append((rr * np.cos(ph)).astype(f32))
    special = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40, 3e38, -3e38]
    ys.append(np.array([a for a in special for b in special], dtype=f32))
    xs.append(np.array([b for a in special for b in special], dtype=f32))
    mags = np.array([1e-40, 1e-30, 1e-12, 1.0, 1e6, 1e30, 3e38], dtype=f32)  # y = +-0 with both signs of x
    ys.append(np.array([z for z in (0.0, -0.0) for sx in (1, -1) for _ in mags], dtype=f32))
    xs.append(np.concatenate([sx * mags for z in (0.0, -0.0) for sx in (1, -1)]).astype(f32))
    y, x = np.concatenate(ys), np.concatenate(xs)
    uniform = np.concatenate([uniform, np.zeros(y.size - uniform.size, dtype=bool)])
    with np.errstate(all="ignore"):
        s = np.abs(y) + np.abs(x)
        out_of_guard = ~(s > f32(1e-30)) | ~(s < f32(1e30))
    return AngleBinInputs(y, x, uniform, y == 0, ~np.isfinite(y) | ~np.isfinite(x), out_of_guard)


def angle_bin_mirror(y, x):
    """numpy mirror (binary32, no contraction) of spfh_bin_of_angle: -> (sure, bin where sure); -1 elsewhere is the
    device's "not sure" """
    with np.errstate(all="ignore"):
        ya, s = np.abs(y), np.abs(y) + np.abs(x)
        c = [f32(ca) * ya - f32(sa) * x for ca, sa in ANGLE_BIN_C]      # (float32 products, float32 difference)
        low = np.minimum.reduce([np.abs(v) for v in c])
        # (numpy's minimum hands a NaN on where fminf drops it: no difference here, a NaN c needs a non-finite input, and
        # then s is inf or NaN and fails s < 1e30f on both sides)
        sure = (low > f32(1e-6) * s) & (s > f32(1e-30)) & (s < f32(1e30)) & (ya != 0)
        m = sum((v > 0).astype(np.int64) for v in c)
        got = np.where(y > 0, 5 + m, 5 - m)
    return sure, got


def angle_bin_want(qo, y, x):
    """the oracle's plain arithmetic: qm_atan2f (qo_math 0), then floor(11 (f1 + pi) d_pi) in binary64"""
    d_pi = float(f32(1.0) / (f32(2.0) * f32(np.pi)))
    f1 = qo.math_fn(0, y, x).astype(np.float64)
    with np.errstate(all="ignore"):
        g = 11.0 * ((f1 + np.pi) * d_pi)
        return np.where(g != g, 0, np.clip(np.floor(g), 0, 10)).astype(np.int64)
