"""Named inputs for the finalize stage (k_finalize in quatro_amd/csrc/solver.hip: chain TIMs, GNC-TLS rotation by gnc_wave /
gnc3_wave, rotation inliers, COTE by cote_axis4, final inliers) and for the stage entry points that run the same device
code (quatro_amd/csrc/stages.hip).  A plain module: deterministic numpy generators, no fixtures, no GPU work.  Used by
tests/test_finalize_cases_cpu.py (the oracle against second restatements, the recipes against what they claim) and
tests/test_gpu_finalize_edges.py (the device against the oracle, bit for bit).

Three families:

    GNC cases      gnc_case(name, dim) -> GncCase(X, Y, noise_bound, gnc_factor, max_it, cost_thr), X / Y: M x dim TIMs
    COTE cases     cote_case(name)     -> CoteCase(X, ranges): one range (float) or one per element; run with the median
                                          on and off
    solve cases    solve_case(name)    -> SolveCase(src, tgt, kw, M, side): L x 4 binary32 correspondences whose maximum
                                          clique has exactly M members, the parameters, and which side of the COTE switch
                                          the COTE population N lands on

The kernel picks the memory layout of every array from the clique size M and the COTE population N; the switch values
are derived below from FIN_LDS_BYTES with the kernel's own byte formulas, and a CPU test compares the constant with the
#define in solver.hip.
"""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------------------------- mirrored constants
FIN_LDS_BYTES = 152 * 1024


def _r16(n):
    return (n + 15) & ~15


def cote_lds_bytes(N):
    """k_finalize's LDS need of three COTE axes at population N: per axis the sorted X (16 N bytes), the sorted positions
    (8 N), six term arrays (16 N each), every array rounded up to 16 bytes"""
    return 3 * (7 * _r16(16 * N) + _r16(8 * N))


M_LDS_YAW = FIN_LDS_BYTES // 40     # 5 arrays of M doubles (X0 X1 Y0 Y1 Wt): the last M with the GNC arrays in LDS
M_LDS_3DOF = FIN_LDS_BYTES // 56    # 7 arrays in the 3-DoF mode
M_LDS_CHAIN = FIN_LDS_BYTES // 64   # 8 M doubles: the in-kernel range-sum chain behind the GNC arrays
N_LDS_COTE = max(n for n in range(1, 2000) if cote_lds_bytes(n) <= FIN_LDS_BYTES)

GNC_DEFAULTS = (0.6, 1.4, 50, 1.1e-4)  # rotation bound 2 x 0.3, factor, iterations, cost threshold of the demo

GncCase = namedtuple("GncCase", "X Y noise_bound gnc_factor max_it cost_thr")
CoteCase = namedtuple("CoteCase", "X ranges")
SolveCase = namedtuple("SolveCase", "src tgt kw M side")  # side: "lds" / "global" (COTE arrays), or None: not claimed


def _seed(name):
    return [ord(c) for c in name]


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ---------------------------------------------------------------------------------------------- GNC cases
def _rot(dim, rng):
    if dim == 2:
        a = rng.uniform(-np.pi, np.pi)
        return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _planted_tims(M, dim, rng, noise=0.02, frac_out=0.3):
    X = rng.uniform(-10, 10, (M, dim))
    Y = X @ _rot(dim, rng).T + rng.normal(0, noise, (M, dim))
    out = rng.random(M) < frac_out
    Y[out] = rng.uniform(-10, 10, (int(out.sum()), dim))
    return X, Y


PLANTED_M = (1, 2, 63, 64, 65, 127, 128, 129, 4097)  # both sides of each 64-lane stride boundary


def _gnc(name, dim):
    rng = np.random.default_rng(_seed(name) + [dim])
    nb, fac, mit, thr = GNC_DEFAULTS
    z = np.zeros((dim, dim))
    quarter = z.copy()
    quarter[0, 1], quarter[1, 0] = -1.0, 1.0
    if dim == 3:
        quarter[2, 2] = 1.0
    if name == "mu_inf":
        # H has R = I exactly, every r^2 = 2 a^2, 2 max_r / nb^2 - 1 = 0: mu = 1 / 0.  The members in the order of a square's
        # sides and the signs alternating, so that the same TIMs are the chain TIMs of four points whose diagonals keep
        # their lengths (solve_case("mu_inf"))
        a = 0.25
        X = np.array([[1.0, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]])
        Y = X + np.array([1.0, -1, 1, -1])[:, None] * np.array([a, a, 0.0])
        return GncCase(X[:, :dim].copy(), Y[:, :dim].copy(), 2 * a, fac, mit, thr)
    if name == "all_exact":
        X = rng.integers(-9, 10, (40, dim)).astype(np.float64)
        return GncCase(X, X @ quarter.T, nb, fac, mit, thr)
    if name == "zero":
        return GncCase(np.zeros((5, dim)), np.zeros((5, dim)), nb, fac, mit, thr)
    if name == "half_turn":
        X = rng.integers(-9, 10, (30, dim)).astype(np.float64)
        D = np.diag([-1.0, -1.0, 1.0][:dim])
        return GncCase(X, X @ D, nb, fac, mit, thr)
    if name == "mirror":
        X = rng.uniform(-10, 10, (50, 3))
        return GncCase(X, X @ np.diag([1.0, 1.0, -1.0]), nb, fac, mit, thr)
    if name == "collinear":
        d = np.array([3.0, 4.0, 12.0][:dim])
        X = rng.integers(-8, 9, 25).astype(np.float64)[:, None] * d
        return GncCase(X, X @ quarter.T, nb, fac, mit, thr)
    if name == "planar":
        X = rng.uniform(-10, 10, (40, 3))
        X[:, 2] = 0.0
        return GncCase(X, X @ _rot(3, rng).T, nb, fac, mit, thr)
    if name == "all_outliers":
        X = rng.uniform(-10, 10, (48, dim))
        Y = rng.uniform(-10, 10, (48, dim)) + 30.0
        return GncCase(X, Y, nb, fac, 200, thr)
    if name == "huge":
        X = rng.uniform(0.5, 1.0, (20, dim)) * 1e200
        return GncCase(X, X @ quarter.T, nb, fac, mit, thr)
    if name == "tiny":
        X = rng.uniform(0.5, 1.0, (20, dim)) * 1e-170
        return GncCase(X, X @ quarter.T, nb, fac, mit, thr)
    if name in ("nan_member", "inf_member"):
        X, Y = _planted_tims(100, dim, rng)
        if name == "nan_member":
            Y[37, 0] = np.nan
        else:
            X[37, dim - 1] = np.inf
        return GncCase(X, Y, nb, fac, mit, thr)
    if name == "tiny_bound":
        X, Y = _planted_tims(90, dim, rng)
        return GncCase(X, Y, 1e-9, fac, mit, thr)
    if name == "never_converges":
        X, Y = _planted_tims(150, dim, rng)
        return GncCase(X, Y, nb, fac, 7, 0.0)
    if name == "one_round":
        X, Y = _planted_tims(150, dim, rng)
        return GncCase(X, Y, nb, fac, mit, np.inf)
    if name.startswith("planted_"):
        X, Y = _planted_tims(int(name[8:]), dim, rng)
        return GncCase(X, Y, nb, fac, mit, thr)
    raise KeyError(name)


GNC_3D_ONLY = ("mirror", "planar")
GNC_NAMES = ("mu_inf", "all_exact", "zero", "half_turn", "mirror", "collinear", "planar", "all_outliers", "huge", "tiny",
             "nan_member", "inf_member", "tiny_bound", "never_converges", "one_round") + tuple(
                 f"planted_{m}" for m in PLANTED_M)
GNC_CASES = [(n, d) for n in GNC_NAMES for d in (2, 3) if d == 3 or n not in GNC_3D_ONLY]
# the optimum of the first round is not unique (or H is 0): the rotation is compared through trace(R H), not entry by entry
GNC_NONUNIQUE = ("zero", "collinear", "half_turn", "mirror", "planar", "tiny")
# what a numpy restatement cannot judge (numpy's SVD does not converge on NaN / inf): hand-stated facts instead.  `huge`
# is here because H itself overflows to inf.  A fixed list: no case is skipped by a condition found at run time
GNC_NOT_RESTATED = ("mu_inf", "nan_member", "inf_member", "huge")

# ---------------------------------------------------------------------------------------------- COTE cases
LADDER_N = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 255, 256, 257, 432, 433, 1024, 1025, 2049)


def _cluster(N, rng):
    """two thirds of the members in a tight cluster, one third spread wide"""
    return np.concatenate([1.5 + 0.1 * rng.standard_normal(N - N // 3), rng.uniform(-20, 20, N // 3)])


def _cote(name):
    rng = np.random.default_rng(_seed(name))
    if name.startswith("same_key"):
        # 40 different X that round onto a handful of keys X - 4 (ulp 2^-51) and X + 4 (ulp 2^-50), descending by position:
        # among equal keys the order goes by position, not by X — the median's "not ascending" fall-back
        X = 1.0 + np.arange(40, 0, -1) * 2.0 ** -52
        if name == "same_key_outliers":
            X = np.concatenate([X, [50.0, -70.0, 90.0]])
        elif name == "same_key_embedded":
            X = np.insert(rng.normal(1.0, 2.0, 300), 150, X)
        return CoteCase(X, 4.0)
    if name == "all_equal":
        return CoteCase(np.full(37, 0.7), 0.3)
    if name == "disjoint":
        return CoteCase(10.0 * rng.permutation(23), 0.3)
    if name == "n1":
        return CoteCase(np.array([2.5]), 0.3)
    if name == "nested_ranges":
        X = rng.uniform(-1, 1, 60)
        R = rng.uniform(0.01, 0.05, 60)
        R[17] = 100.0
        return CoteCase(X, R)
    if name == "range_ties":
        # X on a 0.5 grid, ranges of 0.25 / 0.5 / 0.75: the opening key of one member equals the closing key of another
        return CoteCase(rng.integers(-6, 7, 150) * 0.5, rng.choice([0.25, 0.5, 0.75], 150))
    if name == "zero_range":
        return CoteCase(_cluster(30, rng), 0.0)
    if name == "huge":
        return CoteCase(1e300 * np.array([1.0, 1.05, 1.02, 3.0, 1.01, 0.98, 1.7, 1.03]), 1e299)
    if name == "cost0_nan":
        # the first event's cost is inf - inf (x^2 + x^2 overflows), the far member closes at once and every running sum
        # returns to 0 exactly: NaN first, finite costs after it — Eigen's minCoeff stays on the first
        return CoteCase(np.concatenate([[-1.2e154], _cluster(45, rng)]), 0.3)
    if name in ("nan_mid", "nan_first"):
        X = _cluster(90, rng)
        X[0 if name == "nan_first" else 41] = np.nan
        return CoteCase(X, 0.3)
    if name == "inf_both":
        X = _cluster(60, rng)
        X[11], X[40] = np.inf, -np.inf
        return CoteCase(X, 0.3)
    if name == "all_nan":
        return CoteCase(np.full(9, np.nan), 0.3)
    if name.startswith("ladder_grid_"):
        return CoteCase(np.round(_cluster(int(name[12:]), rng) * 2) / 2, 0.25)
    if name.startswith("ladder_ranges_"):
        N = int(name[14:])
        return CoteCase(_cluster(N, rng), rng.uniform(0.05, 0.6, N))
    if name.startswith("ladder_"):
        return CoteCase(_cluster(int(name[7:]), rng), 0.3)
    raise KeyError(name)


COTE_NAMES = ("same_key", "same_key_outliers", "same_key_embedded", "all_equal", "disjoint", "n1", "nested_ranges",
              "range_ties", "zero_range", "huge", "cost0_nan", "nan_mid", "nan_first", "inf_both", "all_nan") + tuple(
                  f"ladder_{k}{n}" for n in LADDER_N for k in ("", "grid_", "ranges_"))
# non-finite inputs and the range of 0 (every weight inf): hand-stated facts instead of the restatement.  A fixed list
COTE_NOT_RESTATED = ("zero_range", "nan_mid", "nan_first", "inf_both", "all_nan")
# two endpoints on exactly one key: the reference's std::sort compares keys alone and leaves their order unspecified
# (declared divergence D3: the oracle sorts by (key, position)), so the compiled reference is no judge of these
COTE_TIED_KEYS = ("same_key", "same_key_outliers", "same_key_embedded", "all_equal", "range_ties", "cost0_nan") + tuple(
    f"ladder_grid_{n}" for n in LADDER_N if n >= 2)


# ---------------------------------------------------------------------------------------------- solve-level cases
def _rx(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def _pack(src, tgt):
    s4 = np.zeros((src.shape[0], 4), np.float32)
    t4 = np.zeros((src.shape[0], 4), np.float32)
    s4[:, :3], t4[:, :3] = src, tgt
    return s4, t4


def planted(M, n_out, seed=0, noise=0.02, tilt=0.0, mirror=False, zspan=40.0):
    """M inliers under one rigid motion with uniform noise of +-`noise` per axis — far inside the noise bound, so the
    inliers are pairwise consistent: a clique — then n_out uniform outliers (independent points in both clouds), then a
    permutation.  tilt: a roll of that many radians on top of the yaw — lengths stay consistent, the yaw-only model cannot
    fit, GNC iterates with weights in all three bands and the rotation inliers are a strict subset.  mirror: the target
    is the reflection in z of the moved source (for the 3-DoF mode, with zspan = 0.5: a thin slab).  -> (src4, tgt4)"""
    rng = np.random.default_rng([seed, M, n_out, int(round(tilt * 1e6)), int(mirror)])
    L = M + n_out
    half = np.array([40.0, 40.0, zspan])
    src = rng.uniform(-half, half, (L, 3))
    R = _rz(rng.uniform(-3, 3)) @ _rx(tilt)
    t = rng.uniform(-2, 2, 3)
    tgt = src @ R.T + t + rng.uniform(-noise, noise, (L, 3))
    if mirror:
        tgt[:, 2] = -tgt[:, 2]
    tgt[M:] = rng.uniform(-half, half, (n_out, 3))
    p = rng.permutation(L)
    return _pack(src[p], tgt[p])


def _mu_inf_points():
    """four correspondences whose chain TIMs are gnc_case("mu_inf", 2): the corners of a unit square and where its sides
    go; the diagonals keep their lengths, the sides change by at most 0.28: pairwise consistent under beta = 2 x 0.25"""
    c = _gnc("mu_inf", 3)
    src = np.concatenate([np.zeros((1, 3)), np.cumsum(c.X[:3], axis=0)])
    tgt = np.concatenate([np.zeros((1, 3)), np.cumsum(c.Y[:3], axis=0)])
    return _pack(src, tgt)


def _all_exact_points(M, n_out):
    """M distinct lattice points under a quarter turn and an integer shift, exact in binary32: every residual is 0"""
    rng = np.random.default_rng([7, M, n_out])
    cells = rng.permutation(81 * 81 * 11)[:M]
    src = np.stack([cells % 81 - 40, (cells // 81) % 81 - 40, cells // 6561 - 5], axis=1).astype(np.float64)
    tgt = src @ _rz(np.pi / 2).round().T + np.array([3.0, -2.0, 1.0])
    L = M + n_out
    src = np.concatenate([src, rng.uniform(-40, 40, (n_out, 3))])
    tgt = np.concatenate([tgt, rng.uniform(-40, 40, (n_out, 3))])
    p = rng.permutation(L)
    return _pack(src[p], tgt[p])


TILT = 0.01
MU_INF_NOISE_BOUND = 0.25  # the rotation stage's bound is twice this: 2 a
RYRX = [0.9998, 0, 0.02, 0, 1, 0, -0.02, 0, 0.9998]
VARIANTS = {"median0": dict(cote_median=0), "cnb0.1": dict(cote_noise_bound=0.1),
            "ryrx": dict(using_pre_estimated_ryrx=1, ryrx=RYRX), "rotinl": dict(using_rot_inliers_when_estimating_cote=1)}
# the rot-inlier option takes COTE's population from the rotation inliers: one input on either side of the COTE switch
# (seed and tilt found by a scan on the CPU oracle; the CPU test asserts where n_rot_inliers lands)
ROTINL_PAIR = {"rotinl_lds": (500, 4, 0.01), "rotinl_global": (500, 2, 0.01)}  # 432 and 436 rotation inliers


def _side(N):
    return "lds" if N <= N_LDS_COTE else "global"


def _solve(name):
    if name.startswith("yaw_"):
        M = int(name[4:])
        return SolveCase(*planted(M, 150, tilt=TILT), {}, M, _side(M))
    if name.startswith("3dof_"):
        M = int(name[5:])
        return SolveCase(*planted(M, 150, mirror=True, zspan=0.5), dict(reg_mode=1), M, _side(M))
    if name.startswith("var_"):
        _, M, v = name.split("_")
        M = int(M)
        return SolveCase(*planted(M, 150, tilt=TILT), VARIANTS[v], M, None if v == "rotinl" else _side(M))
    if name in ROTINL_PAIR:
        M, seed, tilt = ROTINL_PAIR[name]
        return SolveCase(*planted(M, 150, seed=seed, tilt=tilt), VARIANTS["rotinl"], M, name[7:])
    if name.startswith("mu_inf"):
        kw = dict(noise_bound=MU_INF_NOISE_BOUND)
        if name == "mu_inf_rotinl":
            kw.update(VARIANTS["rotinl"])
        return SolveCase(*_mu_inf_points(), kw, 4, "lds")
    if name == "all_exact_433":
        return SolveCase(*_all_exact_points(433, 150), {}, 433, "global")
    if name.startswith("cnb_"):
        # cote_noise_bound values whose range-sum table the host does not lay down (0) or lays down at the ends of the
        # exponent range; 0 is the only way into the in-kernel chain and its two locations
        _, v, M = name.split("_")
        M = int(M)
        return SolveCase(*planted(M, 150, tilt=TILT), dict(cote_noise_bound=float(v)), M, _side(M))
    raise KeyError(name)


YAW_M = (N_LDS_COTE - 1, N_LDS_COTE, N_LDS_COTE + 1, M_LDS_CHAIN, M_LDS_CHAIN + 1, M_LDS_YAW, M_LDS_YAW + 1)
DOF3_M = (N_LDS_COTE, N_LDS_COTE + 1, M_LDS_3DOF, M_LDS_3DOF + 1)
CNB0_M = (300, M_LDS_CHAIN, M_LDS_CHAIN + 1, M_LDS_YAW + 1)  # the last one: the chain in scratch next to GNC arrays in scratch
SOLVE_NAMES = (tuple(f"yaw_{m}" for m in YAW_M) + tuple(f"3dof_{m}" for m in DOF3_M)
               + tuple(f"var_{m}_{v}" for m in (N_LDS_COTE + 1, M_LDS_YAW + 1) for v in VARIANTS)
               + tuple(ROTINL_PAIR) + ("mu_inf", "mu_inf_rotinl", "all_exact_433")
               + tuple(f"cnb_0_{m}" for m in CNB0_M) + ("cnb_1e-300_300", "cnb_1e200_300"))
SOLVE_ITERATES = tuple(n for n in SOLVE_NAMES if n.split("_")[0] in ("yaw", "3dof", "var", "rotinl", "cnb"))

_cache = {}


def _cached(kind, key, make):
    if (kind, key) not in _cache:
        c = make()
        _freeze(*c)
        _cache[(kind, key)] = c
    return _cache[(kind, key)]


def gnc_case(name, dim):
    """(cached: the arrays are shared and read-only)"""
    return _cached("gnc", (name, dim), lambda: _gnc(name, dim))


def cote_case(name):
    return _cached("cote", name, lambda: _cote(name))


def solve_case(name):
    return _cached("solve", name, lambda: _solve(name))


def same_bits(a, b):
    """bit for bit, NaN equal to NaN (whatever its payload), +inf to +inf"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
