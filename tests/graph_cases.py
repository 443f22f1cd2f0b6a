"""Adversarial correspondence sets for the consistency-graph kernels (k_graph_build_tiles / k_graph_build /
k_graph_build_mfma in quatro_amd/csrc/solver.hip).  A plain module: deterministic generators, no fixtures.

Every case is a block of B = min(512, L // 2) adversarial correspondences at a seeded position among uniform outliers
(independent random points in both clouds: a sparse graph around the block, a short solve).  Correspondence 0 is an
ordinary outlier unless the case says otherwise.  The predicate under test is the reference's solveForScale,
|b/a - 1| <= beta/a AND |a/b - 1| <= beta/b with a, b the lengths of a pair's source and target TIM and
beta = 2 noise_bound sqrt(cbar2), i.e. |b - a| <= beta up to its own roundings; the cases put |b - a| where the kernels'
screens and guards have to hand the pair to the binary64 expression:

    band(beta)        collinear block, half of the targets shifted along the line by beta (1 + r), r = +-10^U(-9, -2),
                      each cloud under its own random rigid motion: ||b - a| - beta| from below a binary32 ulp of the
                      coordinates to beyond the screens' margins
    exact_ties        integer lattice, targets + 0.5 for a random half, beta = 0.5: |b - a| == beta exactly in binary64,
                      the reference's own roundings decide
    flat              band(0.6) unrotated, the other two coordinates within 1e-3 m of correspondence 0's: the second
                      binary16 halves of the MFMA kernel's operands are subnormal
    short_tims        clusters with TIMs of beta / 4 .. 2 beta in both clouds, exact duplicates (0/0 in the reference),
                      one-ulp near-duplicates
    far_origin(d)     band(0.6) with correspondence 0 moved d metres away: squared norms relative to it just below, just
                      above and far above the MFMA kernel's range limit of 1e5
    map_frame[_wide]  band(0.6) in map coordinates (3.2e4, -4.7e4, 150): coordinate ulp 2-4 mm; _wide spreads the outliers
                      over +-400 m so that s + t crosses GB_SMAX
    nonfinite[_row0]  band(0.6) with NaN, +inf, -inf rows in either cloud; _row0 puts one in row 0 (the MFMA origin)
    tiny_beta(beta)   band at beta = 0.004 and beta = 0.01 exactly: the binary32 screens and the MFMA screen are off
"""
from collections import namedtuple

import numpy as np

GraphCase = namedtuple("GraphCase", "name src tgt noise_bound cbar2 block")  # block = (lo, hi): rows lo .. hi - 1

BLOCK = 512
MAP_OFFSET = np.array([3.2e4, -4.7e4, 150.0])


def beta_of(noise_bound, cbar2=1.0):
    return 2 * noise_bound * np.sqrt(cbar2)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _outliers(rng, L, spread=50.0):
    """(src, tgt, lo, B): independent uniform points in both clouds (float64) and where the block goes"""
    B = min(BLOCK, L // 2)
    lo = int(rng.integers(1, L - B + 1))
    return rng.uniform(-spread, spread, (L, 3)), rng.uniform(-spread, spread, (L, 3)), lo, B


def _line_block(rng, B, beta, x=None):
    """sources (x, 0, 0), targets the same, a random half of them shifted along the line by beta (1 + r)"""
    if x is None:
        x = rng.uniform(-50.0, 50.0, B)
    r = rng.choice([-1.0, 1.0], B) * 10.0 ** rng.uniform(-9.0, -2.0, B)
    off = np.where(rng.random(B) < 0.5, beta * (1.0 + r), 0.0)
    s = np.zeros((B, 3))
    s[:, 0] = x
    t = s.copy()
    t[:, 0] += off
    return s, t


def _finish(name, src, tgt, beta, lo, B):
    s4 = np.zeros((src.shape[0], 4), np.float32)
    t4 = np.zeros((tgt.shape[0], 4), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s4[:, :3] = src
        t4[:, :3] = tgt
    return GraphCase(name, s4, t4, beta / 2, 1.0, (lo, lo + B))  # (halving is exact: 2 noise_bound == beta)


def band(L, beta, seed=0, name=None, rotate=True, spread=50.0, origin_d=0.0, translate=None, radial_block=False):
    """The family's base case.  origin_d: correspondence 0 that far from the clouds' centre (before the rigid motions);
    radial_block: the block's line points at correspondence 0, starts 120 m closer to it and is sorted along the line —
    64-row blocks at distinct distances from the origin."""
    rng = np.random.default_rng([seed, int(round(beta * 1e6)), L])
    half = 35.0 if origin_d else 50.0  # (far origin: a cloud radius of 60.6 m keeps (250 + 60.6)^2 below 1e5)
    src, tgt, lo, B = _outliers(rng, L, spread if not origin_d else half)
    x = None
    if origin_d:
        x = rng.uniform(-half, half, B)
        if radial_block:
            x = np.sort(x + 120.0)
    bs, bt = _line_block(rng, B, beta, x)
    c = rng.uniform(-5.0, 5.0, 3) * (0.0 if origin_d else 1.0)  # the line passes near the centre
    src[lo:lo + B], tgt[lo:lo + B] = bs + c, bt + c
    if origin_d:
        src[0] = tgt[0] = np.array([origin_d, 0.0, 0.0])
    if rotate:
        Rs, Rt = _rotation(rng), _rotation(rng)
        ts, tt = rng.uniform(-3.0, 3.0, 3), rng.uniform(-3.0, 3.0, 3)
        src, tgt = src @ Rs.T + ts, tgt @ Rt.T + tt
    if translate is not None:
        src, tgt = src + translate, tgt + translate
    return _finish(name or f"band_{beta:g}", src, tgt, beta, lo, B)


def exact_ties(L, seed=0):
    rng = np.random.default_rng([seed, 101, L])
    src, tgt, lo, B = _outliers(rng, L)
    k = rng.permutation(B).astype(np.float64) - B // 2  # the lattice 0 .. B-1, centred on the cloud, in random order
    bs = np.zeros((B, 3))
    bs[:, 0] = k
    bs[:, 1], bs[:, 2] = 3.0, -7.0
    bt = bs.copy()
    bt[:, 0] += np.where(rng.random(B) < 0.5, 0.5, 0.0)
    src[lo:lo + B], tgt[lo:lo + B] = bs, bt
    return _finish("exact_ties", src, tgt, 0.5, lo, B)


def flat(L, seed=0):
    beta = 0.6
    rng = np.random.default_rng([seed, 102, L])
    src, tgt, lo, B = _outliers(rng, L)
    bs, bt = _line_block(rng, B, beta)
    for cloud, blk in ((src, bs), (tgt, bt)):
        # (correspondence 0 close to the x axis: the flat coordinates keep bits below their first binary16 half)
        cloud[0, 1:] = rng.uniform(-0.05, 0.05, 2)
        blk[:, 1:] = cloud[0, 1:] + rng.uniform(-1e-3, 1e-3, (B, 2))
        cloud[lo:lo + B] = blk
    return _finish("flat", src, tgt, beta, lo, B)


def short_tims(L, seed=0):
    beta = 0.6
    rng = np.random.default_rng([seed, 103, L])
    src, tgt, lo, B = _outliers(rng, L)
    bs, bt = np.zeros((B, 3)), np.zeros((B, 3))
    n = 0
    while n < B:
        m = min(int(rng.integers(8, 33)), B - n)
        d = rng.uniform(beta / 4, 2 * beta)  # the cluster's diameter, the same in both clouds
        cs, ct = rng.uniform(-45.0, 45.0, 3), rng.uniform(-45.0, 45.0, 3)
        bs[n:n + m] = cs + rng.uniform(-0.5, 0.5, (m, 3)) * d / np.sqrt(3.0)
        bt[n:n + m] = ct + rng.uniform(-0.5, 0.5, (m, 3)) * d / np.sqrt(3.0)
        if m >= 8:
            bs[n + 1], bt[n + 1] = bs[n], bt[n]   # duplicate in both clouds: 0/0
            bs[n + 3] = bs[n + 2]                   # duplicate in the source alone: b/0
            bt[n + 5] = bt[n + 4]                   # ... in the target alone
        n += m
    src[lo:lo + B], tgt[lo:lo + B] = bs, bt
    c = _finish("short_tims", src, tgt, beta, lo, B)
    # one-ulp near-duplicates (after the rounding to binary32): every 16th block row copies its predecessor, one ulp off
    # on one axis — in both clouds, in the source alone, in the target alone
    for i, r in enumerate(range(lo + 7, lo + B, 16)):
        ax = i % 3
        if i % 3 != 2:
            c.src[r] = c.src[r - 1]
            c.src[r, ax] = np.nextafter(c.src[r, ax], np.float32(np.inf))
        if i % 3 != 1:
            c.tgt[r] = c.tgt[r - 1]
            c.tgt[r, ax] = np.nextafter(c.tgt[r, ax], np.float32(-np.inf))
    return c


def far_origin(L, d, seed=0):
    return band(L, 0.6, seed=seed + 7 * int(d), name=f"far_origin_{d:g}", origin_d=float(d), radial_block=(d == 330))


def map_frame(L, wide=False, seed=0):
    return band(L, 0.6, seed=seed + (41 if wide else 40), name="map_frame_wide" if wide else "map_frame",
                spread=400.0 if wide else 50.0, translate=MAP_OFFSET)


def nonfinite(L, row0=False, seed=0):
    c = band(L, 0.6, seed=seed + (51 if row0 else 50), name="nonfinite_row0" if row0 else "nonfinite")
    rng = np.random.default_rng([seed, 104, L, int(row0)])
    lo, hi = c.block
    rows = np.concatenate([rng.choice(np.arange(lo, hi), 4, replace=False),
                           rng.choice(np.setdiff1d(np.arange(1, L), np.arange(lo, hi)), 3, replace=False), [L - 1]])
    vals = [np.nan, np.inf, -np.inf]
    for i, r in enumerate(rows):
        (c.src if i % 2 else c.tgt)[r, i % 3] = vals[i % 3]
    if row0:
        c.src[0, 1] = np.nan
    return c


def tiny_beta(L, beta, seed=0):
    return band(L, beta, seed=seed + 60, name=f"tiny_beta_{beta:g}")


CASES = {
    "band_0.6": lambda L: band(L, 0.6),
    "band_0.0101": lambda L: band(L, 0.0101),
    "band_6": lambda L: band(L, 6.0),
    "exact_ties": exact_ties,
    "flat": flat,
    "short_tims": short_tims,
    "far_origin_250": lambda L: far_origin(L, 250),
    "far_origin_330": lambda L: far_origin(L, 330),
    "far_origin_2000": lambda L: far_origin(L, 2000),
    "map_frame": map_frame,
    "map_frame_wide": lambda L: map_frame(L, wide=True),
    "nonfinite": nonfinite,
    "nonfinite_row0": lambda L: nonfinite(L, row0=True),
    "tiny_beta_0.004": lambda L: tiny_beta(L, 0.004),
    "tiny_beta_0.01": lambda L: tiny_beta(L, 0.01),
}
BAND_CASES = ("band_0.6", "band_0.0101", "band_6")
_cache = {}


def case(name, L):
    """The case `name` at L correspondences (cached: the arrays are shared, leave them unchanged)."""
    if (name, L) not in _cache:
        c = CASES[name](L)
        c.src.setflags(write=False)
        c.tgt.setflags(write=False)
        _cache[(name, L)] = c
    return _cache[(name, L)]


def bits_of(bm, L):
    """bit matrix (L x words, uint64) -> L x L bool"""
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), axis=1, bitorder="little")[:, :L].astype(bool)


def pair_lengths(c):
    """a, b (L x L, binary64): TIM lengths as the reference forms them — points widened to double, norms as
    e0 + (e1 + e2), a correctly rounded square root"""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for cloud in (c.src, c.tgt):
            p = cloud[:, :3].astype(np.float64)
            d = [p[None, :, k] - p[:, None, k] for k in range(3)]
            out.append(np.sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])))
    return out


def restate_graph(c):
    """solveForScale in numpy binary64 over all pairs (L x L bool, diagonal clear): the two divisions, cwiseInverse"""
    beta = 2 * c.noise_bound * np.sqrt(c.cbar2)
    a, b = pair_lengths(c)
    with np.errstate(all="ignore"):
        fwd = np.abs(b / a - 1.0) <= beta * (1.0 / a)
        rev = np.abs(a / b - 1.0) <= beta * (1.0 / b)
    m = fwd & rev
    np.fill_diagonal(m, False)
    return m


def extreme_ratio_tims(beta, n=100000, seed=0):
    """(tims_src, tims_tgt): 3 x 2n binary64 TIMs for the stage entry points (qtr_scale_mask takes doubles; 6 doubles of
    scratch per TIM pair: 2n = 200000 fits the default handle's 72 max_corr) with one length
    tiny, 1e-12 .. 1e-3 m, and the other beta + tiny (1 + eps), eps = +-10^U(-12, -6), in random directions and in both
    roles: length ratios up to 1e13, where the reference expression's own rounding (~2^-52 a/b in a/b - 1) is far wider
    than a fixed relative band around (s + t - beta^2)^2 = 4 s t"""
    rng = np.random.default_rng([seed, 105, int(round(beta * 1e6))])
    b = 10.0 ** rng.uniform(-12.0, -3.0, n)
    a = beta + b * (1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12.0, -6.0, n))
    d1, d2 = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    d1[:, ::2], d2[:, ::2] = np.eye(3)[:, [0]], np.eye(3)[:, [1]]  # every other pair along an axis: lengths exact
    d1, d2 = d1 / np.sqrt((d1 * d1).sum(0)), d2 / np.sqrt((d2 * d2).sum(0))
    va, vb = a * d1, b * d2
    return np.concatenate([va, vb], axis=1), np.concatenate([vb, va], axis=1)


def restate_mask(tims_src, tims_tgt, beta):
    """solveForScale on given TIMs (3 x K binary64), in numpy binary64"""
    with np.errstate(all="ignore"):
        a = np.sqrt(tims_src[0] * tims_src[0] + (tims_src[1] * tims_src[1] + tims_src[2] * tims_src[2]))
        b = np.sqrt(tims_tgt[0] * tims_tgt[0] + (tims_tgt[1] * tims_tgt[1] + tims_tgt[2] * tims_tgt[2]))
        return (np.abs(b / a - 1.0) <= beta * (1.0 / a)) & (np.abs(a / b - 1.0) <= beta * (1.0 / b))
