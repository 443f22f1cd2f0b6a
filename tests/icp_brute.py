"""The exhaustive reference of the ICP correspondence search, and the cases the search tests share.

numpy only: no cell grid and nothing from include/qtr_icp_math.h.  The search it pins (quatro_amd/csrc/icp.hip, and the
hash grids of tests/icp_ref/icp_ref.cpp and tests/gicp_ref/gicp_ref.cpp) claims that the grid's shape never changes a
result; here there is no grid to have a shape.  The arithmetic is the documented one, binary64 + - * in the written
order, so the comparison is array equality and not a tolerance:

    q  = ((T0 x + T1 y) + T2 z) + T3                 per row of T, from the float32 source point
    d2 = (dx dx + dy dy) + dz dz,  d = q - t         against EVERY finite target point
    nearest = the lowest target index among those of minimal d2, kept when d2 <= max_d * max_d

then the drop rules of the methods (include/quatro_hip.h, include/qtr_icp_math.h): point-to-plane drops a correspondence
whose target normal is not finite; plane-to-plane skips a source whose normal is not finite or of zero length before the
search and drops a correspondence whose target normal is not finite or of zero length after it.

grid_of / query_cells mirror icp_grid_of and the query side of d_icp_iter.  They are used for PRECONDITIONS only (a case
asserts that it really is on the cell-enlargement path, really has one cell, really leaves the grid); no expected result
comes from them.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

CELL_CAP = 1 << 22     # QTR_ICP_CELL_CAP: the single-pair calls' largest cell table
BATCH_CELLS = 1 << 20  # QTR_ICP_BATCH_CELLS: the table every slot of a batch reserves
_CHUNK_ENTRIES = 1 << 20  # entries of one d2 block (8 threads x 3 float64 blocks of it: ~200 MB at the most)
_THREADS = max(1, min(8, os.cpu_count() or 1))


def f4(a):
    a = np.asarray(a, dtype=np.float32)
    if a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
    return np.ascontiguousarray(a)


def finite3(a4):
    return np.isfinite(np.asarray(a4)[:, :3]).all(axis=1)


def normal_ok(n4):
    n = np.asarray(n4)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return finite3(n4) & (((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) > 0.0)


def transform(src4, T):
    """q [ns, 3] in float64, ((T0 x + T1 y) + T2 z) + T3 per row."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(src4)[:, :3].astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def _block(q, t, stats):
    """rows of q against all of t: index of the first minimal d2, that d2, and (stats) how many targets share it."""
    d = q[:, 0:1] - t[None, :, 0]
    np.multiply(d, d, out=d)
    e = q[:, 1:2] - t[None, :, 1]
    np.multiply(e, e, out=e)
    np.add(d, e, out=d)
    np.subtract(q[:, 2:3], t[None, :, 2], out=e)
    np.multiply(e, e, out=e)
    np.add(d, e, out=d)
    j = d.argmin(axis=1)  # (the first of equal values: the lowest index)
    m = d[np.arange(d.shape[0]), j]
    ties = (d == m[:, None]).sum(axis=1) if stats else None
    return j, m, ties


def search(src4, tgt4, T, max_d, stats=False):
    """The search alone (no method's drop rule): int32[ns] target index or -1, float64[ns] d2 of it (inf: none) and, with
    stats, int[ns] the number of finite targets at exactly the minimal d2 (0: no target in reach)."""
    src4, tgt4 = f4(src4), f4(tgt4)
    ns = src4.shape[0]
    corr = np.full(ns, -1, np.int32)
    d2 = np.full(ns, np.inf)
    ties = np.zeros(ns, np.int64)
    keep = np.flatnonzero(finite3(tgt4))  # ascending: the first minimum among them is the lowest original index
    q = transform(src4, T)
    rows = np.flatnonzero(finite3(src4) & np.isfinite(q).all(axis=1))
    if keep.size and rows.size:
        t = tgt4[keep, :3].astype(np.float64)
        step = max(1, _CHUNK_ENTRIES // keep.size)
        parts = [rows[a:a + step] for a in range(0, rows.size, step)]
        with ThreadPoolExecutor(_THREADS) as ex:
            outs = list(ex.map(lambda r: _block(q[r], t, stats), parts))
        max_d2 = float(max_d) * float(max_d)
        for r, (j, m, k) in zip(parts, outs):
            ok = m <= max_d2  # (the minimum over all targets is in reach exactly when any target is)
            corr[r[ok]] = keep[j[ok]]
            d2[r[ok]] = m[ok]
            if stats:
                ties[r[ok]] = k[ok]
    return (corr, d2, ties) if stats else (corr, d2)


def drop(corr, method, tgt_nrm4=None, src_nrm4=None):
    """The method's own rules on the search's result."""
    out = np.array(corr, dtype=np.int32)
    has = out >= 0
    if method == 0:
        out[has] = np.where(finite3(tgt_nrm4)[out[has]], out[has], -1)
    elif method == 2:
        out[~normal_ok(src_nrm4)] = -1  # (skipped before the search: the same set as dropped after it)
        has = out >= 0
        out[has] = np.where(normal_ok(tgt_nrm4)[out[has]], out[has], -1)
    return out


def nearest(src4, tgt4, T, max_d, tgt_nrm4=None, src_nrm4=None, method=1):
    return drop(search(src4, tgt4, T, max_d)[0], method, tgt_nrm4, src_nrm4)


def mse_count(src4, tgt4, T, corr):
    """(count, mean d2 by math.fsum: the correctly rounded sum of the binary64 d2 values, then one division)."""
    corr = np.asarray(corr)
    has = np.flatnonzero(corr >= 0)
    if has.size == 0:
        return 0, float("nan")
    d = transform(f4(src4)[has], T) - f4(tgt4)[corr[has], :3].astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return int(has.size), math.fsum(d2.tolist()) / has.size


# ---- mirrors for preconditions only -------------------------------------------------------------------------------
def bbox_of(tgt4):
    t = f4(tgt4)
    t = t[finite3(t), :3].astype(np.float64)
    return t.min(axis=0), t.max(axis=0)


def grid_of(bbox_min, bbox_max, max_d, cap):
    """icp_grid_of: (cell side, dims, times the cell was enlarged)."""
    mn, mx = np.asarray(bbox_min, np.float64), np.asarray(bbox_max, np.float64)
    cell, grown = max_d * 1.001, 0
    while np.prod(np.floor((mx - mn) / cell) + 1.0) > cap:
        cell, grown = cell * 1.25, grown + 1
    return cell, tuple(int(v) for v in np.floor((mx - mn) / cell) + 1.0), grown


def query_cells(q, bbox_min, cell, dims):
    """The query side of d_icp_iter per point: (below [n,3]: f == -1, above [n,3]: f == dims, outside [n]: not any)."""
    with np.errstate(invalid="ignore"):
        f = np.floor((q - np.asarray(bbox_min, np.float64)) / cell)
        d = np.asarray(dims, np.float64)
        inside = (f >= -1.0) & (f <= d)
    return f == -1.0, f == d, ~inside.all(axis=1)


# ---- the cases --------------------------------------------------------------------------------------------------------
def rot(roll=0.0, pitch=0.0, yaw=0.0):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


SMALL = rigid(rot(0.012, -0.009, 0.015), [0.25, -0.3, 0.08])  # the perturbation of tests/test_gpu_icp.py


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return f4(v / np.linalg.norm(v, axis=1, keepdims=True))


class Case:
    """One input of the search: clouds, both normal sets, the guess, the distance, and its precondition (a callable that
    asserts on the reference's own figures and returns them as a dict, for the record)."""

    def __init__(self, name, src, tgt, guess, max_d, src_nrm=None, tgt_nrm=None, pre=None, seed=0):
        self.name = name
        self.src, self.tgt = f4(src), f4(tgt)
        self.src_nrm = f4(src_nrm) if src_nrm is not None else unit_normals(self.src.shape[0], seed + 1)
        self.tgt_nrm = f4(tgt_nrm) if tgt_nrm is not None else unit_normals(self.tgt.shape[0], seed + 2)
        self.guess = np.ascontiguousarray(guess, dtype=np.float64).reshape(4, 4)
        self.max_d = float(max_d)
        self.pre = pre

    def grid(self, cap=CELL_CAP):
        mn, mx = bbox_of(self.tgt)
        return (mn,) + grid_of(mn, mx, self.max_d, cap)

    def check_pre(self):
        return self.pre(self) if self.pre else {}


class VoxPair:
    """synth.kitti64_pair(2) voxelised at 0.3 m with both normal sets at 0.5 m and the perturbed guess.  `front` brings
    voxelize(points, leaf) and normals(points, radius): the oracle's on the CPU, the device's own in the GPU file."""

    def __init__(self, front):
        from quatro_amd import synth
        s, t, Tgt = synth.kitti64_pair(2)
        self.src, self.tgt = front.voxelize(s, 0.3), front.voxelize(t, 0.3)
        self.src_nrm, self.tgt_nrm = front.normals(self.src, 0.5), front.normals(self.tgt, 0.5)
        self.guess = Tgt @ SMALL

    def case(self, name, max_d, src=None, tgt=None, pre=None, guess=None):
        s = np.arange(self.src.shape[0]) if src is None else src
        t = np.arange(self.tgt.shape[0]) if tgt is None else tgt
        return Case(name, self.src[s], self.tgt[t], self.guess if guess is None else guess, max_d, self.src_nrm[s],
                    self.tgt_nrm[t], pre)


GRID_MAX_D = (0.02, 0.1, 0.3, 1.0, 7.0, 500.0)
SIZES_NS = (1, 63, 64, 255, 256, 257, 511, 513, 4097)
SIZES_NT = (1, 2, 300)
LATTICE_MAX_D = (0.5, 0.75, math.sqrt(3.0) / 2.0, 1.0)


def _pre_grid(c):
    _, cell22, dims22, g22 = c.grid(CELL_CAP)
    _, cell20, dims20, g20 = c.grid(BATCH_CELLS)
    out = {"cell_2^22": cell22, "dims_2^22": dims22, "enlarged_2^22": g22, "cell_2^20": cell20, "dims_2^20": dims20,
           "enlarged_2^20": g20}
    if c.max_d == 500.0:
        assert dims22 == (1, 1, 1), out
    return out


def grid_cases(vp):
    return [vp.case(f"grid_max_d_{d}", d, pre=_pre_grid) for d in GRID_MAX_D]


def check_grid_family(cases):
    """Across GRID_MAX_D: >= 2 distances enlarge the cell under 2^22, >= 1 more enlarges under 2^20 only."""
    pres = {c.max_d: c.check_pre() for c in cases}
    both = [d for d, p in pres.items() if p["enlarged_2^22"] > 0]
    only20 = [d for d, p in pres.items() if p["enlarged_2^22"] == 0 and p["enlarged_2^20"] > 0]
    assert len(both) >= 2 and len(only20) >= 1, pres
    return {"enlarge_under_2^22": both, "enlarge_under_2^20_only": only20}


def _pre_dims(pred):
    def pre(c):
        _, cell, dims, _ = c.grid()
        assert pred(dims), dims
        return {"dims": dims}
    return pre


def degenerate_cases(vp):
    rng = np.random.default_rng(21)
    flat = np.c_[rng.uniform(-20, 20, (4000, 2)), np.full(4000, 1.5)]
    fsrc = flat[rng.permutation(4000)[:3000]] + np.array([0.1, -0.05, 0.0])
    line = np.c_[np.linspace(-30, 30, 3000), np.zeros(3000), np.zeros(3000)]
    lsrc = line[::2] + np.array([0.013, 0.0, 0.0])
    one = np.array([[3.0, -2.0, 0.5]])
    osrc = one + rng.normal(0, 0.4, (700, 3))
    return [
        Case("flat_in_z", fsrc, flat, np.eye(4), 0.3, pre=_pre_dims(lambda d: d[2] == 1 and d[0] > 1 and d[1] > 1), seed=1),
        Case("flat_in_z_tilted_guess", fsrc, flat, SMALL, 0.3, pre=_pre_dims(lambda d: d[2] == 1), seed=2),
        Case("all_on_a_line", lsrc, line, np.eye(4), 0.05, pre=_pre_dims(lambda d: d[1] == 1 and d[2] == 1 and d[0] > 1),
             seed=3),
        Case("single_point_target", osrc, one, np.eye(4), 0.5, pre=_pre_dims(lambda d: d == (1, 1, 1)), seed=4),
    ]


def size_cases(vp):
    rng = np.random.default_rng(22)
    ns_all, nt_all = vp.src.shape[0], vp.tgt.shape[0]
    out = []
    for n in SIZES_NS:
        out.append(vp.case(f"ns_{n}", 1.0, src=np.sort(rng.choice(ns_all, n, replace=False))))
    near = search(vp.src, vp.tgt, vp.guess, 1.0)[0]
    near = np.unique(near[near >= 0])  # targets that are somebody's nearest: a tiny target still has correspondences
    for n in SIZES_NT:
        out.append(vp.case(f"nt_{n}", 1.0, tgt=np.sort(rng.choice(near, n, replace=False))))
    out.append(vp.case("ns_much_larger_than_nt", 0.5, tgt=np.sort(rng.choice(nt_all, 40, replace=False))))
    return out


def lattice():
    """12 x 12 x 6 integer lattice in permuted order with 100 points duplicated; sources at the face, edge and body
    midpoints of its cells (distances 0.5, sqrt(2)/2, sqrt(3)/2 to 2, 4, 8 targets: exact in binary64)."""
    rng = np.random.default_rng(23)
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), np.arange(6.0), indexing="ij"), -1).reshape(-1, 3)
    tgt = np.concatenate([g, g[rng.choice(g.shape[0], 100, replace=False)]])
    tgt = tgt[rng.permutation(tgt.shape[0])]
    src = []
    for off in ([0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0.5, 0.5]):
        p = g + np.array(off)
        src.append(p[(p <= np.array([11.0, 11.0, 5.0])).all(axis=1)])
    src = np.concatenate(src)
    return src[rng.permutation(src.shape[0])], tgt


def _pre_lattice(c):
    _, d2, ties = search(c.src, c.tgt, c.guess, c.max_d, stats=True)
    out = {"sources": int(c.src.shape[0]), "tied_at_the_minimum": int((ties >= 2).sum()),
           "exactly_at_max_d": int((d2 == c.max_d * c.max_d).sum())}
    assert out["tied_at_the_minimum"] >= 1000, out
    if c.max_d == 0.5:
        assert out["exactly_at_max_d"] >= 1000, out
    return out


def lattice_cases(vp=None):
    src, tgt = lattice()
    return [Case(f"lattice_max_d_{d:.4f}", src, tgt, np.eye(4), d, pre=_pre_lattice, seed=5) for d in LATTICE_MAX_D]


def _pre_outside(c):
    mn, cell, dims, _ = c.grid()
    below, above, outside = query_cells(transform(c.src, c.guess), mn, cell, dims)
    out = {"f_is_-1": int(below.any(axis=1).sum()), "f_is_dims": int(above.any(axis=1).sum()),
           "outside_the_27_cells": int(outside.sum())}
    assert below.any(axis=0).all() and above.any(axis=0).all() and outside.any(), out  # (each branch, in every axis)
    corr = search(c.src, c.tgt, c.guess, c.max_d)[0]
    out["correspondences_from_f_-1_or_dims"] = int((corr[(below | above).any(axis=1) & ~outside] >= 0).sum())
    assert out["correspondences_from_f_-1_or_dims"] > 0, out
    return out


def outside_cases(vp):
    """Sources beyond each face of the target's box by 0.5, 0.999 and 1.5 max_d (opposite a target point on that face
    and spread over the face), at the box's corners, and kilometres off; identity guess."""
    out = []
    for max_d in (0.3, 1.0):
        mn, mx = bbox_of(vp.tgt)
        t = vp.tgt[:, :3].astype(np.float64)
        rng = np.random.default_rng(24)
        pts = []
        for a in range(3):
            for side, wall in ((-1.0, mn[a]), (1.0, mx[a])):
                on = t[t[:, a] == wall]  # the target points that make this face of the box
                for k in (0.5, 0.999, 1.5):
                    p = np.repeat(on, 8, axis=0)
                    p[:, a] = wall + side * k * max_d
                    pts.append(p)
                    p = rng.uniform(mn, mx, (300, 3))
                    p[:, a] = wall + side * k * max_d
                    pts.append(p)
        corners = np.array([[x, y, z] for x in (mn[0], mx[0]) for y in (mn[1], mx[1]) for z in (mn[2], mx[2])])
        pts += [corners, corners + 0.4 * max_d * np.sign(corners - (mn + mx) / 2)]
        pts.append(rng.uniform(-1, 1, (200, 3)) * 50 + np.array([3000.0, -2000.0, 40.0]))
        pts.append(rng.uniform(-1, 1, (200, 3)) * 50 - np.array([7000.0, 0.0, 9000.0]))
        pts.append(vp.src[::40, :3].astype(np.float64))  # and ordinary points inside
        src = np.concatenate(pts)
        out.append(Case(f"outside_the_grid_max_d_{max_d}", src, vp.tgt, np.eye(4), max_d, tgt_nrm=vp.tgt_nrm,
                        pre=_pre_outside, seed=6))
    return out


def _pre_some(c):
    n = int((search(c.src, c.tgt, c.guess, c.max_d)[0] >= 0).sum())
    assert n >= 100, n
    return {"correspondences": n}


def coordinate_cases(vp):
    off = np.array([4.5e5, 5.2e6, 300.0])  # (UTM-sized: float32 keeps 0.5 m steps in y there)
    To = rigid(np.eye(3), off)
    s_off, t_off = vp.src.copy(), vp.tgt.copy()
    s_off[:, :3] = (vp.src[:, :3].astype(np.float64) + off).astype(np.float32)
    t_off[:, :3] = (vp.tgt[:, :3].astype(np.float64) + off).astype(np.float32)
    g_off = To @ vp.guess @ np.linalg.inv(To)
    neg = np.array([-500.0, -300.0, -60.0])
    Tn = rigid(np.eye(3), neg)
    s_neg, t_neg = vp.src.copy(), vp.tgt.copy()
    s_neg[:, :3] += neg.astype(np.float32)
    t_neg[:, :3] += neg.astype(np.float32)
    assert (t_neg[:, :3] < 0).all() and (s_neg[:, :3] < 0).all()
    rng = np.random.default_rng(25)
    z = np.round(rng.uniform(-3, 3, (6000, 3)) * 2) / 2  # half-metre lattice values: many exact zeros
    z = z.astype(np.float32)
    z[(z == 0) & (rng.random(z.shape) < 0.5)] = -0.0
    zs = z[rng.permutation(6000)[:3000]].copy()
    zs[:, :3] += np.float32(0.25) * (rng.integers(0, 2, (3000, 3)) * 2 - 1).astype(np.float32) * (rng.random((3000, 3)) < 0.5)
    zs[(zs == 0) & (rng.random(zs.shape) < 0.5)] = -0.0

    def pre_zero(c):
        out = _pre_some(c)
        out["negative_zeros"] = int((np.signbit(c.tgt[:, :3]) & (c.tgt[:, :3] == 0)).sum())
        out["positive_zeros"] = int((~np.signbit(c.tgt[:, :3]) & (c.tgt[:, :3] == 0)).sum())
        assert out["negative_zeros"] > 100 and out["positive_zeros"] > 100, out
        return out
    return [
        Case("offset_4.5e5_5.2e6_300", s_off, t_off, g_off, 1.0, vp.src_nrm, vp.tgt_nrm, pre=_pre_some),
        Case("offset_4.5e5_5.2e6_300_small_cells", s_off, t_off, g_off, 0.1, vp.src_nrm, vp.tgt_nrm, pre=_pre_some),
        Case("all_negative_octant", s_neg, t_neg, Tn @ vp.guess @ np.linalg.inv(Tn), 1.0, vp.src_nrm, vp.tgt_nrm,
             pre=_pre_some),
        Case("signed_zeros", zs, z, np.eye(4), 0.5, pre=pre_zero, seed=7),
    ]


def nonfinite_cases(vp):
    rng = np.random.default_rng(26)
    s, t, sn, tn = vp.src.copy(), vp.tgt.copy(), vp.src_nrm.copy(), vp.tgt_nrm.copy()
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for a, frac in ((s, 0.02), (t, 0.02), (sn, 0.03), (tn, 0.03)):
        rows = rng.choice(a.shape[0], int(a.shape[0] * frac), replace=False)
        a[rows, rng.integers(0, 3, rows.size)] = bad[rng.integers(0, 3, rows.size)]
    sn[rng.choice(sn.shape[0], 200, replace=False), :3] = 0.0  # zero-length normals: plane-to-plane's other rule
    tn[rng.choice(tn.shape[0], 200, replace=False), :3] = 0.0

    def pre(c):
        raw = search(c.src, c.tgt, c.guess, c.max_d)[0]
        out = {f"dropped_by_method_{m}": int((raw >= 0).sum() - (drop(raw, m, c.tgt_nrm, c.src_nrm) >= 0).sum())
               for m in (0, 2)}
        out["sources_not_finite"] = int((~finite3(c.src)).sum())
        out["targets_not_finite"] = int((~finite3(c.tgt)).sum())
        assert min(out.values()) >= 50, out
        return out
    t_nan = vp.tgt.copy()
    t_nan[:, :3] = np.nan
    t_nan[::3, 1] = np.inf
    return [Case("non_finite_scattered", s, t, vp.guess, 1.0, sn, tn, pre=pre),
            Case("target_all_non_finite", vp.src, t_nan, vp.guess, 1.0, vp.src_nrm, vp.tgt_nrm)]


FAMILIES = {"grid": grid_cases, "degenerate": degenerate_cases, "sizes": size_cases, "lattice": lattice_cases,
            "outside": outside_cases, "coordinates": coordinate_cases, "non_finite": nonfinite_cases}


def all_cases(vp):
    return [c for make in FAMILIES.values() for c in make(vp)]


# ---- the box scene of the fuzz (tests/gpu_fuzz.py) and of the CPU file -----------------------------------------------------
BOX_SIZES = ((1, 1, 1.0), (255, 4000, 0.05), (257, 4000, 0.3), (4000, 4000, 1.0), (5100, 300, 7.0), (3000, 5100, 0.02))


def box_pair(ns, nt, seed):
    """ns source and nt target points drawn from the box scene of icp_restate.box_scene (exact normals), the source a
    slightly moved copy; returns src, src_nrm, tgt, tgt_nrm, guess."""
    import icp_restate as R
    rng = np.random.default_rng(seed)
    pts, nrm = R.box_scene(seed=seed % 7)
    i, j = rng.integers(0, pts.shape[0], ns), rng.integers(0, pts.shape[0], nt)
    Tt = rigid(rot(0.02, -0.01, 0.03), [0.15, -0.1, 0.05])
    tgt, tn = R.apply(Tt, pts[j]), nrm[j].copy()
    tn[:, :3] = nrm[j, :3] @ Tt[:3, :3].T
    src = pts[i].copy()
    src[:, :3] += rng.normal(0, 0.01, (ns, 3)).astype(np.float32)
    return src, nrm[i].copy(), tgt, tn, Tt @ SMALL
