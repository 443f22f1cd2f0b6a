"""No-GPU checks of tests/front_cases.py, the inputs of tests/test_gpu_front_cases.py:

  * the cases stay what they claim: every entry of a case's `claims` is asserted here, on the oracle's output where the
    branch shows there (NaN patterns, signed zeros, SPFH blocks below 100, all-zero rows, list lengths, counts of ties and
    of d2 == r2) and on a binary32 numpy mirror of the branch predicate where it does not (the cell arithmetic of the
    neighbour grid, the c0 == 0 test of the eigenvalue solver, cos_theta == 0): a case that is not on its branch fails
    here, not silently on the GPU;
  * the oracle deserves to be the yardstick on these clouds: its neighbour lists equal a brute force exactly, its voxel
    grid equals a numpy restatement, its normals agree with numpy.linalg.eigh in binary64 wherever the two smallest
    eigenvalues are separated; where a neighbourhood is degenerate there is no independent answer and the oracle's
    pattern is what the claims record;
  * the mirrored constants equal the sources'.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_cases as fc  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
FLT_EPSILON, FLT_MIN = f32(1.1920928955078125e-07), f32(1.17549435e-38)
_outs = {}


def _out(qo, name):
    """the oracle's and the brute force's answers on a case, computed once"""
    if name not in _outs:
        c = fc.case(name)
        off, idx, d2 = qo.radius_neighbors(c.cloud, c.r_fpfh)
        nrm, sp, de = qo.fpfh(c.cloud, c.r_normal, c.r_fpfh)
        _outs[name] = dict(off=off, idx=idx, d2=d2, nrm=nrm, sp=sp, de=de, brute=fc.brute_neighbors(c.cloud, c.r_fpfh))
    return _outs[name]


def _b(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _rows_are(nrm, row):
    return bool(np.all(_b(nrm) == _b(np.array(row, dtype=f32))[None, :]))


def _nan3_curv0(nrm):
    return bool(np.isnan(nrm[:, :3]).all() and np.all(_b(nrm[:, 3]) == 0))


def _blocks(sp):
    return sp.reshape(-1, 3, 11).astype(np.float64).sum(2)


def _k_normal(c, o):
    rn2 = f32(c.r_normal * c.r_normal)
    return np.array([(o["d2"][o["off"][i]:o["off"][i + 1]] < rn2).sum() for i in range(c.cloud.shape[0])])


# ---------------------------------------------------------------------------------------------- constants
def test_mirrored_constants_equal_the_sources():
    hdr = open(os.path.join(ROOT, "quatro_amd", "csrc", "frontend.h")).read()
    src = open(os.path.join(ROOT, "quatro_amd", "csrc", "frontend.hip")).read()
    capi = open(os.path.join(ROOT, "quatro_amd", "csrc", "capi.hip")).read()
    orc = open(os.path.join(ROOT, "oracle", "quatro_oracle.cpp")).read()

    def define(text, name):
        m = re.search(r"^#define %s (\(?[0-9 <]+\)?)" % name, text, flags=re.M)
        assert m, "the #define %s line changed its form" % name
        return eval(m.group(1))  # digits, blanks, shifts and brackets only

    assert define(hdr, "QTR_KMAX") == fc.QTR_KMAX
    assert define(hdr, "QTR_CELL_CAP") == fc.QTR_CELL_CAP
    assert define(src, "FPFH_CHUNK") == fc.FPFH_CHUNK
    assert define(src, "FPFH_PB") == fc.FPFH_PB
    assert define(src, "SPFH_PB") == fc.SPFH_PB
    # the cell side of the neighbour grid, wherever it is formed: the FPFH chain, the voxel stage's cell count (twice), the oracle
    assert float(fc.CELL_MARGIN) == float(f32(1.001))
    assert len(re.findall(r"const float cell = r_fpfh \* 1\.001f;", src)) == 1
    assert len(re.findall(r"fpfh_radius \* 1\.001f\)", capi)) == 2
    assert len(re.findall(r"const float cell = \(float\)radius \* 1\.001f;", orc)) == 1
    assert len(re.findall(r"min\(%d, max\(0, \(int\)floorf\(" % fc.CELL_CLAMP, src)) == 3  # cell_of, one line per axis
    # the switches of k2_neighbors and k2_fpfh that the ball_<m> cases straddle
    assert "if (k <= %d) {" % fc.RANK_SORT_MAX in src and "int n2 = %d;  //" % fc.BITONIC_MIN in src
    assert "int cnt_bits = 12;" in src and 11 * fc.CNT_BITS_SWITCH < 4096 <= 11 * (fc.CNT_BITS_SWITCH + 1)
    for edge in (fc.RANK_SORT_MAX, fc.BITONIC_MIN, fc.QTR_KMAX, fc.CNT_BITS_SWITCH):
        assert edge in fc.BALL_M and edge + 1 in fc.BALL_M
    assert any(m % fc.FPFH_CHUNK == 0 for m in fc.BALL_M) and any(m % fc.FPFH_CHUNK == fc.FPFH_CHUNK - 1 for m in fc.BALL_M)


def test_generators_are_deterministic_and_read_only():
    for name in ("ball_129", "straddle_0.3", "wide_extent"):
        a = fc.case(name)
        assert np.array_equal(_b(a.cloud), _b(fc._make(name).cloud)) and not a.cloud.flags.writeable
    for name in fc.NAMES:
        c = fc.case(name)
        assert c.cloud.shape[0] <= 700 and c.cloud.shape[1] == 4 and c.cloud.dtype == f32 and not c.cloud[:, 3].any()
        assert f32(c.r_normal) == c.r_normal and f32(c.r_fpfh) == c.r_fpfh and c.r_normal <= c.r_fpfh


# ---------------------------------------------------------------------------------------------- the oracle as yardstick
@pytest.mark.parametrize("name", fc.NAMES)
def test_oracle_lists_equal_the_brute_force(qo, name):
    o = _out(qo, name)
    boff, bidx, bd2 = o["brute"]
    assert np.array_equal(o["off"], boff) and np.array_equal(o["idx"], bidx)
    assert np.array_equal(_b(o["d2"]), _b(bd2))


def _eigh_normals(c, o):
    """per point with at least three neighbours inside r_normal: (smallest eigenvector of the binary64 covariance, whether
    it can judge).  It can where the angle the binary32 single-pass covariance may turn it by, err / gap to first order,
    stays below 1e-3 rad — under the 1.4e-3 rad that dot > 1 - 1e-6 allows: gap the distance of the two smallest
    eigenvalues, err = (8 + k) 2^-24 max |p|^2 (nine sums of k terms and six products of means, each rounded to binary32
    at the magnitude of |p|^2)."""
    P = c.cloud[:, :3].astype(np.float64)
    rn2 = f32(c.r_normal * c.r_normal)
    out = {}
    for i in range(P.shape[0]):
        s, e = o["off"][i], o["off"][i + 1]
        nb = o["idx"][s:e][o["d2"][s:e] < rn2]
        if nb.size < 3:
            continue
        Q = P[nb]
        m = Q.mean(0)
        w, V = np.linalg.eigh((Q[:, :, None] * Q[:, None, :]).mean(0) - np.outer(m, m))
        err = (8 + nb.size) * 2.0 ** -24 * (Q ** 2).sum(1).max()
        out[i] = (V[:, 0], (w[1] - w[0]) * 1e-3 > err)
    return out


NOT_DEGENERATE = tuple(n for n in fc.NAMES if n not in fc.DEGENERATE)
JUDGED = {}


@pytest.mark.parametrize("name", NOT_DEGENERATE)
def test_oracle_normals_against_eigh_in_binary64(qo, name):
    c, o = fc.case(name), _out(qo, name)
    ref = _eigh_normals(c, o)
    kn = _k_normal(c, o)
    assert np.array_equal(np.isnan(o["nrm"]).all(1), kn < 3)  # four NaNs exactly where fewer than three points are in reach
    judged = 0
    for i, (v, can) in ref.items():
        if not can:
            continue
        n = o["nrm"][i, :3].astype(np.float64)
        assert abs(np.dot(n, v)) > 1 - 1e-6, (name, i)
        assert np.dot(n, -c.cloud[i, :3].astype(np.float64)) >= -1e-5  # turned to the viewpoint, the origin
        judged += 1
    JUDGED[name] = judged
    if not name.startswith("ball_"):  # (inside a ball the two smallest eigenvalues are close: few points can be judged)
        assert judged >= 3, (name, judged)


def test_voxel_grid_against_the_numpy_restatement(qo):
    c = fc.case("voxel_borders")
    leaf = c.claims["leaf"]
    out = qo.voxelize(c.cloud, leaf)
    exp = fc.voxelize_numpy(c.cloud, leaf)
    assert out.shape[0] == exp.shape[0] == c.claims["n_voxels"]
    assert np.array_equal(_b(out[:, :3]), _b(exp)) and not out[:, 3].any()
    # what the case is there for: every second point lies exactly on a voxel border, the one before it an ulp below it in
    # every coordinate — in the voxel below; and the lattice spans both signs
    on, below = c.cloud[0::2, :3], c.cloud[1::2, :3]
    q = on.astype(np.float64) / leaf
    assert np.array_equal(q, np.round(q)) and q.min() < 0 < q.max()
    inv = f32(1.0) / f32(leaf)
    assert np.array_equal(np.floor(below * inv), np.floor(on * inv) - 1)


@pytest.mark.parametrize("name", fc.FPFH_NAMES)
def test_keyframe_leaf_leaves_every_point_a_voxel_of_its_own(qo, name):
    """the keyframe route voxelises first: at keyframe_leaf(name) the oracle's voxel grid returns the cloud's own points,
    in voxel order or — a grid beyond int32 — as they came"""
    c = fc.case(name)
    v = qo.voxelize(c.cloud, fc.keyframe_leaf(name))
    assert v.shape == c.cloud.shape
    key = lambda a: a[np.lexsort((_b(a[:, 2]), _b(a[:, 1]), _b(a[:, 0])))]
    assert np.array_equal(_b(key(v)), _b(key(c.cloud)))


# ---------------------------------------------------------------------------------------------- straddle
@pytest.mark.parametrize("r", fc.STRADDLE_R)
def test_straddle_pairs_need_the_margin_of_the_cell_side(qo, r):
    name = f"straddle_{r}"
    c, o = fc.case(name), _out(qo, name)
    cl, x = c.claims, c.cloud[:, 0]
    rf = f32(r)
    assert c.r_fpfh == float(rf)
    if r == 0.75:
        assert cl["n_kept"] == cl["n_kept_found"] == 0  # exact radius, exact quotients: the control
    else:
        assert cl["n_kept"] >= 32
    assert len(cl["pairs"]) >= cl["n_kept"] + 32  # (the control pairs next to the margined grid's borders)
    mn = c.cloud[:, 0].min()
    assert mn == fc.STRADDLE_MN == x[0] and float(mn) != round(float(mn), 3)  # the anchor pins the box minimum
    boff, bidx, _ = o["brute"]
    for off, idx in ((boff, bidx), (o["off"], o["idx"])):  # the brute force, then the oracle
        for a in cl["pairs"]:
            assert sorted(idx[off[a]:off[a + 1]]) == [a, a + 1] and sorted(idx[off[a + 1]:off[a + 2]]) == [a, a + 1]
        assert off[1] == 1  # the anchor is alone
    # the un-margined grid puts the kept pairs two cells apart: a 3 x 3 x 3 scan from either point never sees the other;
    # the margined grid puts every pair within one cell — the simulation of cell_of in binary32
    a = cl["kept"]
    assert np.all(np.abs(fc.cells_of(x[a + 1], mn, rf) - fc.cells_of(x[a], mn, rf)) == 2)
    p = cl["pairs"]
    cell = rf * fc.CELL_MARGIN
    assert np.all(np.abs(fc.cells_of(x[p + 1], mn, cell) - fc.cells_of(x[p], mn, cell)) <= 1)
    # each pair on a row of its own, at least 3 r from every other point
    yz = c.cloud[p, 1:3].astype(np.float64)
    assert np.array_equal(yz, c.cloud[p + 1, 1:3]) and len({tuple(v) for v in yz}) == len(p)
    assert cl["row_step"] >= 3 * r and np.all(np.mod(yz, cl["row_step"]) == 0)
    dims, raw = fc.grid_cells(c.cloud, c.r_fpfh)
    assert np.array_equal(dims, raw) and dims.prod() <= fc.QTR_CELL_CAP  # no clamp; the keyframe route takes the dense table


# ---------------------------------------------------------------------------------------------- claims
def _c0_mirror(c, o, i):
    """binary32 mirror of k2_normals up to the branch of pcl's eigenvalue solver: the nine single-pass sums in list order,
    the covariance, its scaling, c0 in the source's order of operations"""
    rn2 = f32(c.r_normal * c.r_normal)
    s, e = o["off"][i], o["off"][i + 1]
    nb = o["idx"][s:e][o["d2"][s:e] < rn2]
    acc = [f32(0)] * 9
    for j in nb:
        x, y, z = c.cloud[j, :3]
        for t, v in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
            acc[t] = acc[t] + v
    acc = [a / f32(nb.size) for a in acc]
    cov = {0: acc[0] - acc[6] * acc[6], 1: acc[1] - acc[6] * acc[7], 2: acc[2] - acc[6] * acc[8],
           4: acc[3] - acc[7] * acc[7], 5: acc[4] - acc[7] * acc[8], 8: acc[5] - acc[8] * acc[8]}
    scale = max(abs(v) for v in cov.values())
    if scale <= FLT_MIN:
        scale = f32(1)
    m = {k: v / scale for k, v in cov.items()}
    two = f32(2)
    c0 = m[0] * m[4] * m[8] + two * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] - m[8] * m[1] * m[1]
    assert type(c0) is f32
    return c0, scale, cov[0] + cov[4] + cov[8]


def _list_pairs_with(o, pred):
    """number of list entries (i, j), j != i, whose d2 satisfies pred"""
    owner = np.repeat(np.arange(o["off"].size - 1), np.diff(o["off"]))
    return int((pred(o["d2"]) & (o["idx"] != owner)).sum())


@pytest.mark.parametrize("name", fc.FPFH_NAMES)
def test_case_is_on_the_branch_it_claims(qo, name):
    c, o = fc.case(name), _out(qo, name)
    cl, n = c.claims, c.cloud.shape[0]
    nrm, sp, de, k = o["nrm"], o["sp"], o["de"], np.diff(o["off"])
    rn2, r2 = f32(c.r_normal * c.r_normal), f32(c.r_fpfh * c.r_fpfh)
    checked = set()

    def claim(key):
        checked.add(key)
        return cl.get(key)

    if name.startswith("straddle_"):
        checked.update(cl)  # (test_straddle_pairs_need_the_margin_of_the_cell_side)
    if claim("d2_equal_rn2"):
        assert _list_pairs_with(o, lambda d: d == rn2) > 0  # in the lists, and cut from the normals by the strict <
    if claim("d2_equal_r2"):
        p = c.cloud[:, :3].astype(np.float64)
        exact = ((p[:, None] - p[None]) ** 2).sum(2)  # (lattice coordinates: exact in binary64)
        assert (exact == float(r2)).sum() > 0 and _list_pairs_with(o, lambda d: d >= r2) == 0
    if claim("d2_ties"):
        owner = np.repeat(np.arange(n), k)
        tie = (o["d2"][1:] == o["d2"][:-1]) & (owner[1:] == owner[:-1])
        assert tie.sum() >= cl["d2_ties"] and np.all(o["idx"][1:][tie] > o["idx"][:-1][tie])
    if claim("nan_normal_finite_curv"):
        assert (np.isnan(nrm[:, :3]).all(1) & np.isfinite(nrm[:, 3])).sum() >= cl["nan_normal_finite_curv"]
    if claim("negative_coordinates"):
        assert (c.cloud[:, :3].min(0) < 0).all() and (c.cloud[:, :3].max(0) > 0).all()
    if claim("list_length"):
        assert np.all(k == cl["list_length"]) and n == cl["list_length"]
    if claim("is_ball") is not None:
        ball = cl["is_ball"]
        checked.update(("long_length", "short_max"))
        assert np.all(k[ball] == cl["long_length"]) and cl["long_length"] > fc.QTR_KMAX
        assert np.all(k[~ball] <= cl["short_max"]) and np.all(k[~ball] >= 2)
        for pb in (fc.SPFH_PB, fc.FPFH_PB):  # long (pending) and short lists inside one workgroup's block of points
            mixed = [ball[b:b + pb].any() and not ball[b:b + pb].all() for b in range(0, n, pb)]
            assert sum(mixed) >= len(mixed) // 2
    if claim("k_fpfh"):
        checked.add("k_normal")
        kn = _k_normal(c, o)
        assert list(k) == cl["k_fpfh"] and list(kn) == cl["k_normal"]
        assert np.array_equal(np.isnan(nrm).all(1), kn < 3) and np.isfinite(nrm[kn >= 3]).all()
        assert not sp[0].any() and not de[0].any()  # k = 1: hist_incr = 100 / 0 and nothing to add it to
        assert np.isfinite(sp).all() and np.isfinite(de).all()
    if claim("route"):
        checked.add("clamped_points")
        dims, raw = fc.grid_cells(c.cloud, c.r_fpfh)
        assert raw[0] > fc.CELL_CLAMP + 1 == dims[0] and dims.prod() <= fc.QTR_CELL_CAP and cl["route"] == "dense"
        cx = fc.cells_of(c.cloud[:, 0], c.cloud[:, 0].min(), f32(c.r_fpfh) * fc.CELL_MARGIN)
        assert (cx > fc.CELL_CLAMP).sum() >= cl["clamped_points"]
        owner = np.repeat(np.arange(n), k)
        a, b = cx[owner], cx[o["idx"]]
        for lo in (fc.CELL_CLAMP - 1, fc.CELL_CLAMP):  # neighbours on either side of the last border kept and of the first one dropped
            assert ((a == lo) & (b == lo + 1)).sum() > 0
    if claim("quadratic_branch"):
        for i in range(n):
            c0, scale, _ = _c0_mirror(c, o, i)
            assert abs(c0) < FLT_EPSILON and scale > FLT_MIN
    if claim("normal_bits"):
        assert _rows_are(nrm, cl["normal_bits"])
    if claim("cos_theta_zero"):
        checked.add("origin_index")
        assert not c.cloud[cl["origin_index"]].any()
        p, v = c.cloud[:, :3], nrm[:, :3]
        w = f32(0) - p
        assert np.all(w[:, 0] * v[:, 0] + w[:, 1] * v[:, 1] + w[:, 2] * v[:, 2] == 0)  # +-0: not < 0, no flip
        assert _rows_are(nrm, (0.0, 0.0, 1.0, 0.0))  # the eigenvector as the cross product left it
    if claim("pattern"):
        assert cl["pattern"] == "nan3_curv0" and _nan3_curv0(nrm)
        for i in range(n):
            c0, scale, eig_sum = _c0_mirror(c, o, i)
            if name == "identical":
                assert scale == 1 and eig_sum == 0  # scale <= FLT_MIN, and the curvature's guard
    if claim("finite_normals"):
        assert np.isfinite(nrm).all(1).sum() >= cl["finite_normals"]
    if claim("zero_rows"):
        assert not sp.any() and not de.any()
    if claim("zero_d2_pairs"):
        assert _list_pairs_with(o, lambda d: d == 0) == cl["zero_d2_pairs"]
    if claim("blocks_below_100"):
        assert np.all(_blocks(sp)[k > 1] < 99.0)  # pairs skipped (coincident points, v_norm == 0) leave their mass out
    if claim("curvature_third"):
        assert np.all(np.abs(nrm[:, 3].astype(np.float64) - 1.0 / 3) < 1e-6)
        for i in range(n):
            assert abs(_c0_mirror(c, o, i)[0]) >= FLT_EPSILON  # the cubic branch
    if claim("nan_normals"):
        plain = _out(qo, "plane_lattice")["nrm"]
        assert np.isnan(nrm[:, :3]).all(1).sum() >= cl["nan_normals"] and not np.isnan(plain).any()
        assert np.array_equal(k, np.diff(_out(qo, "plane_lattice")["off"]))  # the same lattice, moved
    if claim("opposite_normals"):
        assert _rows_are(nrm[:64], (-0.0, -0.0, -1.0, 0.0)) and _rows_are(nrm[64:], (0.0, 0.0, 1.0, 0.0))
    if claim("other_layer_at_rn"):
        owner = np.repeat(np.arange(n), k)
        across = c.cloud[owner, 2] != c.cloud[o["idx"], 2]
        assert (across & (o["d2"] == rn2)).sum() == n and not (across & (o["d2"] < rn2)).any()
    if claim("denormal_d2"):
        assert _list_pairs_with(o, lambda d: (d > 0) & (d < FLT_MIN)) >= 2
    if claim("nan_descriptors"):
        assert np.isnan(de).any(1).sum() >= cl["nan_descriptors"] and np.isfinite(sp).all()
    assert checked >= set(cl), set(cl) - checked
