"""The voxel map's contract (include/qtr_vmap_math.h) on the host: the restatement of the device map
(tests/vmap_ref/vmap_ref.cpp, compiled by g++ from the shared header) against an independent numpy implementation, the grid
rule, the fold order, the member filter, the capacity refusal, and — before any GPU run — the equality with method 3's
restatement on the inputs tests/test_gpu_vmap.py uses."""
import math

import numpy as np
import pytest

import icp_restate as R
import vgicp_restate as V
import vmap_cases as K
import vmap_restate as M


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_map(a, b):
    fa, fb = a.fetch_all(), b.fetch_all()
    assert np.array_equal(fa[M.COORDS], fb[M.COORDS]) and np.array_equal(fa[M.COUNT], fb[M.COUNT])
    assert np.array_equal(_bits(fa[M.SUMS]), _bits(fb[M.SUMS])) and np.array_equal(_bits(fa[M.RECORDS]), _bits(fb[M.RECORDS]))
    assert np.array_equal(fa[M.CLOUD].view(np.uint32), fb[M.CLOUD].view(np.uint32))


def _scene(side):
    """The box scene of the ICP tests under a pose, moved off the voxel faces: no world coordinate within 1e-9 sides of one."""
    pts, nrm = R.box_scene(300, seed=4)
    pose = R.rigid(R.rot(0.02, -0.03, 0.4), [0.377, -1.291, 0.613])
    X = pts[:, :3].astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    f = X / side
    assert np.abs(f - np.round(f)).min() > 1e-9
    return pts, nrm, pose


def test_restatement_agrees_with_an_independent_numpy_implementation():
    """Records and every iteration of a 12-iteration registration.  Measured here (binary64, different association orders
    and np.linalg.inv against the adjugate): records 2.90e-16 at worst, transforms 1.11e-15 at worst over the twelve
    iterations; the assertions are ten times those."""
    side = 0.8
    pts, nrm, pose = _scene(side)
    half = pts.shape[0] // 2
    ref, npm = M.RefMap(side, 1 << 16), K.NumpyMap(side)
    for m in (ref, npm):
        m.insert(pts[:half], nrm[:half], pose)
        m.insert(pts[half:], nrm[half:], pose)
    f = ref.fetch_all()
    coords, n, mu, Cb = npm.records()
    assert np.array_equal(f[M.COORDS], coords) and np.array_equal(f[M.COUNT], n.astype(np.int32))
    C6 = np.stack([Cb[:, 0, 0], Cb[:, 0, 1], Cb[:, 0, 2], Cb[:, 1, 1], Cb[:, 1, 2], Cb[:, 2, 2]], axis=1)
    rec_err = max(np.abs(f[M.RECORDS][:, :3] - mu).max() / np.abs(mu).max(), np.abs(f[M.RECORDS][:, 3:] - C6).max())
    # the source: a sample of the scene seen from a perturbed frame; no q lands within 1e-9 sides of a face at any iteration
    rng = np.random.default_rng(9)
    sel = rng.choice(pts.shape[0], 1500, replace=False)
    src, sn = pts[sel].copy(), R.f4(nrm[sel, :3] + rng.normal(scale=0.05, size=(1500, 3)))
    src[:, :3] += rng.normal(scale=0.03, size=(1500, 3)).astype(np.float32)
    guess = pose @ R.rigid(R.rot(0.05, -0.04, 0.07), [0.55, -0.45, 0.3])
    got = ref.register(src, sn, guess, teps=0.0, feps=0.0, max_iter=12)
    want = npm.register(src, sn, guess, 12)
    assert got["iterations"] == 12
    errs = []
    for k in range(12):
        Tk = got["trace"][k, :16].reshape(4, 4)
        q = src[:, :3].astype(np.float64) @ Tk[:3, :3].T + Tk[:3, 3]
        assert np.abs(q / side - np.round(q / side)).min() > 1e-9
        errs.append(np.abs(Tk - want[k]).max())
    print(f"restatement vs numpy: records {rec_err:.2e}, transforms {max(errs):.2e} (per iteration {['%.1e' % e for e in errs]})")
    assert rec_err <= 2.9e-15
    assert max(errs) <= 1.11e-14
    assert R.rot_err_deg(got["T"], pose) < R.rot_err_deg(guess, pose)


def test_grid_rule():
    for c in (1.0, 0.5, 0.3):
        for k in (0, 1, 7, -1, -5, 1000, -1000):
            assert M.coord(k * c, c) == math.floor((k * c) / c)
        assert M.coord(3 * 0.5, 0.5) == 3 and M.coord(-3 * 0.5, 0.5) == -3  # exactly k c -> voxel k
        assert M.coord(-0.0, c) == 0 and M.coord(0.0, c) == 0
        assert M.coord(-1e-12, c) == -1 and M.coord(-0.25 * c, c) == -1 and M.coord(-1.25 * c, c) == -2
        for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300, 1e30):
            assert M.coord(bad, c) is None
    # the six ends of the grid at side 0.5 (2^20 / 2 is exact): the lowest face belongs, the highest does not
    lo, hi = -(1 << 20) * 0.5, (1 << 20) * 0.5
    assert M.coord(lo, 0.5) == -(1 << 20) and M.coord(np.nextafter(lo, -np.inf), 0.5) is None
    assert M.coord(np.nextafter(hi, -np.inf), 0.5) == (1 << 20) - 1 and M.coord(hi, 0.5) is None
    m = M.RefMap(0.5, 64)
    inside = [(lo, 0, 0), (0, lo, 0), (0, 0, lo), (np.nextafter(hi, 0), 0, 0), (0, np.nextafter(hi, 0), 0), (0, 0, np.nextafter(hi, 0))]
    outside = [(np.nextafter(lo, -np.inf), 0, 0), (0, np.nextafter(lo, -np.inf), 0), (0, 0, np.nextafter(lo, -np.inf)),
               (hi, 0, 0), (0, hi, 0), (0, 0, hi)]
    # (float32 inputs cannot be one binary64 ulp outside: the pose's translation carries the coordinate exactly)
    for pos, member in [(p, 1) for p in inside] + [(p, 0) for p in outside]:
        pose = R.rigid(np.eye(3), pos)
        info = m.insert(np.zeros((1, 4), np.float32), R.f4([[0, 0, 1.0]]), pose)
        assert info["n_members"] == member, pos
    assert len(m) == 6
    want = sorted([(-(1 << 20), 0, 0), (0, -(1 << 20), 0), (0, 0, -(1 << 20)), ((1 << 20) - 1, 0, 0), (0, (1 << 20) - 1, 0),
                   (0, 0, (1 << 20) - 1)], key=lambda c: (c[2], c[1], c[0]))
    assert [tuple(c) for c in m.fetch(M.COORDS)] == want
    # keys: z most significant, then y, then x, offset 2^20
    assert M.key(-(1 << 20), -(1 << 20), -(1 << 20)) == 0 and M.key(0, 0, 0) == ((1 << 20) << 42) + ((1 << 20) << 21) + (1 << 20)
    assert M.key((1 << 20) - 1, (1 << 20) - 1, (1 << 20) - 1) == (1 << 63) - 1


def _fold(xyz4, nrm4, pose, side, order):
    """The rule's sums for the points in `order`, all of which fall into one voxel: plain Python floats."""
    acc = [0.0] * 9
    P = np.asarray(pose, np.float64)
    for i in order:
        x, y, z = (float(v) for v in xyz4[i, :3])
        X = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
        a = [float(v) for v in nrm4[i, :3]]
        la = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        a = [v / la for v in a]
        m = [(P[r, 0] * a[0] + P[r, 1] * a[1]) + P[r, 2] * a[2] for r in range(3)]
        for k in range(3):
            acc[k] = acc[k] + X[k]
        for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            acc[3 + k] = acc[3 + k] + m[r] * m[c]
    return np.array(acc)


def test_fold_order():
    rng = np.random.default_rng(2)
    pose = R.rigid(R.rot(0.3, -0.2, 1.1), [0.5, -0.25, 2.0])
    pts, nrm = K.cloud_of_voxels([(0, 0, 0), (1, -2, 3), (-4, 0, 1)], 1.0, per_voxel=(40, 90, 7), seed=1)
    pts = K._local(pose, pts[:, :3].astype(np.float64))
    pts = R.f4(pts)
    n = pts.shape[0]
    whole = M.RefMap(1.0, 64)
    whole.insert(pts, nrm, pose)
    for k in (1, 37, n - 1):  # whole = [0:k] then [k:n], bit for bit
        parts = M.RefMap(1.0, 64)
        parts.insert(pts[:k], nrm[:k], pose)
        parts.insert(pts[k:], nrm[k:], pose)
        _same_map(whole, parts)
    # one voxel's points: the sums are the rule's fold in storage order, and a permuted cloud's are the fold in ITS order
    one, one_n = K.cloud_of_voxels([(2, 2, 2)], 1.0, per_voxel=(50,), seed=3)
    ident = np.eye(4)
    for order in (np.arange(50), rng.permutation(50)):
        m = M.RefMap(1.0, 4)
        m.insert(one[order], one_n[order], ident)
        assert np.array_equal(_bits(m.fetch(M.SUMS)[0]), _bits(_fold(one, one_n, ident, 1.0, order)))
    a, b = M.RefMap(1.0, 4), M.RefMap(1.0, 4)
    a.insert(one, one_n, ident)
    b.insert(one[::-1], one_n[::-1], ident)
    assert np.array_equal(a.fetch(M.COUNT), b.fetch(M.COUNT))
    assert not np.array_equal(_bits(a.fetch(M.SUMS)), _bits(b.fetch(M.SUMS)))  # (50 random doubles: the order shows)
    # A then B against B then A: the same voxels and counts, each the fold over ITS concatenation
    A, An = one[:20], one_n[:20]
    B, Bn = one[20:], one_n[20:]
    ab, ba = M.RefMap(1.0, 4), M.RefMap(1.0, 4)
    ab.insert(A, An)
    ab.insert(B, Bn)
    ba.insert(B, Bn)
    ba.insert(A, An)
    assert np.array_equal(_bits(ab.fetch(M.SUMS)[0]), _bits(_fold(one, one_n, ident, 1.0, np.arange(50))))
    assert np.array_equal(_bits(ba.fetch(M.SUMS)[0]), _bits(_fold(one, one_n, ident, 1.0, np.r_[20:50, 0:20])))
    assert ab.info()["n_inserts"] == 2 and ab.info()["n_members"] == 50


def test_members_are_filtered_on_each_of_the_five_conditions():
    ok_p, ok_n = [0.25, 0.25, 0.25], [0.0, 0.0, 2.0]
    cases = [  # (point, normal, pose, member)
        (ok_p, ok_n, np.eye(4), 1),
        ([np.nan, 0, 0], ok_n, np.eye(4), 0), ([0, np.inf, 0], ok_n, np.eye(4), 0),                    # p finite
        (ok_p, [0, 0, 0], np.eye(4), 0), (ok_p, [np.nan, 1, 0], np.eye(4), 0), (ok_p, [1, np.inf, 0], np.eye(4), 0),  # normal
        ([3e38, 3e38, 3e38], ok_n, R.rigid(np.full((3, 3), 1e300), [0, 0, 0]), 0),                     # X finite
        (ok_p, ok_n, R.rigid(np.eye(3), [1e7, 0, 0]), 0), (ok_p, ok_n, R.rigid(np.eye(3), [0, 0, -1e7]), 0),  # coordinates
    ]
    m = M.RefMap(1.0, 16)
    for p, a, pose, member in cases:
        info = m.insert(R.f4([p]), R.f4([a]), pose)
        assert (info["n_points"], info["n_members"]) == (1, member), (p, a)
    assert len(m) == 1 and m.info()["n_members"] == 1
    # the world normal is R (a / |a|), normalised once: under the identity m m^T of (0, 0, 2) is e_z e_z^T exactly
    assert m.fetch(M.SUMS)[0].tolist() == [0.25, 0.25, 0.25, 0, 0, 0, 0, 0, 1.0]
    # X stays in binary64: a world position that binary32 cannot hold keeps its bits
    m2 = M.RefMap(1.0, 4)
    m2.insert(R.f4([[0.1, 0.2, 0.3]]), R.f4([ok_n]), R.rigid(np.eye(3), [1000.0, 0, 0]))
    x = m2.fetch(M.SUMS)[0, 0]
    assert x == float(np.float32(0.1)) + 1000.0 and float(np.float32(x)) != x


def test_capacity_refusal_leaves_the_map_unchanged():
    coords, extra = K.crowded(64, 62)
    pts, nrm = K.cloud_of_voxels(coords, 1.0)
    m = M.RefMap(1.0, 64)
    m.insert(pts, nrm)
    assert len(m) == 62
    before = m.fetch_all()
    more, more_n = K.cloud_of_voxels(np.concatenate([coords[:5], extra[:3]]), 1.0, seed=5)  # 3 new voxels: 65 > 64
    with pytest.raises(M.CapacityError):
        m.insert(more, more_n)
    after = m.fetch_all()
    for k in (M.COORDS, M.COUNT, M.SUMS):
        assert np.array_equal(before[k], after[k])
    assert m.info()["n_inserts"] == 1
    fit, fit_n = K.cloud_of_voxels(np.concatenate([coords[:5], extra[:2]]), 1.0, seed=5)  # 2 new: exactly 64
    info = m.insert(fit, fit_n)
    assert info["n_new_voxels"] == 2 and info["n_touched_voxels"] == 7 and len(m) == 64


def test_hand_built_case_has_the_shapes_it_claims():
    inserts, s, sn = K.hand_built()
    m = M.RefMap(K.SIDE, 4096)
    infos = [m.insert(*c) for c in inserts]
    f = m.fetch_all()
    by = {tuple(c): int(n) for c, n in zip(f[M.COORDS], f[M.COUNT])}
    assert (by[K.V1], by[K.V65], by[K.V300], by[K.VALL]) == (1, 65, 300, 21)
    assert by[(K.LO, 0, 0)] == 1 and by[(0, K.HI, 0)] == 1 and not any(abs(c[2]) > 100 for c in by)
    # the points on faces went to the voxel the face opens: (1, .25, .25) -> (2, 0, 0), the origin -> (0, 0, 0), ...
    for c in ((2, 0, 0), (-3, -1, 0), (0, 0, 0), (0, 5, -4), (1, 1, 1), (-4, -4, -4)):
        assert c in by, c
    assert (f[M.COORDS] < 0).any() and sum(i["n_members"] for i in infos) < 700
    assert [i["n_points"] for i in infos] == [150, 420, 130]
    r = m.register(s, sn, np.eye(4), teps=0.0, feps=0.0, max_iter=1, corr_iter=0)
    assert r["corr"][:5].tolist() == [0] * 5 and (r["corr"][5:14] == -1).all() and r["corr"][14] == 0
    assert 150 < r["n_corr"] < 300
    r8 = m.register(s, sn, K.GUESS, teps=0.0, feps=0.0, max_iter=8)
    assert r8["valid"] and r8["iterations"] == 8


def test_map_registration_equals_method_3_on_the_positive_octant():
    """The chosen inputs of the GPU test: with a target point exactly at the origin, every other coordinate >= 0 and the
    identity pose, the world grid is method 3's and the two restatements agree bit for bit at every iteration."""
    s, sn, t, tn = K.octant_hand_built()
    for guess, iters in ((np.eye(4), 1), (K.GUESS, 10)):
        m = M.RefMap(1.0, 4096)
        m.insert(t, tn, None)
        a = m.register(s, sn, guess, teps=0.0, feps=0.0, max_iter=iters)
        b = V.run(s, sn, t, tn, guess, max_d=1.0, teps=0.0, feps=0.0, max_iter=iters)
        assert np.array_equal(b["grid"][:3], [0, 0, 0])
        assert a["iterations"] == b["iterations"] == iters
        assert np.array_equal(_bits(a["trace"]), _bits(b["trace"])) and np.array_equal(_bits(a["T"]), _bits(b["T"]))
        assert (a["n_corr"], a["stop_reason"]) == (b["n_corr"], b["stop_reason"])
        assert a["fitness"] == b["fitness"] and a["rmse"] == b["rmse"]
        assert np.array_equal(a["corr"] >= 0, b["corr"] >= 0)
        # the records too: method 3's at its representatives
        rec = b["records"][b["records"][:, 0] > 0]
        rec = rec[np.argsort(rec[:, 10])]
        f = m.fetch_all()
        lin = f[M.COORDS][:, 0] + 7 * (f[M.COORDS][:, 1] + 7 * f[M.COORDS][:, 2])
        assert np.array_equal(np.sort(lin), rec[:, 10].astype(np.int64))
        assert np.array_equal(_bits(f[M.RECORDS][np.argsort(lin)]), _bits(rec[:, 1:10]))


def test_constant_velocity_guess_is_the_api_s():
    from quatro_amd import api
    A = R.rigid(R.rot(0.01, 0.02, 0.3), [1.0, 2.0, 0.1])
    B = R.rigid(R.rot(0.015, 0.01, 0.35), [2.0, 2.4, 0.12])
    g = api.constant_velocity_guess(A, B)
    assert np.array_equal(_bits(g), _bits(M.constant_velocity_guess(A, B)))
    assert np.abs(g - B @ np.linalg.inv(A) @ B).max() < 1e-12


def test_the_ten_entry_points_are_declared_exported_and_bound():
    """The entry points of include/quatro_voxelmap.h are ten of libquatro_ext.so's exports, every one has its ctypes
    signature, and libquatro_hip.so exports none of them (its table stays include/quatro_hip.h's)."""
    import ctypes
    import os
    import subprocess
    import ext_abi
    from quatro_amd import lib as ql
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    assert len(ext_abi.check_header("quatro_voxelmap.h")) == 10
    src = r"""
#include <stdio.h>
#include "quatro_voxelmap.h"
int main(void){printf("%zu %zu %zu\n", sizeof(qtr_voxel_map_params), sizeof(qtr_voxel_map_info), sizeof(qtr_voxel_map_insert_info)); return 0;}
"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", os.path.join(d, "s")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    assert sizes == [ctypes.sizeof(ql.VoxelMapParams), ctypes.sizeof(ql.VoxelMapInfo), ctypes.sizeof(ql.VoxelMapInsertInfo)]
