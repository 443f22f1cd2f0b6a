"""The cross-workgroup reduction the ICP iteration and the evaluation share (icp_reduce_tail, icp.hip) at the workgroup
counts where it can go wrong: sources of 1, 255, 256, 257 and 513 points (1, 1, 1, 2 and 3 workgroups of 256) against a
target of 300.  Per size: two iterations of each ICP method, one evaluation, and a batch of keyframe evaluations whose
pairs mix the sizes on both sides (the grouped kernels, the per-pair box fold included).  Every record is compared bit for
bit with its restatement, called as test_gpu_icp.py, test_gpu_gicp.py and test_gpu_eval.py call them.  Both normal sets
are explicit, so no FPFH chain runs in the raw-cloud cases.

The scene is a jittered 0.4 m lattice on three faces of a cube: no two points share a 0.3 m voxel, so a keyframe made of
n of them has exactly n voxels (asserted) and the batch reaches the same sizes, the one-voxel keyframe included."""
import numpy as np
import pytest

import eval_restate as er
import gicp_restate as G
import icp_restate as R

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 513)
N_TGT = 300
# what the source is off by: the ICP's guess and the evaluated transform
T0 = R.rigid(R.rot(0.010, -0.008, 0.012), [0.05, -0.04, 0.03])


def _scene(n, seed):
    """n points of the lattice (14 x 14 sites on each of the faces x = 0, y = 0, z = 0, the first site 0.4 m from the
    edges) moved by up to 0.03 m along every axis, and their faces' normals."""
    rng = np.random.default_rng(seed)
    sites = rng.permutation(3 * 196)[:n]
    face, i, j = sites // 196, (sites % 196) // 14, sites % 14
    pts, nrm = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    for f in range(3):
        m = face == f
        a, b = [x for x in range(3) if x != f]
        pts[m, a], pts[m, b] = 0.4 * (i[m] + 1), 0.4 * (j[m] + 1)
        nrm[m, f] = 1.0
    pts[:, :3] += rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32)
    return pts, nrm


@pytest.fixture(scope="module")
def clouds():
    tgt, tgt_nrm = _scene(N_TGT, 1)
    src, src_nrm = _scene(max(SIZES), 2)
    return src, src_nrm, tgt, tgt_nrm


@pytest.mark.parametrize("n", SIZES)
def test_two_iterations_of_every_method_equal_the_restatements(hip, clouds, n):
    from quatro_amd import lib as ql
    src, src_nrm, tgt, tgt_nrm = clouds
    s, a = src[:n], src_nrm[:n]
    for method in (ql.ICP_POINT_TO_PLANE, ql.ICP_POINT_TO_POINT, ql.ICP_PLANE_TO_PLANE):
        prm = ql.default_icp_params(method=method, max_iterations=2)
        if method == ql.ICP_PLANE_TO_PLANE:
            g = hip.gicp(s, tgt, a, tgt_nrm, T0, prm)
            o = G.run(s, a, tgt, tgt_nrm, T0, max_iter=2)
        else:
            g = hip.icp(s, tgt, tgt_nrm, T0, prm)
            o = R.run(s, tgt, tgt_nrm, T0, max_iter=2, method=method)
        trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
        corr = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
        what = f"{n} points, method {method}"
        print(f"{what}: {g['iterations']} iterations, stop {g['stop_reason']}, {g['n_corr']} correspondences")
        assert g["status"] == 0, what
        assert (g["iterations"], g["stop_reason"], g["n_corr"], g["valid"], g["converged"]) == \
            (o["iterations"], o["stop_reason"], o["n_corr"], o["valid"], o["converged"]), what
        assert np.array_equal(er.bits(g["T"]), er.bits(o["T"])), what
        assert np.array_equal(er.bits([g["fitness"], g["rmse"]]), er.bits([o["fitness"], o["rmse"]])), what
        assert np.array_equal(er.bits(trace), er.bits(o["trace"])), what
        assert np.array_equal(corr, o["corr"]), what
        if n >= 255:  # (the sums are of many terms: nearly every source point has a target within reach)
            assert g["iterations"] == 2 and g["n_corr"] > n // 2, what


@pytest.mark.parametrize("n", SIZES)
def test_one_evaluation_equals_the_restatement(hip, clouds, n):
    from quatro_amd import lib as ql
    src, _, tgt, tgt_nrm = clouds
    got = hip.evaluate(src[:n], tgt, T0, tgt_nrm)
    want = er.evaluate(src[:n], tgt, T0, 1.0, tgt_nrm)
    assert got["status"] == 0 and er.same_record(got, want) == [], (n, er.same_record(got, want))
    assert np.array_equal(hip.debug_fetch(ql.DBG_EVAL_CORR, np.int32), want["corr"]), n
    assert got["n_source"] == n and (n < 255 or got["n_plane"] > n // 2), (n, got["n_plane"])


def test_a_batch_of_keyframe_evaluations_mixes_the_sizes(hip, clouds):
    from quatro_amd import lib as ql
    src, _, tgt, _ = clouds
    kfs = {n: hip.keyframe(src[:n]) for n in SIZES}
    kfs[N_TGT] = hip.keyframe(tgt)
    try:
        vox = {n: kf.fetch(ql.KF_VOX) for n, kf in kfs.items()}
        nrm = {n: kf.fetch(ql.KF_NORMALS) for n, kf in kfs.items()}
        for n in kfs:
            assert vox[n].shape[0] == n == kfs[n].info["n_voxels"], (n, vox[n].shape)
        # every size as a source against the 300, then targets of one, two and three workgroups of the box fold
        pairs = [(n, N_TGT) for n in SIZES] + [(N_TGT, 1), (257, 513), (513, 256), (1, 255)]
        got = hip.evaluate_keyframes_batch([(kfs[a], kfs[b], T0) for a, b in pairs])
        assert len(got) == len(pairs)
        for (a, b), g in zip(pairs, got):
            want = er.evaluate(vox[a], vox[b], T0, 1.0, nrm[b])
            assert g["status"] == 0 and er.same_record(g, want) == [], ((a, b), er.same_record(g, want))
            assert g["n_source"] == a, (a, b)
            one = hip.evaluate_keyframes(kfs[a], kfs[b], T0)
            assert er.same_record(one, g) == [], (a, b)
        assert sum(g["n_corr"] for g in got) > 1000
    finally:
        for kf in kfs.values():
            kf.close()
