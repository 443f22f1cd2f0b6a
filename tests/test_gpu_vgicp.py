"""Voxelised plane-to-plane (VGICP) refinement on the MI355X, method QTR_ICP_VOXEL_PLANE_TO_PLANE through qtr_gicp /
qtr_icp / qtr_refine_pair / qtr_submit_batch_refine and the keyframe entries: bit-parity with the host restatement of the
loop (tests/vgicp_ref/vgicp_ref.cpp) at every iteration, the path equalities of plane-to-plane, the batched path against
register + refine (the grid comes from the rule, not from an arena's capacity), isolation between the methods, the cell
cap, the C++ wrapper, and the accuracy on tilted scans."""
import os
import subprocess

import numpy as np
import pytest

import icp_restate as R
import vgicp_restate as V

pytestmark = pytest.mark.gpu

TILT = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")

# Rotation / translation error of the restatement (= the device, bit for bit) on the tilted kitti64_pair_16k(0..3) at the
# default parameters from the registration's T, known on the CPU before any GPU run (DESIGN.md section 9 has the table): the
# pairs on which the voxel method lowers the registration's rotation error.
IMPROVES = (0, 1, 2, 3)


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same_icp(a, b, what=""):
    assert a.get("status", 0) == b.get("status", 0), what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _same_reg(a, b, what=""):
    assert a["status"] == b["status"], what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert _f64bits(a["cost"]) == _f64bits(b["cost"]), what
    assert (a["n_src"], a["n_tgt"], a["L"]) == (b["n_src"], b["n_tgt"], b["L"]), what


def _tilted(pair):
    s, t, Tgt = pair
    return s, R.apply(TILT, t), TILT @ Tgt


def _perturbed(Tgt):
    return Tgt @ R.rigid(R.rot(0.012, -0.009, 0.015), [0.25, -0.3, 0.08])


def _vg(**kw):
    from quatro_amd import lib as ql
    return ql.default_icp_params(method=ql.ICP_VOXEL_PLANE_TO_PLANE, **kw)


def _handle(n_slots, **env):
    from quatro_amd import lib as ql
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ql.Handle(0, n_slots=n_slots)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def vox_pair(hip):
    """kitti64_pair(2)'s voxel clouds with both normal sets from qtr_fpfh."""
    from quatro_amd import synth
    s, t, Tgt = synth.kitti64_pair(2)
    vs, vt = hip.voxelize(s, 0.3), hip.voxelize(t, 0.3)
    ns, _ = hip.fpfh(vs, 0.5, 0.5)
    nt, _ = hip.fpfh(vt, 0.5, 0.5)
    return vs, vt, ns, nt, Tgt


@pytest.fixture(scope="module")
def pairs():
    """The ten pairs of tests/test_gpu_icp_batch.py: kitti64_pair(0..4) and kitti64_pair_16k(0..4), every other one with
    its target tilted."""
    from quatro_amd import synth
    out = []
    for k in range(5):
        for big in (False, True):
            p = (synth.kitti64_pair_16k if big else synth.kitti64_pair)(k)
            if (k + big) % 2 == 0:
                p = _tilted(p)
            out.append((p[0], p[1], 10 * k + big))
    return out


@pytest.fixture(scope="module")
def single_ref(pairs):
    """register_pair + refine_pair of the ten pairs with this method, per ICP keyword set (computed once, never changed)."""
    from quatro_amd import lib as ql
    cache = {}

    def get(icp_kw):
        key = tuple(sorted(icp_kw.items()))
        if key not in cache:
            h1 = _handle(1)
            try:
                out = []
                for s, t, seed in pairs:
                    r = h1.register_pair(s, t, ql.default_frontend_params(seed=seed))
                    out.append((r, h1.refine_pair(None, _vg(**icp_kw))))
                cache[key] = out
            finally:
                h1.close()
        return cache[key]
    return get


def test_vgicp_is_bit_equal_to_the_restatement_every_iteration(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    g = hip.gicp(vs, vt, ns, nt, G0, _vg(max_iterations=40))
    trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
    corr_last = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
    o = V.run(vs, ns, vt, nt, G0, max_iter=40)
    print(f"vgicp: {g['iterations']} iterations, stop {g['stop_reason']}, {g['n_corr']} correspondences, "
          f"rot err {R.rot_err_deg(G0, Tgt):.4f} -> {R.rot_err_deg(g['T'], Tgt):.4f} deg")
    assert g["valid"] and g["iterations"] >= 3
    assert (g["iterations"], g["stop_reason"], g["n_corr"]) == (o["iterations"], o["stop_reason"], o["n_corr"])
    assert np.array_equal(g["T"], o["T"]) and g["fitness"] == o["fitness"] and g["rmse"] == o["rmse"]
    assert np.array_equal(trace, o["trace"])
    assert np.array_equal(corr_last, o["corr"])
    # every iteration's correspondence set: the loop cut after k updates leaves iteration k's set behind
    for k in range(1, g["iterations"]):
        gk = hip.gicp(vs, vt, ns, nt, G0, _vg(max_iterations=k))
        ok = V.run(vs, ns, vt, nt, G0, max_iter=k, corr_iter=k - 1)
        assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_CORR, np.int32), ok["corr"]), k
        assert np.array_equal(gk["T"], o["trace"][k - 1, :16].reshape(4, 4)), k
    # a second run gives the same bits (k_icp_place's atomic ranks differ from run to run: the records do not)
    g2 = hip.gicp(vs, vt, ns, nt, G0, _vg(max_iterations=40))
    assert np.array_equal(g2["T"], g["T"])
    assert np.array_equal(hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18), trace)


def _hand_built():
    """n_t = 700 targets, n_s = 300 sources (neither a multiple of 256) on 1 m voxels over the box [0, 4]^3: voxel (0,0,0)
    with 1 member, (1,0,0) with 65 and (2,1,0) with 300 (each of the two also holds 5 points with unusable normals, which
    are not members), the rest spread over z >= 1; a target at the maximum corner (4, 4, 4), which opens cell (4, 4, 4) of a
    5 x 5 x 5 grid; a non-finite target; unusable normals on both sides; sources on faces and outside the grid.  The
    targets' storage order is a random permutation: members of a voxel lie anywhere."""
    rng = np.random.default_rng(5)

    def inside(cell, n):
        return np.array(cell) + 0.0625 + 0.875 * rng.random((n, 3))
    t = np.concatenate([inside((0, 0, 0), 1), inside((1, 0, 0), 65), inside((2, 1, 0), 300),
                        inside((1, 0, 0), 5), inside((2, 1, 0), 5),
                        rng.random((323, 3)) * np.array([4.0, 4.0, 3.0]) + np.array([0, 0, 1.0]),
                        [[4.0, 4.0, 4.0]]])
    t[0] = 0.0
    assert t.shape[0] == 700
    tn = rng.normal(size=(700, 3))
    tn[0] = [0.0, 0.0, 2.0]
    tn[366:371] = 0.0                     # not members
    tn[371:376, 1] = [np.nan, np.inf, np.nan, -np.inf, np.nan]
    tn[376::9] = 0.0                      # (among the spread ones too)
    tn[699] = [0.0, 1.0, 0.0]
    t[400] = np.nan                       # a non-finite target
    perm = rng.permutation(700)
    t4, tn4 = R.f4(t[perm]), R.f4(tn[perm])
    s = rng.random((300, 3)) * 4.4 - 0.2  # some outside the grid
    s[:6] = [[1.0, 0.5, 0.5], [2.0, 1.0, 0.5], [3.0, 2.0, 1.0], [0.0, 0.0, 0.0], [4.0, 4.0, 4.0], [5.0, 4.5, 4.5]]
    s[6] = [np.nan, 1.0, 1.0]
    s[7] = [1e30, 1.0, 1.0]
    sn = rng.normal(size=(300, 3))
    sn[8::19] = 0.0
    sn[9::23, 2] = np.inf
    sn[:8] = [0.0, 0.0, 1.0]
    return R.f4(s), R.f4(sn), t4, tn4


def test_hand_built_case_is_bit_equal_to_the_restatement(hip):
    from quatro_amd import lib as ql
    s, sn, t, tn = _hand_built()
    base = V.run(s, sn, t, tn, np.eye(4), max_iter=1)
    assert np.array_equal(base["grid"], [0, 0, 0, 5, 5, 5, 125])
    sizes = sorted(int(x) for x in base["records"][base["records"][:, 0] > 0, 0])
    print(f"hand-built: {len(sizes)} voxels, sizes {sizes[:3]} .. {sizes[-3:]}, first-iteration correspondences {base['n_corr']}")
    assert sizes[0] == 1 and sizes[-1] == 300 and 65 in sizes
    by_cell = {int(r[10]): int(r[0]) for r in base["records"] if r[0] > 0}
    assert (by_cell[0], by_cell[1], by_cell[2 + 5 * 1], by_cell[124]) == (1, 65, 300, 1)
    # the sources on faces, at the origin and at the corner: [1, .5, .5] -> cell (1,0,0), [2, 1, .5] -> (2,1,0), the origin
    # and the corner their own voxels; [3, 2, 1] an existing or an empty voxel; outside, NaN and huge: none
    rep = {int(r[10]): j for j, r in enumerate(base["records"]) if r[0] > 0}
    assert base["corr"][:2].tolist() == [rep[1], rep[7]] and base["corr"][3:5].tolist() == [rep[0], rep[124]]
    assert (base["corr"][5:8] == -1).all()
    # the identity: every matched source reports its voxel's representative, the lowest member index (restated records)
    reps = set(np.flatnonzero(base["records"][:, 0] > 0).tolist())
    assert set(base["corr"][base["corr"] >= 0].tolist()) <= reps
    for guess, iters in ((np.eye(4), 1), (R.rigid(R.rot(0.01, -0.02, 0.015), [0.05, -0.04, 0.03]), 8)):
        g = hip.gicp(s, t, sn, tn, guess, _vg(max_iterations=iters, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0))
        corr = hip.debug_fetch(ql.DBG_ICP_CORR, np.int32)
        trace = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
        o = V.run(s, sn, t, tn, guess, max_iter=iters, teps=0.0, feps=0.0)
        _same_icp(g, o, f"{iters} iterations")
        assert np.array_equal(corr, o["corr"]) and np.array_equal(trace, o["trace"])
        assert g["valid"] and g["iterations"] == iters


def test_refine_pair_and_the_normal_paths_give_qtr_gicps_bits(hip, vox_pair):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, Tgt = _tilted(synth.kitti64_pair_16k(1))
    fp = ql.default_frontend_params(seed=1)
    r = hip.register_pair(s, t, fp)
    p = hip.refine_pair(None, _vg())
    vs = hip.debug_fetch(ql.DBG_VOX_SRC, np.float32).reshape(-1, 4)
    vt = hip.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
    ns, _ = hip.fpfh(vs, fp.normal_radius, fp.fpfh_radius)
    nt, _ = hip.fpfh(vt, fp.normal_radius, fp.fpfh_radius)
    q = hip.gicp(vs, vt, ns, nt, r["T"], _vg())
    assert p["valid"] and p["iterations"] >= 2
    _same_icp(p, q, "refine_pair vs qtr_gicp on the slot's clouds")
    # NULL normals = explicit ones
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    prm = _vg(normal_radius=0.5)
    a = hip.gicp(vs, vt, ns, nt, G0, prm)
    assert a["valid"] and a["iterations"] >= 3
    for got, what in ((hip.icp(vs, vt, None, G0, prm), "qtr_icp, no normals"),
                      (hip.icp(vs, vt, nt, G0, prm), "qtr_icp, target normals"),
                      (hip.gicp(vs, vt, None, None, G0, prm), "qtr_gicp, no normals"),
                      (hip.gicp(vs, vt, ns, None, G0, prm), "qtr_gicp, source normals"),
                      (hip.gicp(vs, vt, None, nt, G0, prm), "qtr_gicp, target normals")):
        _same_icp(a, got, what)


def test_device_memory_and_keyframes_give_the_host_paths_bits(hip, vox_pair, pairs):
    import torch
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    prm = _vg()
    d = [torch.from_numpy(x).cuda() for x in (vs, vt, ns, nt)]
    a = hip.gicp(vs, vt, ns, nt, G0, prm)
    _same_icp(a, hip.gicp(d[0], d[1], d[2], d[3], G0, prm), "qtr_gicp, both normal sets")
    _same_icp(a, hip.gicp(d[0], d[1], None, None, G0, prm), "qtr_gicp, no normals")
    _same_icp(a, hip.icp(d[0], d[1], d[3], G0, prm), "qtr_icp, target normals")
    # qtr_register_keyframes + refine = the raw-scan path
    for i in (0, 3):
        s, t, seed = pairs[i]
        fp = ql.default_frontend_params(seed=seed)
        hip.register_pair(s, t, fp)
        want = hip.refine_pair(None, prm)
        ks, kt = hip.keyframe(s), hip.keyframe(t)
        try:
            hip.register_keyframes(ks, kt, fp)
            _same_icp(hip.refine_pair(None, prm), want, f"keyframes, pair {i}")
        finally:
            ks.close()
            kt.close()
        assert want["valid"]


CASES = [  # (batch slots, ICP parameters, environment of the batch handle, method-0 distance that sizes the arenas first)
    (16, {}, {}, None),                              # two lanes of 8, the defaults
    (4, {"max_iterations": 4}, {}, None),            # slots reused chunk after chunk; a short loop
    (4, {}, {"QTR_ICP_BLOCK": "5"}, None),           # blocks of 5 launches
    # 0.3 m voxels: 0.83 M .. 1.9 M cells over these boxes, on either side of the 2^20 cells every slot reserves for a batch
    # (a method-0 batch at 3 m has sized the arenas first): a grid derived from the table's capacity would show
    (4, {"max_correspondence_distance": 0.3}, {}, 3.0),
]


@pytest.mark.parametrize("n_slots,icp_kw,env,first_d", CASES)
def test_batch_refine_is_bit_equal_to_the_single_pair_path(pairs, single_ref, n_slots, icp_kw, env, first_d):
    from quatro_amd import lib as ql
    ref = single_ref(icp_kw)
    hb = _handle(n_slots, **env)
    try:
        if first_d is not None:
            hb.register_batch_refine(pairs[:n_slots], icp=ql.default_icp_params(max_correspondence_distance=first_d))
        res, refined = hb.register_batch_refine(pairs, icp=_vg(**icp_kw))
        kf = [(hb.keyframe(s), hb.keyframe(t), seed) for s, t, seed in pairs[:4]]
        try:
            kres, kref = hb.register_batch_keyframes(kf, icp=_vg(**icp_kw))
        finally:
            for a, b, _ in kf:
                a.close()
                b.close()
    finally:
        hb.close()
    for i, ((r1, g1), r, g) in enumerate(zip(ref, res, refined)):
        assert r["status"] == ql.QTR_OK and g["status"] == ql.QTR_OK and (g["valid"] or first_d is not None), i
        _same_reg(r, r1, f"result {i} vs register_pair")
        _same_icp(g, g1, f"refined {i}")
    for i in range(4):
        _same_icp(kref[i], ref[i][1], f"keyframe batch, refined {i}")
    print(f"{n_slots} slots {icp_kw}: iterations {sorted({g['iterations'] for g in refined})}, "
          f"stop reasons {sorted({g['stop_reason'] for g in refined})}")


def test_mixed_batch_leaves_a_correspondence_only_pair_unrefined():
    from quatro_amd import lib as ql
    from quatro_amd import synth
    a = _tilted(synth.kitti64_pair_16k(0))
    b = synth.kitti64_pair(1)
    cs, ct, _, _ = synth.correspondences(L=2000, inlier_frac=0.2, seed=3)
    mixed = [(a[0], a[1], 1), (None, None, 2, cs, ct), (b[0], b[1], 3)]
    hb = _handle(4)
    h1 = _handle(1)
    try:
        res, refined = hb.register_batch_refine(mixed, icp=_vg())
        single = []
        for i in (0, 2):
            h1.register_pair(mixed[i][0], mixed[i][1], ql.default_frontend_params(seed=mixed[i][2]))
            single.append(h1.refine_pair(None, _vg()))
    finally:
        hb.close()
        h1.close()
    assert [r["status"] for r in res] == [ql.QTR_OK] * 3
    assert [g["status"] for g in refined] == [ql.QTR_OK, ql.QTR_ERR_NOT_RUN, ql.QTR_OK]
    assert not refined[1]["valid"] and np.array_equal(refined[1]["T"], res[1]["T"])
    _same_icp(refined[0], single[0], "pair 0")
    _same_icp(refined[2], single[1], "pair 2")


def test_no_state_crosses_between_the_methods(hip, vox_pair):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, _ = _tilted(synth.kitti64_pair(3))
    fp = ql.default_frontend_params(seed=3)
    hip.register_pair(s, t, fp)
    alone = [hip.refine_pair(None, ql.default_icp_params(method=m)) for m in (0, 1, 2)]
    hip.register_pair(s, t, fp)
    g = hip.refine_pair(None, _vg())
    after = [hip.refine_pair(None, ql.default_icp_params(method=m)) for m in (0, 1, 2)]
    g2 = hip.refine_pair(None, _vg())
    for m in (0, 1, 2):
        _same_icp(alone[m], after[m], f"method {m} after the voxel method")
    _same_icp(g, g2, "the voxel method after the other three")
    # no stale records: plane-to-plane on ANOTHER target, then the voxel method on this one
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    want = hip.gicp(vs, vt, ns, nt, G0, _vg())
    hip.register_pair(s, t, fp)
    hip.refine_pair(None, _vg(max_correspondence_distance=2.0))     # other records in the arena
    hip.refine_pair(None, ql.default_icp_params(method=ql.ICP_PLANE_TO_PLANE))
    _same_icp(hip.gicp(vs, vt, ns, nt, G0, _vg()), want, "after a plane-to-plane call on a different target")
    _same_icp(want, V.run(vs, ns, vt, nt, G0), "restatement")


def test_only_the_two_plane_to_plane_methods_go_through_qtr_gicp_and_the_cell_cap_refuses(hip, vox_pair):
    from quatro_amd import lib as ql
    vs, vt, ns, nt, Tgt = vox_pair
    for method in (ql.ICP_POINT_TO_PLANE, ql.ICP_POINT_TO_POINT, 4, 7):
        with pytest.raises(ql.QuatroHipError) as ei:
            hip.gicp(vs, vt, ns, nt, Tgt, ql.default_icp_params(method=method))
        assert ei.value.code == ql.QTR_ERR_BAD_ARG, method
    e = hip.gicp(vs[:0], vt, ns[:0], nt, Tgt, _vg())
    assert not e["valid"] and np.array_equal(e["T"], Tgt)
    e = hip.gicp(vs, np.full_like(vt, np.nan), ns, nt, Tgt, _vg())  # no finite target point
    assert not e["valid"] and e["stop_reason"] == 4 and np.array_equal(e["T"], Tgt)
    # the cell cap: 0.01 m voxels on a 10 m box; the slot stays usable and the grid is not coarsened
    rng = np.random.default_rng(1)
    t = R.f4(rng.random((500, 3)) * 10.0)
    t[0, :3], t[1, :3] = 0.0, 10.0
    n = R.f4(np.tile([0.0, 0.0, 1.0], (500, 1)))
    G0 = _perturbed(Tgt)
    want = hip.gicp(vs, vt, ns, nt, G0, _vg())
    with pytest.raises(ql.QuatroHipError) as ei:
        hip.gicp(t, t, n, n, np.eye(4), _vg(max_correspondence_distance=0.01))
    assert ei.value.code == ql.QTR_ERR_CAPACITY and "0.01" in str(ei.value) and "10" in str(ei.value), str(ei.value)
    assert V.run(t, n, t, n, np.eye(4), max_d=0.01)["status"] == V.CAPACITY
    _same_icp(hip.gicp(vs, vt, ns, nt, G0, _vg()), want, "after the refusal")
    # in a batch only that pair's refined status carries it
    from quatro_amd import synth
    a = synth.kitti64_pair(1)
    hb = _handle(2)
    try:
        res, refined = hb.register_batch_refine([(a[0], a[1], 3)], icp=_vg(max_correspondence_distance=0.05))
        res2, refined2 = hb.register_batch_refine([(a[0], a[1], 3)], icp=_vg())
    finally:
        hb.close()
    assert res[0]["status"] == ql.QTR_OK and refined[0]["status"] == ql.QTR_ERR_CAPACITY and not refined[0]["valid"]
    assert np.array_equal(refined[0]["T"], res[0]["T"])
    assert refined2[0]["status"] == ql.QTR_OK and refined2[0]["valid"]


def test_python_class_reaches_the_voxel_method(hip, vox_pair):
    from quatro_amd import api
    vs, vt, ns, nt, Tgt = vox_pair
    icp = api.IterativeClosestPoint(handle=hip, method="voxel_plane_to_plane")
    icp.setInputSource(vs)
    icp.setInputTarget(vt)
    icp.setSourceNormals(ns)
    icp.setTargetNormals(nt)
    out = icp.align(_perturbed(Tgt))
    assert icp.hasConverged() and out.shape == vs.shape
    assert np.array_equal(icp.getFinalTransformation(), hip.gicp(vs, vt, ns, nt, _perturbed(Tgt), _vg())["T"])


@pytest.mark.parametrize("normals", ["computed", "given"])
def test_cpp_vgicp_demo_gives_the_python_paths_bits(hip, vox_pair, tmp_path, normals):
    from quatro_amd import build as qbuild
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "vgicp_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "vgicp_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    vs, vt, ns, nt, Tgt = vox_pair
    G0 = _perturbed(Tgt)
    for a, name in ((vs, "s.bin"), (vt, "t.bin"), (ns, "ns.bin"), (nt, "nt.bin")):
        a.tofile(str(tmp_path / name))
    (tmp_path / "g.txt").write_text(" ".join(repr(float(x)) for x in G0.reshape(-1)))
    args = [exe, str(tmp_path / "s.bin"), str(tmp_path / "t.bin"), str(tmp_path / "g.txt")]
    if normals == "given":
        args += [str(tmp_path / "ns.bin"), str(tmp_path / "nt.bin")]
    out = subprocess.run(args, capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    T = np.array([int(w, 16) for ln in out[1:5] for w in ln.split()], dtype=np.uint64).view(np.float64).reshape(4, 4)
    g = hip.gicp(vs, vt, ns, nt, G0, _vg()) if normals == "given" else hip.gicp(vs, vt, None, None, G0, _vg())
    assert np.array_equal(T, g["T"]), (out, g["T"])


def test_voxel_method_against_the_registration_on_tilted_scans(hip):
    """Rotation / translation error against the generator's truth on the tilted kitti64_pair_16k(0..3) at the default
    parameters, from the registration's T: the registration, plane-to-plane, the voxel method (the table of DESIGN.md
    section 9).  The voxel method's result is the host restatement's, bit for bit, so which pairs improve is known on the
    CPU: IMPROVES lists them, and the assertion is made on exactly those."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    rows = []
    for k in range(4):
        s, t, Tgt = _tilted(synth.kitti64_pair_16k(k))
        fp = ql.default_frontend_params(seed=k)
        r = hip.register_pair(s, t, fp)
        p2p = hip.refine_pair(None, ql.default_icp_params(method=ql.ICP_PLANE_TO_PLANE))
        g = hip.refine_pair(None, _vg())
        vs = hip.debug_fetch(ql.DBG_VOX_SRC, np.float32).reshape(-1, 4)
        vt = hip.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
        ns, _ = hip.fpfh(vs, fp.normal_radius, fp.fpfh_radius)
        nt, _ = hip.fpfh(vt, fp.normal_radius, fp.fpfh_radius)
        o = V.run(vs, ns, vt, nt, r["T"])
        _same_icp({**g, "status": 0}, o, f"pair {k}: device vs restatement")
        e = [R.rot_err_deg(x["T"], Tgt) for x in (r, p2p, g)]
        d = [float(np.linalg.norm(x["T"][:3, 3] - Tgt[:3, 3])) for x in (r, p2p, g)]
        print(f"pair {k}: quatro {e[0]:.3f} deg {d[0]:.3f} m | plane-to-plane {e[1]:.3f} deg {d[1]:.3f} m, "
              f"{p2p['iterations']} it, stop {p2p['stop_reason']} | voxel {e[2]:.3f} deg {d[2]:.3f} m, "
              f"{g['iterations']} it, stop {g['stop_reason']}, {g['n_corr']} corr")
        rows.append((g["valid"], e[0], e[2]))
    for k, (valid, e0, e2) in enumerate(rows):
        assert valid, k
        if k in IMPROVES:
            assert e2 < e0, (k, e0, e2)
