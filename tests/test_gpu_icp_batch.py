"""Batched ICP refinement on the MI355X (qtr_submit_batch_refine): every refined record bit-equal to register_pair +
refine_pair of the same pair, every registration record bit-equal to register_batch, tilted pairs brought to the
single-pair bounds, the documented statuses of a mixed batch, device memory, no side effects, bad arguments and raw
sweeps."""
import ctypes
import os

import numpy as np
import pytest

import icp_restate as R

pytestmark = pytest.mark.gpu

LIM = {}  # (the default limits: 65536 voxels, so the 10^5-point random cloud below is over them)
TILT = R.rigid(R.rot(np.radians(1.5), np.radians(-1.0), 0.0), np.zeros(3))
ICP_KEYS = ("iterations", "stop_reason", "n_corr", "valid", "converged")


def _tilted(pair):
    s, t, Tgt = pair
    return s, R.apply(TILT, t), TILT @ Tgt


@pytest.fixture(scope="module")
def pairs():
    """Ten pairs: kitti64_pair(0..4) and kitti64_pair_16k(0..4), every other one with its target tilted."""
    from quatro_amd import synth
    out = []
    for k in range(5):
        for big in (False, True):
            p = (synth.kitti64_pair_16k if big else synth.kitti64_pair)(k)
            if (k + big) % 2 == 0:
                p = _tilted(p)
            out.append((p[0], p[1], 10 * k + big))
    return out


def _handle(n_slots, **env):
    from quatro_amd import lib as ql
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ql.Handle(0, n_slots=n_slots, **LIM)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _f64bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _same_icp(a, b, what=""):
    assert a["status"] == b["status"], what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert all(a[k] == b[k] for k in ICP_KEYS), (what, [(k, a[k], b[k]) for k in ICP_KEYS])
    assert _f64bits(a["fitness"]) == _f64bits(b["fitness"]) and _f64bits(a["rmse"]) == _f64bits(b["rmse"]), what


def _same_reg(a, b, what=""):
    assert a["status"] == b["status"], what
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)), what
    assert _f64bits(a["cost"]) == _f64bits(b["cost"]), what
    assert (a["n_src"], a["n_tgt"], a["L"]) == (b["n_src"], b["n_tgt"], b["L"]), what
    for k in ("clique", "final_inliers"):
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), (what, k)


def _single(h1, pairs, icp):
    """register_pair + refine_pair(None, icp) of every pair on a one-slot handle."""
    from quatro_amd import lib as ql
    out = []
    for s, t, seed in pairs:
        r = h1.register_pair(s, t, ql.default_frontend_params(seed=seed))
        out.append((r, h1.refine_pair(None, icp)))
    return out


CASES = [  # (batch slots, ICP parameters, environment of the batch handle)
    (16, {}, {}),                                                   # two lanes of 8
    (4, {"max_iterations": 4}, {}),                                 # slots reused chunk after chunk; a short loop
    (4, {"method": 1, "max_iterations": 12}, {"QTR_ICP_BLOCK": "5"}),  # point-to-point, blocks of 5 launches
]


@pytest.mark.parametrize("n_slots,icp_kw,env", CASES)
def test_batch_refine_is_bit_equal_to_the_single_pair_path(pairs, n_slots, icp_kw, env):
    from quatro_amd import lib as ql
    icp = ql.default_icp_params(**icp_kw)
    h1 = _handle(1)
    hb = _handle(n_slots, **env)
    hp = _handle(n_slots)
    try:
        ref = _single(h1, pairs, icp)
        plain = hp.register_batch(pairs)
        res, refined = hb.register_batch_refine(pairs, icp=icp)
    finally:
        h1.close()
        hb.close()
        hp.close()
    for i, ((r1, g1), p, r, g) in enumerate(zip(ref, plain, res, refined)):
        assert r["status"] == ql.QTR_OK, i
        _same_reg(r, p, f"result {i}")
        _same_reg(r, r1, f"result {i} vs register_pair")
        _same_icp(g, g1, f"refined {i}")
    its = {g["iterations"] for g in refined}
    reasons = {g["stop_reason"] for g in refined}
    print(f"{n_slots} slots {icp_kw}: iterations {sorted(its)}, stop reasons {sorted(reasons)}")
    if not icp_kw:  # (pairs of one group stop at different iterations)
        assert len(its) > 1


def test_batch_refine_brings_tilted_pairs_to_the_single_pair_bounds():
    from quatro_amd import lib as ql
    from quatro_amd import synth
    tp = [_tilted(synth.kitti64_pair_16k(k)) for k in range(4)]
    hb = _handle(8)
    h1 = _handle(1)
    try:
        res, refined = hb.register_batch_refine([(s, t, k) for k, (s, t, _) in enumerate(tp)])
        single = _single(h1, [(s, t, k) for k, (s, t, _) in enumerate(tp)], ql.default_icp_params())
    finally:
        hb.close()
        h1.close()
    for k, (g, (_, g1)) in enumerate(zip(refined, single)):
        _same_icp(g, g1, f"pair {k}")
    errs = []
    for k, ((_, _, Tgt), r, g) in enumerate(zip(tp, res, refined)):
        e0, e1 = R.rot_err_deg(r["T"], Tgt), R.rot_err_deg(g["T"], Tgt)
        dt = np.linalg.norm(g["T"][:3, 3] - Tgt[:3, 3])
        print(f"pair {k}: quatro {e0:.3f} deg -> icp {e1:.3f} deg, {dt:.3f} m, {g['iterations']} iterations, "
              f"stop {g['stop_reason']}")
        errs.append((g["status"], g["valid"], e0, e1, dt))
    # (measured: 0.094, 0.076, 0.320 and 0.151 deg, 2.4-4.5 cm.  Pair 2 stops on transformation_epsilon at 0.32 deg with
    # the default parameters — the single-pair path's own bits, checked above — so it is held to e0 / 3 and 8 cm only)
    for k, (st, valid, e0, e1, dt) in enumerate(errs):
        assert st == ql.QTR_OK and valid, k
        assert e0 >= 1.5 and e1 <= e0 / 3 and dt <= 0.08, k
        assert e1 <= 0.25 or k == 2, k


def test_mixed_batch_statuses_and_clean_batch_equality():
    from quatro_amd import lib as ql
    from quatro_amd import synth
    a = _tilted(synth.kitti64_pair_16k(0))
    b = synth.kitti64_pair_16k(1)
    c = _tilted(synth.kitti64_pair_16k(2))
    cs, ct, _, _ = synth.correspondences(L=2000, inlier_frac=0.2, seed=3)
    big = np.zeros((100000, 4), dtype=np.float32)  # ~10^5 voxels at 0.3 m: over max_voxels
    big[:, :3] = np.random.default_rng(5).uniform(-100, 100, (100000, 3))
    empty = np.zeros((0, 4), dtype=np.float32)
    mixed = [(a[0], a[1], 1),                # scans
             (None, None, 2, cs, ct),         # correspondences only
             (b[0], b[1], 3, cs, ct),         # scans + correspondences
             (big, big, 4),                   # over max_voxels
             (c[0], c[1], 5, empty, empty)]   # scans + zero correspondences: clique too small, still refined
    hb = _handle(8)
    hc = _handle(8)
    try:
        res, refined = hb.register_batch_refine(mixed)
        clean = [mixed[0], mixed[2], mixed[4]]
        cres, cref = hc.register_batch_refine(clean)
    finally:
        hb.close()
        hc.close()
    st = [r["status"] for r in res]
    assert st == [ql.QTR_OK, ql.QTR_OK, ql.QTR_OK, ql.QTR_ERR_CAPACITY, ql.QTR_ERR_CLIQUE_TOO_SMALL], st
    assert [g["status"] for g in refined] == [ql.QTR_OK, ql.QTR_ERR_NOT_RUN, ql.QTR_OK, ql.QTR_ERR_NOT_RUN, ql.QTR_OK]
    for i in (1, 3):  # not refined: the registration's T, not valid
        assert not refined[i]["valid"] and np.array_equal(refined[i]["T"], res[i]["T"]), i
    assert refined[0]["valid"]  # (pair 2 starts from the T of unrelated correspondences: whatever ICP makes of it)
    for j, i in enumerate((0, 2, 4)):
        _same_reg(res[i], cres[j], f"result {i}")
        _same_icp(refined[i], cref[j], f"refined {i}")


def test_device_memory_form_gives_the_host_bits(pairs):
    import torch
    from quatro_amd import lib as ql
    sub = pairs[:6]
    icp = ql.default_icp_params()
    hb = _handle(4)
    try:
        hres, href = hb.register_batch_refine(sub, icp=icp)
        items = [{"src": torch.from_numpy(np.ascontiguousarray(s)).cuda(), "tgt": torch.from_numpy(np.ascontiguousarray(t)).cuda(),
                  "fp": ql.default_frontend_params(seed=seed)} for s, t, seed in sub]
        torch.cuda.synchronize()
        dres, dref = hb.register_batch_dev_refine(items, ql.demo_params(), icp)
    finally:
        hb.close()
    for i in range(len(sub)):
        assert np.array_equal(dres[i]["T"].view(np.uint64), hres[i]["T"].view(np.uint64)), i
        _same_icp(dref[i], href[i], f"pair {i}")


def test_batch_refine_has_no_side_effects(pairs):
    from quatro_amd import lib as ql
    sub = pairs[:5]
    s, t, seed = pairs[1]
    fp = ql.default_frontend_params(seed=seed)
    icp = ql.default_icp_params()
    hb = _handle(4)
    hf = _handle(4)
    try:
        before = hb.register_pair(s, t, fp)
        before_icp = hb.refine_pair(None, icp)
        hb.register_batch_refine(sub, icp=icp)
        with pytest.raises(ql.QuatroHipError) as e:
            hb.refine_pair(None, icp)
        assert e.value.code == ql.QTR_ERR_BAD_ARG
        after = hb.register_batch(sub)
        fresh = hf.register_batch(sub)
        for i, (x, y) in enumerate(zip(after, fresh)):
            _same_reg(x, y, f"register_batch {i}")
        with pytest.raises(ql.QuatroHipError) as e:
            hb.refine_pair(None, icp)
        assert e.value.code == ql.QTR_ERR_BAD_ARG
        hb.register_batch_refine(sub, icp=icp)
        again = hb.register_pair(s, t, fp)
        again_icp = hb.refine_pair(None, icp)
    finally:
        hb.close()
        hf.close()
    _same_reg(again, before, "register_pair")
    _same_icp(again_icp, before_icp, "refine_pair")


def test_bad_arguments_are_refused_with_nothing_enqueued(pairs):
    from quatro_amd import lib as ql
    C = ctypes
    sub = pairs[:2]
    icp = ql.default_icp_params()
    hb = _handle(4)
    try:
        good_res, good_ref = hb.register_batch_refine(sub, icp=icp)
        keep = [(ql._f4(s), ql._f4(t)) for s, t, _ in sub]
        descs = (ql.PairDesc * 2)()
        for i, ((s, t), (_, _, seed)) in enumerate(zip(keep, sub)):
            descs[i] = ql.PairDesc(s.ctypes.data, s.shape[0], t.ctypes.data, t.shape[0], seed, None, None, 0, None, None, 0)
        fp, prm = ql.default_frontend_params(), ql.demo_params()
        results, refined = (ql.Result * 2)(), (ql.IcpResult * 2)()
        lib = hb._lib
        bad_icp = ql.default_icp_params(max_iterations=0)
        calls = [(None, refined), (C.byref(icp), None), (C.byref(bad_icp), refined)]
        for k, (ip, rf) in enumerate(calls):
            rc = lib.qtr_submit_batch_refine(hb._h, descs, 2, C.byref(fp), C.byref(prm), ip, results, rf, ql.MEM_HOST)
            assert rc == ql.QTR_ERR_BAD_ARG, k
            assert lib.qtr_wait(hb._h) == ql.QTR_OK  # (nothing in flight)
            res, ref = hb.register_batch_refine(sub, icp=icp)
            for i in range(2):
                _same_reg(res[i], good_res[i], f"call {k} pair {i}")
                _same_icp(ref[i], good_ref[i], f"call {k} pair {i}")
        rc = lib.qtr_submit_batch_refine(hb._h, descs, 0, C.byref(fp), C.byref(prm), C.byref(icp), results, None,
                                         ql.MEM_HOST)
        assert rc == ql.QTR_OK and lib.qtr_wait(hb._h) == ql.QTR_OK
        res, ref = hb.register_batch_refine([], icp=icp)
        assert res == [] and ref == []
    finally:
        hb.close()


def test_raw_sweeps_are_refined_on_the_preprocessed_clouds():
    from quatro_amd import lib as ql
    from quatro_amd import synth
    tgt_T = TILT @ R.rigid(R.rot(0.0, 0.0, 0.3), [1.0, -0.5, 0.0])
    scans = [synth.kitti64_raw_scan(i)[0] for i in range(2)]
    pairs = [(sc, R.apply(tgt_T, sc), 7 + i) for i, sc in enumerate(scans)]
    hb = _handle(4)
    try:
        hb.set_batch_preprocess()
        res, refined = hb.register_batch_refine(pairs)
    finally:
        hb.close()
    for i, (r, g) in enumerate(zip(res, refined)):
        e0, e1 = R.rot_err_deg(r["T"], tgt_T), R.rot_err_deg(g["T"], tgt_T)
        print(f"raw pair {i}: {r['n_src']} / {r['n_tgt']} voxels, quatro {e0:.3f} deg -> icp {e1:.3f} deg")
        assert r["status"] == ql.QTR_OK and g["status"] == ql.QTR_OK and g["valid"], i
        assert e1 < e0, i
