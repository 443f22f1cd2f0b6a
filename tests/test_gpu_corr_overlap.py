"""qtr_register_pair_corr with its back end enqueued BESIDE the front end (third stream, the smaller k_hcore_async shape):
every record equals the serial order's (a handle created under QTR_CORR_OVERLAP=0) and the two calls qtr_feature_pair +
qtr_solve, bit for bit — on every back-end path by size, with stage events on and off, host and device correspondences,
QTR_HOST_WAIT=block, a front end that fails behind the back end's enqueue, the long-list round that re-enters the front
end, and what follows on the slot.  No timing is a pass condition."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from quatro_amd import lib as ql
from quatro_amd import synth

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=65536, max_voxels=16384, max_corr=8192)  # (tests/test_gpu_front_edges.py)
SMALL = dict(max_points=65536, max_voxels=1024, max_corr=8192)    # the handle that refuses the normal pair
LONG_LEAF = 0.01
# the empty back end, below any clique, the single-wave core path (no k_hcore_async), k_hcore_async's lower end (above
# hcore_min_l = 1280) and its full shape under the new cap
SIZES = (0, 2, 300, 1281, 5000)


def _moved(p, yaw, t, seed, sigma):
    q = p.copy()
    q[:, :3] = (p[:, :3].astype(np.float64) @ synth.yaw_matrix(yaw).T + np.asarray(t)).astype(np.float32)
    q[:, :3] += np.random.default_rng(seed).normal(0, sigma, (q.shape[0], 3)).astype(np.float32)
    return q


@pytest.fixture(scope="module")
def data():
    """The scan recipes of tests/test_gpu_front_edges.py (its `data` fixture checks them against the oracle): normal — a lidar
    pair of 10 k voxels; small — its points within 20 m; tiny — 250 points on a 0.8 m patch; long — 600 points in a 0.5 m
    cube, every point with more than QTR_KMAX neighbours at leaf 0.01."""
    s, t, _ = synth.kitti64_pair(1)
    near = lambda p: np.ascontiguousarray(p[np.linalg.norm(p[:, :3], axis=1) < 20.0])
    g = np.random.default_rng(3)
    g.uniform(0, 5.0, 2000), g.uniform(0, 5.0, 2000), g.normal(0, 0.01, 2000)  # (the `passing` pair's draws: tiny follows them)
    c = np.zeros((600, 4), dtype=np.float32)
    c[:, :3] = np.random.default_rng(5).uniform(0, 0.5, (600, 3))
    d = _moved(c, 0.2, (0.05, -0.03, 0.01), 11, 0.0005)
    e = np.zeros((250, 4), dtype=np.float32)
    e[:, 0], e[:, 1] = g.uniform(0, 0.8, 250), g.uniform(0, 0.8, 250)
    e[:, 2] = 0.1 * np.sin(5.0 * e[:, 0]) * np.cos(4.0 * e[:, 1]) + g.normal(0, 0.002, 250)
    f = _moved(e, 0.2, (0.05, -0.03, 0.01), 13, 0.0005)
    return {"normal": (s, t), "small": (near(s), near(t)), "long": (c, d), "tiny": (e, f)}


def _fp(kind):
    return ql.default_frontend_params(seed=2, voxel_size={"long": LONG_LEAF}.get(kind, 0.3))


def _corr(L, seed=7):
    if L == 0:
        z = np.zeros((0, 4), dtype=np.float32)
        return z, z.copy()
    return synth.correspondences(L, 0.05 if L >= 1000 else 0.1, seed, noise=0.1)[:2]


@contextlib.contextmanager
def _env(**kv):
    """environment variables the library reads at qtr_create, set around a handle's creation and restored afterwards"""
    keep = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(limits=LIMITS, overlap=True, events=True, block=False, **kw):
    with _env(QTR_CORR_OVERLAP=None if overlap else "0", QTR_STAGE_EVENTS=None if events else "0",
              QTR_HOST_WAIT="block" if block else None):
        return ql.Handle(0, **limits, **kw)


def _dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)) for a in arrays]
    torch.cuda.synchronize()
    return out


def _corr_call_dev(h, scans_dev, cs, ct, L, fp, slot=0, check=True):
    """qtr_register_pair_corr on device scans, device correspondences and device index lists -> (rc, Result, record)"""
    import torch
    s, t = scans_dev
    cap = max(L, 1)
    cl = torch.zeros(cap, dtype=torch.int32, device=s.device)
    fin = torch.zeros(cap, dtype=torch.int32, device=s.device)
    torch.cuda.synchronize()
    res, nm, prm = ql.Result(), C.c_int(), ql.demo_params()
    rc = h._lib.qtr_register_pair_corr(h._h, slot, s.data_ptr(), s.shape[0], t.data_ptr(), t.shape[0], C.byref(fp),
                                       cs.data_ptr() if L else None, ct.data_ptr() if L else None, L, C.byref(prm),
                                       C.byref(res), C.addressof(nm), cl.data_ptr(), fin.data_ptr(), cap, ql.MEM_DEVICE)
    if check:
        h._check(rc, ok=(ql.QTR_OK, ql.QTR_ERR_CLIQUE_TOO_SMALL))
    out = ql._result_dict(res, cl.cpu().numpy(), None, fin.cpu().numpy())
    out["n_matched"] = nm.value
    return rc, res, out


def _record(r):
    return (r["status"], r["valid"], r["clique"].size, r["final_inliers"].size, r["cost"], r["n_src"], r["n_tgt"], r["L"])


def _same(got, want):
    """the whole record, T bit for bit"""
    assert _record(got) == _record(want)
    assert np.array_equal(got["T"].view(np.uint64), want["T"].view(np.uint64))
    assert np.array_equal(got["clique"], want["clique"]) and np.array_equal(got["final_inliers"], want["final_inliers"])
    if "n_matched" in want:
        assert got["n_matched"] == want["n_matched"]


@pytest.fixture(scope="module")
def two_calls(data):
    """What the one call must return, from a third handle: qtr_feature_pair's counts and qtr_solve's record, per pair kind
    and per correspondence set (computed once, shared, never changed)."""
    h = _handle()
    try:
        front = {k: h.feature_pair(*data[k], _fp(k)) for k in ("small", "tiny", "long")}
        cache = {}

        def want(kind, L, seed=7):
            key = (kind, L, seed)
            if key not in cache:
                r = dict(h.solve(*_corr(L, seed)))
                r["n_src"], r["n_tgt"], r["n_matched"] = front[kind]["n_src"], front[kind]["n_tgt"], front[kind]["L"]
                cache[key] = r
            return cache[key]

        for L in SIZES:
            want("small", L)
        for kind in ("small", "tiny"):
            for L, seed in ((300, 11), (1281, 12)):
                want(kind, L, seed)
        want("long", 1500, 3)
        want("small", 700, 13)
        yield want
    finally:
        h.close()


@pytest.mark.parametrize("events,device_corr,block", [(True, False, False), (False, False, False), (True, True, False),
                                                      (False, True, False), (True, False, True)])
def test_overlapped_equals_serial_equals_two_calls(data, two_calls, events, device_corr, block):
    fp = _fp("small")
    pair = data["small"]
    scans_dev = _dev(*pair) if device_corr else None
    got = {}
    for overlap in (True, False):
        h = _handle(overlap=overlap, events=events, block=block)
        try:
            for L in SIZES:
                cs, ct = _corr(L)
                if device_corr:
                    dcs, dct = _dev(cs, ct)
                    got[overlap, L] = _corr_call_dev(h, scans_dev, dcs, dct, L, fp)[2]
                else:
                    got[overlap, L] = h.register_pair_corr(*pair, cs, ct, fp)
        finally:
            h.close()
    for L in SIZES:
        _same(got[True, L], two_calls("small", L))
        _same(got[False, L], two_calls("small", L))
        _same(got[True, L], got[False, L])


def test_nothing_stale_across_alternating_calls(data, two_calls):
    """eight calls on one slot: two correspondence sets of different size and two scan pairs in turn"""
    h = _handle()
    try:
        for i in range(8):
            kind = ("small", "tiny")[(i // 2) % 2]
            L, seed = ((300, 11), (1281, 12))[i % 2]
            cs, ct = _corr(L, seed)
            _same(h.register_pair_corr(*data[kind], cs, ct, _fp(kind)), two_calls(kind, L, seed))
    finally:
        h.close()


def test_front_end_that_fails_behind_the_back_ends_enqueue(data, two_calls):
    """max_voxels = 1024 refuses the normal pair AFTER the voxel stage, when the back end of 1281 device correspondences is
    on its way: the record is the serial order's (counts and status, nothing of the solver), the correspondences may be
    overwritten on return, and the slot's next call is not touched by the abandoned chain."""
    import torch
    fp = _fp("normal")
    scans = _dev(*data["normal"])
    refused = {}
    for overlap in (True, False):
        h = _handle(SMALL, overlap=overlap)
        try:
            dcs, dct = _dev(*_corr(1281, 12))
            rc, res, rec = _corr_call_dev(h, scans, dcs, dct, 1281, fp, check=False)
            dcs.zero_(), dct.zero_()
            torch.cuda.synchronize()
            assert rc == ql.QTR_ERR_CAPACITY and "max_voxels" in h.last_error()
            assert (res.status, res.n_corr, res.valid, res.n_clique, res.n_final, res.n_rot_inliers, res.max_core, res.n_edges) == \
                (ql.QTR_ERR_CAPACITY, 1281, 0, 0, 0, 0, 0, 0)
            assert not np.any(rec["T"]) and rec["cost"] == 0
            refused[overlap] = bytes(res)
            cs, ct = _corr(700, 13)
            _same(h.register_pair_corr(*data["small"], cs, ct, _fp("small")), two_calls("small", 700, 13))
        finally:
            h.close()
    assert refused[True] == refused[False]


def test_long_list_round_with_the_back_end_in_flight(data, two_calls):
    """a fresh handle meets a cloud with lists longer than QTR_KMAX: the front end goes round again, the back end does not"""
    fp = _fp("long")
    cs, ct = _corr(1500, 3)
    ref = _handle()
    try:
        matched = ref.register_pair(*data["long"], fp)["L"]
    finally:
        ref.close()
    want = two_calls("long", 1500, 3)
    assert want["n_matched"] == matched
    h = _handle()
    try:
        first = h.register_pair_corr(*data["long"], cs, ct, fp)
        second = h.register_pair_corr(*data["long"], cs, ct, fp)
    finally:
        h.close()
    _same(first, want)
    _same(second, want)


def test_what_follows_on_the_slot(data, two_calls):
    """qtr_refine_pair is ordered on the slot's stream: it sees the finished back end (its guess is that call's T) — the
    same record as under the serial order, with another slot's call in between."""
    fp = _fp("small")
    scans = _dev(*data["small"])
    tiny = _dev(*data["tiny"])
    refined, other = {}, {}
    for overlap in (True, False):
        h = _handle(overlap=overlap, n_slots=2)
        try:
            dcs, dct = _dev(*_corr(1281, 12))
            rec = _corr_call_dev(h, scans, dcs, dct, 1281, fp, slot=0)[2]
            _same(rec, two_calls("small", 1281, 12))
            d2s, d2t = _dev(*_corr(300, 11))
            other[overlap] = _corr_call_dev(h, tiny, d2s, d2t, 300, _fp("tiny"), slot=1)[2]
            refined[overlap] = h.refine_pair(slot=0)
        finally:
            h.close()
        _same(other[overlap], two_calls("tiny", 300, 11))
    assert refined[True].keys() == refined[False].keys()
    for k in refined[True]:
        assert np.array_equal(np.asarray(refined[True][k]), np.asarray(refined[False][k])), k


def test_stage_times_of_the_overlapped_call(data):
    h = _handle(events=True)
    try:
        h.register_pair_corr(*data["small"], *_corr(1281), _fp("small"))
        st = h.stage_times()
    finally:
        h.close()
    for k in ("graph", "clique", "solve", "total"):
        assert np.isfinite(st[k]) and st[k] > 0, (k, st)
    assert st["total"] >= max(st[k] for k in ("voxelize", "fpfh", "match", "graph", "clique", "solve")), st


@pytest.mark.parametrize("host_corr", [False, True])
def test_back_end_is_ordered_behind_the_slots_earlier_work(data, host_corr):
    """qtr_feature_pair with device outputs returns without synchronising: its keypoint copies are still queued on the slot's
    stream.  qtr_register_pair_corr right behind it, no synchronisation in between — on those very buffers as device
    correspondences (the back end must see the finished copies), or on host correspondences (their staging into the slot's
    matched-cloud buffers must not overtake the copies out of them)."""
    import torch
    fp = _fp("small")
    ref = _handle()
    try:
        front = ref.feature_pair(*data["small"], fp)
        L = front["L"]
        assert L > 2
        want_kps = ref.solve(front["src_kps"], front["tgt_kps"])
        other = _corr(1281, 12)
        want_other = ref.solve(*other)
    finally:
        ref.close()
    dev = torch.device("cuda", 0)
    s, t = _dev(*data["small"])
    for overlap in (True, False):
        h = _handle(overlap=overlap)
        try:
            for rep in range(3):
                cap = int(h.limits.max_corr)
                sk = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
                tk = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
                cl = torch.zeros(cap, dtype=torch.int32, device=dev)
                fin = torch.zeros(cap, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ns, nt, Lg = C.c_int(), C.c_int(), C.c_int()
                res, nm, prm = ql.Result(), C.c_int(), ql.demo_params()
                h._check(h._lib.qtr_feature_pair(h._h, 0, s.data_ptr(), s.shape[0], t.data_ptr(), t.shape[0], C.byref(fp),
                                                 C.byref(ns), C.byref(nt), C.byref(Lg), sk.data_ptr(), tk.data_ptr(), None, cap,
                                                 ql.MEM_DEVICE))
                assert Lg.value == L
                if host_corr:
                    got = h.register_pair_corr(*data["small"], *other, fp)
                    want = want_other
                else:
                    rc = h._lib.qtr_register_pair_corr(h._h, 0, s.data_ptr(), s.shape[0], t.data_ptr(), t.shape[0], C.byref(fp),
                                                       sk.data_ptr(), tk.data_ptr(), L, C.byref(prm), C.byref(res),
                                                       C.addressof(nm), cl.data_ptr(), fin.data_ptr(), cap, ql.MEM_DEVICE)
                    h._check(rc, ok=(ql.QTR_OK, ql.QTR_ERR_CLIQUE_TOO_SMALL))
                    got = ql._result_dict(res, cl.cpu().numpy(), None, fin.cpu().numpy())
                    want = want_kps
                torch.cuda.synchronize()
                assert np.array_equal(sk[:L].cpu().numpy(), front["src_kps"]) and np.array_equal(tk[:L].cpu().numpy(), front["tgt_kps"])
                assert (got["status"], got["valid"], got["L"], got["cost"]) == (want["status"], want["valid"], want["L"], want["cost"])
                assert np.array_equal(got["T"].view(np.uint64), want["T"].view(np.uint64))
                assert np.array_equal(got["clique"], want["clique"]) and np.array_equal(got["final_inliers"], want["final_inliers"])
        finally:
            h.close()


def test_stage_times_of_the_serial_order_are_one_chain(data):
    """under QTR_CORR_OVERLAP=0 the call's events follow one another on one stream (the matcher's end is recorded for a
    call with given correspondences too): every stage is measured and the stages add up to the total — consecutive
    differences of one clock, so the tolerance is float rounding of seven sub-millisecond values (1e-3 ms is generous)"""
    h = _handle(overlap=False, events=True)
    try:
        h.register_pair(*data["tiny"], _fp("tiny"))  # (leaves an older ev[7] behind: the next call must record its own)
        h.register_pair_corr(*data["small"], *_corr(1281), _fp("small"))
        st = h.stage_times()
    finally:
        h.close()
    stages = ("voxelize", "fpfh", "match", "graph", "clique", "solve")
    for k in stages + ("total",):
        assert np.isfinite(st[k]) and st[k] > 0, (k, st)
    assert abs(sum(st[k] for k in stages) - st["total"]) < 1e-3, st
