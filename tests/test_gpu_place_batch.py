"""The grouped place query on the MI355X, through the C ABI of libquatro_ext.so: every row of a batch equal, as raw records,
to the restatement (tests/place_batch_restate.py over tests/place_restate.py) AND to the single calls; every score of every
range; the contract's edges; retrieval, api.find_loops and api.close_loops on the twelve revisits; the C++ demo."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import place_batch_restate as pb
import place_restate as pr

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 1


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _hi(hi):
    return BIG if hi is None else hi


def single(h, ix, src, k, lo, hi, slot=0):
    """The single call's records for a source: a Keyframe -> qtr_place_query, a descriptor -> qtr_place_query_desc."""
    from quatro_amd import lib as ql
    out, n = np.zeros(64, dtype=ql.PLACE_MATCH_DTYPE), C.c_int(-1)
    po = out.ctypes.data_as(C.POINTER(ql.PlaceMatch))
    if isinstance(src, ql.Keyframe):
        h._check(h._lib.qtr_place_query(h._h, slot, ix._ix, src._kf, lo, _hi(hi), k, po, C.byref(n)))
    else:
        ptr, mem = ql._ptr(src)
        h._check(h._lib.qtr_place_query_desc(h._h, slot, ix._ix, ptr, mem, lo, _hi(hi), k, po, C.byref(n)))
    return out[:n.value].copy()


class Case:
    """Items of a batch with, per item, the descriptor behind it (for the restatement) and the source of its single call."""

    def __init__(self):
        self.items, self.descs, self.singles, self.ranges = [], [], [], []

    def add(self, item, desc, single_src, rng):
        self.items.append((item, rng))
        self.descs.append(desc)
        self.singles.append(single_src)
        self.ranges.append((rng[0], _hi(rng[1])))


def check_batch(h, ix, E, case, k, slot=0, scores=False, memo=None):
    """One query_batch against the restatement and the single calls, raw records; with `scores` every DIST / SHIFT too."""
    from quatro_amd import lib as ql
    got, n = ix.query_batch(case.items, k, slot=slot, raw=True)
    want, wn = pb.query_batch(case.descs, case.ranges, E, k) if memo is None else memo
    assert np.array_equal(n, wn), (n, wn)
    assert np.array_equal(raw(got), raw(want))
    seen = {}
    for q, (src, (lo, hi)) in enumerate(zip(case.singles, case.ranges)):
        key = (id(src), lo, hi)
        if key not in seen:
            seen[key] = single(h, ix, src, k, lo, hi, slot)
        assert n[q] == len(seen[key]) and np.array_equal(raw(got[q, :n[q]]), raw(seen[key])), q
    if scores:
        for q, (d, rng) in enumerate(zip(case.descs, case.ranges)):
            wd, ws = pb.scores(d, rng, E)
            gd, gs = ix.batch_fetch(q, ql.PLACE_BATCH_DIST, slot), ix.batch_fetch(q, ql.PLACE_BATCH_SHIFT, slot)
            assert gd.dtype == np.float32 and gs.dtype == np.int32 and len(gd) == len(gs) == len(wd), q
            assert np.array_equal(raw(gd), raw(wd.astype(np.float32))) and np.array_equal(gs, ws), q
    return got, n


@pytest.fixture(scope="module")
def six(hip):
    """Six synthetic scans as keyframes, with their voxels."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    scans = [s for k in range(3) for s in synth.kitti64_pair(k)[:2]]
    kfs = [hip.keyframe(s) for s in scans]
    vox = [kf.fetch(ql.KF_VOX) for kf in kfs]
    yield kfs, vox
    for kf in kfs:
        kf.close()


@pytest.fixture(scope="module")
def mixture(hip, six):
    """20 x 60: an index of 23 entries — six keyframes, one all-zero descriptor (6), two identical entries (7, 15), one entry
    that is entry 2 turned by 11 sectors (9), the rest entries scaled ring by ring and rolled — and a second index of 3."""
    kfs, vox = six
    rng = np.random.default_rng(7)
    ix, ix2 = hip.place_index(32), hip.place_index(4)
    for kf in kfs:
        ix.add(kf)
    base = [ix.fetch(i) for i in range(6)]
    while len(ix) < 23:
        i = len(ix)
        if i == 6:
            d = np.zeros((20, 60), np.float32)
        elif i == 9:
            d = np.roll(base[2], 11, axis=1)
        elif i == 15:
            d = ix.fetch(7)
        else:
            d = (np.roll(base[i % 6], int(rng.integers(60)), axis=1) * rng.uniform(0.5, 1.5, (20, 1))).astype(np.float32)
        assert ix.add_desc(np.ascontiguousarray(d)) == i
    E = np.stack([ix.fetch(i) for i in range(23)])
    for j in (4, 9, 21):
        ix2.add_desc(np.ascontiguousarray(np.roll(E[j], 3, axis=1)))
    E2 = np.stack([ix2.fetch(i) for i in range(3)])
    kf_desc = [pr.describe(v) for v in vox]
    yield ix, E, ix2, E2, kf_desc
    ix.close()
    ix2.close()


RANGES = [(0, None), (5, 5), (-5, 10 ** 6), (1, 4), (17, 22), (3, 4), (5, 8), (9, 13), (14, 19), (22, 40), (30, 50)]


def _mixture_case(hip, six, mixture, Q, salt=0):
    """Q items: the five kinds in turn, the ranges in another rhythm."""
    import torch
    kfs, _ = six
    ix, E, ix2, E2, kf_desc = mixture
    rng = np.random.default_rng(100 + Q)
    case = Case()
    case.keep = []
    for q in range(Q):
        r = RANGES[(3 * q + Q + salt) % len(RANGES)]
        kind = q % 5
        if kind == 0:
            i = (q // 5) % 6
            case.add(kfs[i], kf_desc[i], kfs[i], r)
        elif kind == 1:
            d = np.ascontiguousarray(np.roll(E[(q * 5) % 23], q % 60, axis=1) * rng.uniform(0.7, 1.3, (20, 1)), dtype=np.float32)
            case.add(d, d, d, r)
        elif kind == 2:
            d = np.ascontiguousarray(np.roll(E[(q * 3) % 23], (7 * q) % 60, axis=1))
            t = torch.from_numpy(d).cuda().contiguous()
            case.keep.append(t)
            case.add(t, d, t, r)
        elif kind == 3:
            i = (q * 2) % 23
            case.add(i, E[i], np.ascontiguousarray(E[i]), r)
        else:
            i = q % 3
            case.add((ix2, i), E2[i], np.ascontiguousarray(E2[i]), r)
    return case


def test_mixture_of_kinds_ranges_and_k_equals_restatement_and_single_calls(hip, six, mixture):
    ix, E = mixture[0], mixture[1]
    QT = pb.qt(pb.stride(20, 60))
    assert QT == 2
    for Q in (1, QT - 1, QT, QT + 1, 2 * QT + 1, 19):
        case = _mixture_case(hip, six, mixture, Q)
        for k in (1, 10, 64):
            check_batch(hip, ix, E, case, k, scores=(k == 10))
    # all five kinds with every range, the union holed ((1, 4) and (17, 22) alone leave 4 .. 16 unasked)
    for salt in range(1, len(RANGES)):
        check_batch(hip, ix, E, _mixture_case(hip, six, mixture, 5, salt), 10, scores=True)
    holed = Case()
    holed.add(3, E[3], np.ascontiguousarray(E[3]), (1, 4))
    holed.add(20, E[20], np.ascontiguousarray(E[20]), (17, 22))
    holed.add(6, E[6], np.ascontiguousarray(E[6]), (0, None))  # the all-zero descriptor: distance 1 to everything
    holed.add(7, E[7], np.ascontiguousarray(E[7]), (0, None))  # the twins 7 and 15 tie at 0, ordered by id
    holed.add(2, E[2], np.ascontiguousarray(E[2]), (9, 10))    # entry 9 is entry 2 turned by 11 sectors
    got, n = check_batch(hip, ix, E, holed, 5, scores=True)
    assert list(n) == [3, 5, 5, 5, 1]
    assert all(got[2, r]["distance"] == 1.0 and got[2, r]["id"] == r for r in range(5))
    assert [int(got[3, r]["id"]) for r in range(2)] == [7, 15] and got[3, 0]["distance"] == 0 and got[3, 1]["distance"] == 0
    assert got[4, 0]["id"] == 9 and got[4, 0]["distance"] == 0 and got[4, 0]["shift"] == 11
    # every range empty: nothing runs, every count is 0
    empty = Case()
    for q in range(3):
        empty.add(q, E[q], np.ascontiguousarray(E[q]), (5 + q, 5))
    got, n = ix.query_batch(empty.items, 4, raw=True)
    assert not n.any() and not raw(got).any()
    assert ix.query_batch([], 4) == []


@pytest.mark.parametrize("R,S", [(32, 64), (4, 8), (9, 13)])
def test_other_shapes_with_one_query_more_than_a_tile(hip, six, R, S):
    from quatro_amd import lib as ql
    kfs, vox = six
    p = ql.default_place_params(num_rings=R, num_sectors=S, max_range=60.0, height_offset=1.5)
    Q = pb.qt(pb.stride(R, S)) + 1
    assert Q == 3
    rng = np.random.default_rng(R * 100 + S)
    with hip.place_index(8, p) as ix:
        for kf in kfs:
            ix.add(kf)
        kd = [pr.describe(v, R, S, 60.0, 1.5) for v in vox]
        ix.add_desc(np.ascontiguousarray(np.roll(kd[1], 3, axis=1)))
        ix.add_desc(np.ascontiguousarray(kd[4] * rng.uniform(0.5, 1.5, (R, 1)), dtype=np.float32))
        E = np.stack([ix.fetch(i) for i in range(8)])
        assert all(np.array_equal(raw(E[i]), raw(kd[i])) for i in range(6))
        case = Case()
        ranges = [(0, None), (1, 6), (3, 4), (2, 8), (5, 5)]
        for q in range(Q):
            r = ranges[q % len(ranges)]
            if q % 3 == 0:
                case.add(kfs[q % 6], kd[q % 6], kfs[q % 6], r)
            elif q % 3 == 1:
                case.add(q % 8, E[q % 8], np.ascontiguousarray(E[q % 8]), r)
            else:
                d = np.ascontiguousarray(np.roll(E[q % 8], q % S, axis=1) * rng.uniform(0.8, 1.2, (R, 1)), dtype=np.float32)
                case.add(d, d, d, r)
        check_batch(hip, ix, E, case, 8, scores=True)


@pytest.fixture(scope="module")
def long48(hip):
    """4 x 8: an index of 65 537 entries, one more than 1024 queries may search at once."""
    from quatro_amd import lib as ql
    N = ql.PLACE_BATCH_MAX_PAIRS // ql.PLACE_BATCH_MAX + 1
    rng = np.random.default_rng(48)
    E = rng.uniform(0.1, 4.0, (N, 4, 8)).astype(np.float32)
    E[rng.random((N, 4, 8)) < 0.2] = 0.0
    p = ql.default_place_params(num_rings=4, num_sectors=8)
    ix = hip.place_index(N, p)
    add, ident = hip._lib.qtr_place_index_add_desc, C.c_int(-1)
    for i in range(N):
        assert add(hip._h, 0, ix._ix, E[i].ctypes.data, ql.MEM_HOST, C.byref(ident)) == 0
    assert len(ix) == N == 65537
    yield ix, E
    ix.close()


def test_a_union_range_past_one_pass_of_the_score_grid(hip, long48):
    ix, E = long48
    n = 4 * pb.GRID_X + 5  # one pass covers 4 entries per workgroup
    assert n == 8197
    rng = np.random.default_rng(3)
    case = Case()
    d = np.ascontiguousarray(E[100] * rng.uniform(0.9, 1.1, (4, 1)), dtype=np.float32)
    case.add(d, d, d, (0, n))
    case.add(8190, E[8190], np.ascontiguousarray(E[8190]), (8188, n))
    case.add(5, E[5], np.ascontiguousarray(E[5]), (3, n - 2))
    got, cnt = check_batch(hip, ix, E[:n], case, 10, scores=True)
    assert list(cnt) == [10, 9, 10] and got[1, 0]["id"] == 8190 and got[2, 0]["id"] == 5


def test_1024_queries_in_one_call_and_1025_refused(hip, mixture):
    from quatro_amd import lib as ql
    ix, E = mixture[0], mixture[1]
    rng = np.random.default_rng(1024)
    host = [np.ascontiguousarray(E[i] * rng.uniform(0.8, 1.2, (20, 1)), dtype=np.float32) for i in range(4)]
    case = Case()
    for q in range(1024):
        r = (0, 16) if q % 2 == 0 else (3, 11)
        if q % 8 == 7:
            d = host[(q // 8) % 4]
            case.add(d, d, d, r)
        else:
            i = (q // 2) % 16
            case.add(i, E[i], case.singles[q - 32] if q >= 32 else np.ascontiguousarray(E[i]), r)
    memo, want = {}, np.zeros((1024, 10), dtype=pb.MATCH_DTYPE)
    wn = np.zeros(1024, np.int32)
    for q in range(1024):
        key = (id(case.singles[q]), case.ranges[q])
        if key not in memo:
            memo[key] = pb.query_batch([case.descs[q]], [case.ranges[q]], E, 10)
        want[q], wn[q] = memo[key][0][0], memo[key][1][0]
    assert len(memo) <= 40
    got, n = check_batch(hip, ix, E, case, 10, memo=(want, wn))
    assert list(n[:2]) == [10, 8]
    more = case.items + [case.items[0]]
    with pytest.raises(ql.QuatroHipError) as e:
        ix.query_batch(more, 10)
    assert e.value.code == ql.QTR_ERR_BAD_ARG and "1025" in str(e.value)


@pytest.fixture(scope="module")
def h2():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


def _items(*its):
    from quatro_amd import lib as ql
    return (ql.PlaceQueryItem * len(its))(*its)


def _item(kf=None, desc=None, frm=None, entry=-1, mem=0, lo=0, hi=BIG):
    from quatro_amd import lib as ql
    it = ql.PlaceQueryItem()
    it.kf, it.desc, it.from_, it.entry, it.mem, it.id_lo, it.id_hi = kf, desc, frm, entry, mem, lo, hi
    return it


def test_every_refusal_leaves_the_outputs_as_the_contract_says(hip, h2, six, mixture, long48):
    from quatro_amd import lib as ql
    kfs, vox = six
    ix, E, ix2 = mixture[0], mixture[1], mixture[2]
    lib2, bad = ql.load_ext(), ql.QTR_ERR_BAD_ARG
    d0 = np.ascontiguousarray(E[0])
    good = _item(entry=1)

    def call(h, index, items, Q, k, want, out_null=False, n_null=False, n_items=None):
        out = np.full((max(Q, 1) * 64,), 0x5A, np.uint8).repeat(16)  # (room for Q x 64 records)
        n = np.full(max(Q, 1), 7, np.int32)
        rc = lib2.qtr_place_query_batch(h._h, 0, index, items, Q, k, None if out_null else out.ctypes.data,
                                        None if n_null else n.ctypes.data)
        assert rc == want, (rc, want, h.last_error())
        assert (out == 0x5A).all()  # `out` is untouched
        if Q > 0 and not n_null:
            assert not n.any()  # every n_out[q] is 0
        return h.last_error()

    with h2.keyframe(np.ascontiguousarray(vox[0])) as foreign_kf, h2.place_index(2) as foreign_ix, \
            hip.place_index(2, ql.default_place_params(num_rings=20, num_sectors=59)) as other_shape:
        foreign_ix.add_desc(d0)
        other_shape.add_desc(np.ones((20, 59), np.float32))
        two = _items(good, _item(entry=2))
        assert lib2.qtr_place_query_batch(hip._h, 0, ix._ix, two, 0, 5, None, None) == ql.QTR_OK  # Q == 0
        call(hip, ix._ix, two, -1, 5, bad)
        big = (ql.PlaceQueryItem * 1025)(*([good] * 1025))
        assert "1025" in call(hip, ix._ix, big, 1025, 5, bad)
        for k in (0, -1, 65):
            call(hip, ix._ix, two, 2, k, bad)
        call(hip, None, two, 2, 5, bad)
        call(hip, ix._ix, None, 2, 5, bad)
        call(hip, ix._ix, two, 2, 5, bad, out_null=True)
        call(hip, ix._ix, two, 2, 5, bad, n_null=True)
        assert lib2.qtr_place_query_batch(hip._h, 3, ix._ix, two, 2, 5, None, None) == bad  # a bad slot
        assert "item 1" in call(hip, ix._ix, _items(good, _item(desc=d0.ctypes.data, mem=7)), 2, 5, bad)  # a bad mem
        assert "no source" in call(hip, ix._ix, _items(good, _item()), 2, 5, bad)  # an item with no source
        call(hip, ix._ix, _items(good, _item(entry=23)), 2, 5, bad)  # entry outside the searched index
        call(hip, ix._ix, _items(good, _item(frm=ix2._ix, entry=3)), 2, 5, bad)  # ... outside its own index
        call(hip, ix._ix, _items(good, _item(frm=ix2._ix, entry=-1)), 2, 5, bad)
        assert "another handle" in call(hip, ix._ix, _items(good, _item(kf=foreign_kf._kf)), 2, 5, bad)
        assert "another handle" in call(h2, ix._ix, two, 2, 5, bad)  # this index through another handle
        assert "another handle" in call(hip, ix._ix, _items(good, _item(frm=foreign_ix._ix, entry=0)), 2, 5, bad)
        assert "20 x 59" in call(hip, ix._ix, _items(good, _item(frm=other_shape._ix, entry=0)), 2, 5, bad)
    # 1024 queries x 65 537 entries: one pair too many; 1023 of them, or one entry fewer, would be within the cap
    lix = long48[0]
    many = (ql.PlaceQueryItem * 1024)(*([_item(entry=0, hi=8)] * 1023 + [_item(entry=1)]))
    msg = call(hip, lix._ix, many, 1024, 5, ql.QTR_ERR_CAPACITY)
    assert "65537" in msg and str(1 << 26) in msg
    # after all that the index answers as before
    assert [m["id"] for m in ix.query_batch([(7, (0, None))], 2)[0]] == [7, 15]


def test_a_single_query_gives_the_same_bytes_before_and_after_a_batch(hip, six, mixture):
    kfs, _ = six
    ix, E = mixture[0], mixture[1]
    d = np.ascontiguousarray(E[11])
    before = [single(hip, ix, kfs[3], 10, 0, None), single(hip, ix, d, 64, 2, 21)]
    case = _mixture_case(hip, six, mixture, 12)
    ix.query_batch(case.items, 7)
    after = [single(hip, ix, kfs[3], 10, 0, None), single(hip, ix, d, 64, 2, 21)]
    assert all(np.array_equal(raw(a), raw(b)) and len(a) for a, b in zip(before, after))
    # and the slot's last batch is still served after the single queries
    wd, ws = pb.scores(case.descs[4], case.ranges[4], E)
    assert np.array_equal(raw(ix.batch_fetch(4)), raw(wd)) and np.array_equal(ix.batch_fetch(4, 2), ws)
    from quatro_amd import lib as ql
    for q, what in ((-1, 1), (12, 1), (0, 0), (0, 3)):
        with pytest.raises(ql.QuatroHipError):
            ix.batch_fetch(q, what)


def test_two_threads_batch_from_two_slots_against_one_index(h2, mixture):
    E = mixture[1]
    rng = np.random.default_rng(22)
    with h2.place_index(40) as ix:
        for i in range(40):
            ix.add_desc(np.ascontiguousarray(np.roll(E[i % 23], i // 23 * 9, axis=1) * rng.uniform(0.5, 1.5, (20, 1)), dtype=np.float32))
        from quatro_amd import lib as ql
        with pytest.raises(ql.QuatroHipError):
            ix.batch_fetch(0, slot=1)  # no batch has run on that slot
        items = [[(i, (t, 40 - 3 * t)) for i in range(t, 40, 2)] + [(np.ascontiguousarray(E[5 + t]), (0, None))] for t in range(2)]
        seq = [ix.query_batch(items[t], 6 + t, slot=t, raw=True) for t in range(2)]
        out = [[None] * 6, [None] * 6]

        def work(t):
            for r in range(6):
                out[t][r] = ix.query_batch(items[t], 6 + t, slot=t, raw=True)

        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        for t in range(2):
            assert seq[t][1].all()
            for r in range(6):
                assert np.array_equal(raw(out[t][r][0]), raw(seq[t][0])) and np.array_equal(out[t][r][1], seq[t][1]), (t, r)


def test_destroying_the_handle_frees_a_used_batch_arena():
    import torch
    from quatro_amd import lib as ql
    torch.cuda.synchronize()
    h = ql.Handle(0)
    h.close()
    free0, _ = torch.cuda.mem_get_info()
    h = ql.Handle(0)
    ix = h.place_index(4)
    ix.add_desc(np.ones((20, 60), dtype=np.float32))
    d = np.ones((20, 60), dtype=np.float32)
    got, n = ix.query_batch([d] * 1024, 3, raw=True)  # 1024 slots of 5040 bytes, their table and records: over 5 MB
    assert n.tolist() == [1] * 1024 and not got["distance"].any()
    h.close()  # (neither the index nor the arena was released by hand)
    free1, _ = torch.cuda.mem_get_info()
    assert free1 >= free0 - (2 << 20), (free0, free1)


@pytest.fixture(scope="module")
def revisits(hip):
    """tests/test_gpu_place.py's twelve scenes: the SOURCE scans of kitti64_pair(k, max_xy=2.0) and their revisits, the
    TARGET scans; one index holds the 12 scenes followed by the 12 revisits."""
    from quatro_amd import synth
    pairs = [synth.kitti64_pair(k, max_xy=2.0) for k in range(12)]
    src = [hip.keyframe(p[0]) for p in pairs]
    tgt = [hip.keyframe(p[1]) for p in pairs]
    ix = hip.place_index(24)
    for kf in src + tgt:
        ix.add(kf)
    yield src, tgt, ix
    ix.close()
    for kf in src + tgt:
        kf.close()


def test_twelve_revisits_as_one_batch_and_find_loops(hip, revisits):
    from quatro_amd import api
    src, tgt, ix = revisits
    got, n = ix.query_batch([(kf, (0, 12)) for kf in tgt], 3, raw=True)
    for k in range(12):
        one = single(hip, ix, tgt[k], 3, 0, 12)
        assert n[k] == 3 and np.array_equal(raw(got[k]), raw(one)), k
        assert got[k, 0]["id"] == k
    loops = api.find_loops(ix, 12, 2)
    assert len(loops) == 24 and all(m == [] for m in loops[:12])
    for k in range(12):
        i = 12 + k  # the revisit of scene k asks the entries [0, k]: scene k is the last of them
        d = np.ascontiguousarray(ix.fetch(i))
        one = single(hip, ix, d, 2, 0, k + 1)
        assert [(m["id"], m["shift"]) for m in loops[i]] == [(int(r["id"]), int(r["shift"])) for r in one]
        assert [raw(np.float32(m["distance"])).tolist() for m in loops[i]] == [raw(r["distance"]).tolist() for r in one]
        assert loops[i][0]["id"] == k, (k, loops[i])
    near = api.find_loops(ix, 12, 2, max_distance=0.4, first=12)
    assert len(near) == 12 and all(m["distance"] <= 0.4 for ms in near for m in ms)
    assert all([m["id"] for m in near[k]] == [m["id"] for m in loops[12 + k] if m["distance"] <= 0.4] for k in range(12))


def test_close_loops_equals_three_close_loop_calls(hip, revisits):
    from quatro_amd import api
    from quatro_amd import lib as ql
    src, tgt, ix = revisits
    fp = ql.default_frontend_params(seed=0)
    qs = [tgt[1], tgt[6], tgt[10]]
    got = api.close_loops(hip, ix, src, qs, 2, id_hi=12, fp=fp)
    assert len(got) == 3
    for g, q in zip(got, qs):
        one = api.close_loop(hip, ix, src, q, 2, id_hi=12, fp=fp)
        assert [(m["id"], m["shift"]) for m in g["matches"]] == [(m["id"], m["shift"]) for m in one["matches"]]
        assert (g["best"], g["best_id"]) == (one["best"], one["best_id"]) and len(g["records"]) == len(one["records"]) == 2
        for a, b in zip(g["records"], one["records"]):
            assert a["status"] == b["status"] and a["valid"] == b["valid"]
            assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64))
            assert np.array_equal(a["clique"], b["clique"]) and np.array_equal(a["final_inliers"], b["final_inliers"])
    assert [g["best_id"] for g in got] == [1, 6, 10]


def test_cpp_place_batch_demo_builds_links_and_runs(hip, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    assert os.path.dirname(qbuild.build_ext(force=False, verbose=False)) == os.path.dirname(libpath)
    exe = str(tmp_path / "place_batch_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "place_batch_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-lquatro_ext", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    scans = [synth.kitti64_pair(k, max_xy=2.0)[1] for k in (3, 2)] + [synth.kitti64_pair(k, max_xy=2.0)[0] for k in (2, 3, 4)]
    files = []
    for k, sc in enumerate(scans):
        files.append(str(tmp_path / f"{k}.bin"))
        synth.save_kitti_bin(files[-1], sc)
    out = subprocess.run([exe, "2", "2"] + files, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    kfs = [hip.keyframe(ql.read_kitti_bin(f)) for f in files]
    try:
        with hip.place_index(3) as ix:
            for kf in kfs[2:]:
                ix.add(kf)
            want = []
            rows = [ix.query(kfs[0], 2), ix.query(kfs[1], 2), ix.query_desc(ix.fetch(0), 2, 1)]
            rows = [("query", q, ms) for q, ms in enumerate(rows)]
            rows += [("loop", i, ix.query_desc(ix.fetch(i), 2, 0, i)) for i in range(3)]
            for what, q, ms in rows:
                for r, m in enumerate(ms):
                    bits = int(np.float32(m["distance"]).view(np.uint32))
                    want.append(f"{what} {q} match {r} id {m['id']} shift {m['shift']} distance_bits {bits:08x}")
            assert out[:len(want)] == want and out[len(want):] == [""], out
            assert rows[0][2][0]["id"] == 1 and rows[1][2][0]["id"] == 0
    finally:
        for kf in kfs:
            kf.close()
