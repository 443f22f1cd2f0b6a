"""The grouped place query without a GPU: the header's two entry points against the extension library's symbol table,
binding and ctypes mirror; the host-side plan of include/qtr_place_batch_math.h compiled with g++ against its
Python mirror (tests/place_batch_restate.py); api.find_loops / api.close_loops over a fake index."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ext_abi
import place_batch_restate as pb

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TWO = {"qtr_place_query_batch", "qtr_place_batch_fetch"}


@pytest.fixture(scope="module")
def ref_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="place_batch_ref_"), "libplace_batch_ref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "place_batch_ref", "place_batch_ref.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.place_batch_ref_layout.restype = None
    lib.place_batch_ref_layout.argtypes = [ctypes.c_void_p]
    lib.place_batch_ref_clamp.restype = None
    lib.place_batch_ref_clamp.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.place_batch_ref_union.restype = None
    lib.place_batch_ref_union.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.place_batch_ref_slot.restype = ctypes.c_longlong
    return lib


def test_the_extension_library_exports_the_headers_two_names_and_the_mirrors_match_the_compiled_header(ref_lib):
    from quatro_amd import lib as ql
    assert ext_abi.check_header("quatro_place_batch.h") == TWO  # declared, listed, exported by libquatro_ext.so alone
    hip, _ = ext_abi.libraries()
    assert set(ql.PLACE_BATCH_EXPORTS) == TWO
    assert not (ext_abi.table(hip) & TWO) and not (set(ql.EXPORTS) & TWO)
    # the ctypes mirrors against sizeof / offsetof of the compiled header
    got = np.zeros(17, np.int32)
    ref_lib.place_batch_ref_layout(got.ctypes.data)
    I = ql.PlaceQueryItem
    assert list(got) == [ctypes.sizeof(I), I.kf.offset, I.desc.offset, I.from_.offset, I.entry.offset, I.mem.offset,
                         I.id_lo.offset, I.id_hi.offset, ctypes.sizeof(ql.PlaceMatch), ql.PLACE_BATCH_MAX,
                         ql.PLACE_BATCH_MAX_PAIRS, ql.PLACE_BATCH_DIST, ql.PLACE_BATCH_SHIFT, pb.QT_CAP, pb.LDS_BYTES, pb.GRID_X, 1]
    assert (int(got[0]), int(got[8]), int(got[9]), int(got[10])) == (40, 16, 1024, 1 << 26)
    assert ql.PLACE_MATCH_DTYPE == pb.MATCH_DTYPE and ql.PLACE_MATCH_DTYPE.itemsize == 16
    assert [ql.PLACE_MATCH_DTYPE.fields[n][1] for n, _ in ql.PlaceMatch._fields_] == [getattr(ql.PlaceMatch, n).offset
                                                                                     for n, _ in ql.PlaceMatch._fields_]


def test_the_query_tile_fits_the_lds_at_every_legal_shape(ref_lib):
    seen = set()
    for R in range(4, 33):
        for S in range(8, 65):
            st = pb.stride(R, S)
            assert ref_lib.place_batch_ref_stride(R, S) == st and st % 4 == 0 and st >= (R + 1) * S
            QT = ref_lib.place_batch_ref_qt(st)
            assert QT == pb.qt(st), (R, S)
            assert 1 <= QT <= pb.QT_CAP and (QT + 4) * st * 4 <= 65536
            assert QT == pb.QT_CAP or (QT + 5) * st * 4 > 65536  # the largest that fits, under the cap
            seen.add(QT)
    assert seen == {pb.QT_CAP} and pb.QT_CAP == 2  # (the cap binds everywhere: 32 x 64, the largest entry, would allow 3)
    assert 65536 // (pb.stride(32, 64) * 4) - 4 == 3 and 65536 // (pb.stride(20, 60) * 4) - 4 == 9


def _clamp(lib, lo, hi, size):
    out = np.zeros(2, np.int32)
    lib.place_batch_ref_clamp(lo, hi, size, out.ctypes.data)
    return int(out[0]), int(out[1])


def _union(lib, ranges):
    lo = np.array([a for a, _ in ranges] + [0], np.int32)
    hi = np.array([b for _, b in ranges] + [0], np.int32)
    out = np.full(2, -7, np.int32)
    lib.place_batch_ref_union(lo.ctypes.data, hi.ctypes.data, len(ranges), out.ctypes.data)
    return int(out[0]), int(out[1])


def test_ranges_are_clamped_and_united_as_the_mirror_says(ref_lib):
    big = 2 ** 31 - 1
    for lo, hi, size, want in [(0, big, 23, (0, 23)), (-5, 10 ** 6, 23, (0, 23)), (5, 5, 23, (0, 0)), (7, 3, 23, (0, 0)),
                               (30, 40, 23, (0, 0)), (22, 40, 23, (22, 23)), (-9, 0, 23, (0, 0)), (-9, 1, 23, (0, 1)),
                               (0, big, 0, (0, 0)), (3, 8, 23, (3, 8))]:
        assert _clamp(ref_lib, lo, hi, size) == pb.clamp(lo, hi, size) == want, (lo, hi, size)
    cases = [[], [(0, 0)], [(0, 0), (0, 0)], [(3, 8)], [(3, 5), (17, 21)], [(0, 0), (17, 21), (0, 0), (3, 5)],
             [(0, 23), (5, 6)], [(5, 6), (0, 0), (6, 7)], [(9, 10), (0, 1)], [(0, 0), (22, 23)]]
    want = [(0, 0), (0, 0), (0, 0), (3, 8), (3, 21), (3, 21), (0, 23), (5, 7), (0, 10), (22, 23)]
    for ranges, w in zip(cases, want):
        assert _union(ref_lib, ranges) == pb.union(ranges) == w, ranges
    rng = np.random.default_rng(2)
    for _ in range(200):
        size = int(rng.integers(0, 50))
        raw = [(int(rng.integers(-10, 60)), int(rng.integers(-10, 60))) for _ in range(int(rng.integers(1, 9)))]
        ranges = [pb.clamp(a, b, size) for a, b in raw]
        assert ranges == [_clamp(ref_lib, a, b, size) for a, b in raw]
        assert _union(ref_lib, ranges) == pb.union(ranges)
        ulo, uhi = pb.union(ranges)
        assert all(ulo <= a and b <= uhi for a, b in ranges if b > a) and 0 <= ulo <= uhi <= size


def test_the_pair_cap_on_both_sides_and_the_table_layout(ref_lib):
    cap = 1 << 26
    for Q, U in [(1024, 65536), (1024, 65537), (1023, 65600), (1, cap), (1, cap + 1), (2, cap // 2), (2, cap // 2 + 1), (0, 5),
                 (1024, 0), (1024, 2 ** 31 - 1), (1000, 67108), (1000, 67109)]:
        assert bool(ref_lib.place_batch_ref_pairs_ok(Q, U)) == pb.pairs_ok(Q, U) == (Q * U <= cap), (Q, U)
    assert pb.pairs_ok(1024, 65536) and not pb.pairs_ok(1024, 65537)
    # (q, e) -> q * U + (e - ulo), in 64 bits
    for q, e, ulo, U in [(0, 5, 5, 10), (3, 7, 5, 10), (1023, 65535 + 9, 9, 65536), (1, 2 ** 26 + 2, 3, 2 ** 26)]:
        assert ref_lib.place_batch_ref_slot(q, e, ulo, U) == q * U + (e - ulo)


class FakeIndex:
    """What api.find_loops / close_loops use of a PlaceIndex: len() and query_batch.  Entry i sits at position i on a line,
    the distance of two entries is |i - j| / 100."""

    def __init__(self, size):
        self.size, self.calls = size, []

    def __len__(self):
        return self.size

    def query_batch(self, items, k):
        self.calls.append(list(items))
        out = []
        for src, (lo, hi) in items:
            at = src if isinstance(src, int) else src.at
            lo, hi = pb.clamp(lo, 2 ** 31 - 1 if hi is None else hi, self.size)
            ids = sorted(range(lo, hi), key=lambda j: (abs(at - j), j))[:k]
            out.append([{"id": j, "shift": 0, "distance": np.float32(abs(at - j) / 100.0), "yaw": 0.0} for j in ids])
        return out


def test_find_loops_ranges_chunks_and_filter(monkeypatch):
    from quatro_amd import api
    from quatro_amd import lib as ql
    ix = FakeIndex(40)
    got = api.find_loops(ix, 10, 3)
    assert len(ix.calls) == 1 and [src for src, _ in ix.calls[0]] == list(range(40))
    assert [rng for _, rng in ix.calls[0]] == [(0, i - 10 + 1) for i in range(40)]  # the entries [0, i - min_gap]
    assert len(got) == 40 and all(g == [] for g in got[:10])
    assert [m["id"] for m in got[10]] == [0] and [m["id"] for m in got[25]] == [15, 14, 13]
    # first / last
    ix = FakeIndex(40)
    got = api.find_loops(ix, 10, 3, first=20, last=23)
    assert [src for src, _ in ix.calls[0]] == [20, 21, 22] and [[m["id"] for m in g] for g in got] == [[10, 9, 8], [11, 10, 9],
                                                                                                    [12, 11, 10]]
    assert api.find_loops(FakeIndex(40), 10, 3, first=38, last=99)[1][0]["id"] == 29
    # max_distance filters on the host: entry 25's matches are at 0.10, 0.11, 0.12
    assert [[m["id"] for m in g] for g in api.find_loops(FakeIndex(40), 10, 3, max_distance=0.11, first=25, last=26)] == [[15, 14]]
    assert api.find_loops(FakeIndex(40), 10, 3, max_distance=0.05, first=25, last=26) == [[]]
    # both caps hold in every chunk, every entry is asked once and in order
    for q_cap, pair_cap, size, gap in [(7, 1 << 26, 40, 10), (1024, 150, 40, 10), (5, 60, 40, 0), (1024, 1 << 26, 40, 10),
                                       (16, 64, 33, 3)]:
        monkeypatch.setattr(ql, "PLACE_BATCH_MAX", q_cap)
        monkeypatch.setattr(ql, "PLACE_BATCH_MAX_PAIRS", pair_cap)
        ix = FakeIndex(size)
        got = api.find_loops(ix, gap, 2)
        asked = []
        for call in ix.calls:
            ranges = [pb.clamp(lo, hi, size) for _, (lo, hi) in call]
            ulo, uhi = pb.union(ranges)
            assert 1 <= len(call) <= q_cap and len(call) * (uhi - ulo) <= pair_cap, (q_cap, pair_cap, len(call), ulo, uhi)
            asked += [src for src, _ in call]
        assert asked == list(range(size)) and len(got) == size
        if q_cap == 1024 and pair_cap == 1 << 26:
            assert len(ix.calls) == 1
        else:
            assert len(ix.calls) > 1


class FakeKf:
    def __init__(self, at):
        self.at = at


class FakeHandle:
    def __init__(self):
        self.calls = []

    def register_batch_keyframes(self, pairs, fp, params, icp):
        self.calls.append(list(pairs))
        recs = [{"valid": (s.at + t.at) % 3 != 0, "n_final": 100 - abs(s.at - t.at), "final_inliers": []} for s, t, _ in pairs]
        return recs if icp is None else (recs, [{"status": 0, "pair": (s.at, t.at)} for s, t, _ in pairs])


def test_close_loops_makes_one_search_and_one_registration():
    from quatro_amd import api
    from quatro_amd import lib as ql
    fp = ql.FrontendParams()
    fp.seed = 5
    kfs = [FakeKf(i) for i in range(30)]
    queries = [FakeKf(12), (FakeKf(3), (20, 25)), (FakeKf(7), (4, 4)), FakeKf(29)]
    ix, h = FakeIndex(30), FakeHandle()
    got = api.close_loops(h, ix, kfs, queries, 2, id_lo=0, id_hi=10, fp=fp)
    assert len(ix.calls) == 1 and len(h.calls) == 1
    assert [rng for _, rng in ix.calls[0]] == [(0, 10), (20, 25), (4, 4), (0, 10)]
    ids = [[m["id"] for m in g["matches"]] for g in got]
    assert ids == [[9, 8], [20, 21], [], [9, 8]]
    assert [(s.at, t.at, seed) for s, t, seed in h.calls[0]] == [(12, 9, 5), (12, 8, 5), (3, 20, 5), (3, 21, 5), (29, 9, 5),
                                                                (29, 8, 5)]
    assert [len(g["records"]) for g in got] == [2, 2, 0, 2] and all("refined" not in g for g in got)
    for g in got:
        assert g["best"] == api.best_candidate(g["records"])
        assert g["best_id"] == (g["matches"][g["best"]]["id"] if g["best"] >= 0 else -1)
    assert (got[0]["best"], got[0]["best_id"]) == (1, 8)  # (12 + 9) % 3 == 0: not valid
    assert (got[2]["best"], got[2]["best_id"]) == (-1, -1)
    h = FakeHandle()
    got = api.close_loops(h, FakeIndex(30), kfs, queries, 2, id_hi=10, fp=fp, icp=object())
    assert [[r["pair"] for r in g["refined"]] for g in got] == [[(12, 9), (12, 8)], [(3, 20), (3, 21)], [], [(29, 9), (29, 8)]]
    # nothing to search, nothing to register
    h = FakeHandle()
    assert api.close_loops(h, FakeIndex(30), kfs, [], 2, fp=fp) == [] and h.calls == []
    assert api.close_loops(h, FakeIndex(30), kfs, [(FakeKf(1), (5, 5))], 2, fp=fp) == [
        {"matches": [], "records": [], "best": -1, "best_id": -1}] and h.calls == []
