"""No-GPU checks of the place index: the ctypes mirrors of the new structs have the C sizes and field offsets, every new
entry is exported, bound and refuses NULL arguments before it touches a device; the restatement (tests/place_restate.py)
has the properties the contract states — and equals include/qtr_place_math.h compiled for the host, bit for bit; and
api.close_loop registers exactly what the search returned."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import place_restate as pr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

NEW_ENTRIES = ("qtr_default_place_params", "qtr_place_index_create", "qtr_place_index_destroy", "qtr_place_index_get_info",
               "qtr_place_describe", "qtr_place_index_add", "qtr_place_index_add_desc", "qtr_place_index_fetch",
               "qtr_place_query", "qtr_place_query_desc")


@pytest.fixture(scope="module")
def lib():
    from quatro_amd import build as qbuild
    qbuild.build(force=False, verbose=False)
    from quatro_amd import lib as ql
    return ql.load()


def test_new_entries_are_exported_and_bound(lib):
    from quatro_amd import lib as ql
    for n in NEW_ENTRIES:
        assert n in ql.EXPORTS and hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None, n


def test_place_struct_layouts_match_header(lib):
    """sizeof and the offset of every field, from a C program compiled against the header."""
    from quatro_amd import lib as ql
    structs = (("qtr_place_params", ql.PlaceParams), ("qtr_place_match", ql.PlaceMatch),
               ("qtr_place_index_info", ql.PlaceIndexInfo))
    prints, want = [], []
    for cname, T in structs:
        prints.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(T))
        for f, _ in T._fields_:
            prints.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(T, f).offset)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "quatro_hip.h"\nint main(void){' + "".join(prints) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = list(map(int, subprocess.check_output([exe]).split()))
    assert got == want
    p = ql.default_place_params()
    assert (p.num_rings, p.num_sectors, p.max_range, p.height_offset) == (20, 60, 80.0, 2.0)


def test_null_arguments_are_refused_without_a_device(lib):
    from quatro_amd import lib as ql
    bad = ql.QTR_ERR_BAD_ARG
    p, info = ql.default_place_params(), ql.PlaceIndexInfo()
    ix, n, ident = C.c_void_p(), C.c_int(7), C.c_int(-5)
    pts = np.zeros((8, 4), dtype=np.float32)
    desc = np.zeros((20, 60), dtype=np.float32)
    out = (ql.PlaceMatch * 64)()
    lib.qtr_default_place_params(None)  # (a no-op)
    assert lib.qtr_place_index_create(None, C.byref(p), 16, C.byref(ix)) == bad and not ix
    assert lib.qtr_place_index_create(None, C.byref(p), 16, None) == bad
    lib.qtr_place_index_destroy(None, None)  # (a no-op)
    assert lib.qtr_place_index_get_info(None, C.byref(info)) == bad
    assert lib.qtr_place_describe(None, 0, C.byref(p), pts.ctypes.data, 8, desc.ctypes.data, ql.MEM_HOST) == bad
    assert lib.qtr_place_index_add(None, 0, None, None, C.byref(ident)) == bad and ident.value == -5
    assert lib.qtr_place_index_add_desc(None, 0, None, desc.ctypes.data, ql.MEM_HOST, C.byref(ident)) == bad
    assert lib.qtr_place_index_fetch(None, None, 0, ql.PLACE_DESC, None, 0) < 0
    assert lib.qtr_place_query(None, 0, None, None, 0, 10, 5, out, C.byref(n)) == bad and n.value == 0
    n.value = 7
    assert lib.qtr_place_query_desc(None, 0, None, desc.ctypes.data, ql.MEM_HOST, 0, 10, 5, out, C.byref(n)) == bad
    assert n.value == 0
    assert lib.qtr_place_query_desc(None, 0, None, desc.ctypes.data, ql.MEM_HOST, 0, 10, 5, None, None) == bad


# ---- restatement properties ------------------------------------------------------------------------------------------
def _centred_cloud(rng, R=20, S=60, max_range=80.0, fill=0.6, per_cell=3):
    """Points at the CENTRES of a random subset of the polar cells (far from every bin border), heights in (-1.5, 6)."""
    ring, sec = np.nonzero(rng.random((R, S)) < fill)
    ring, sec = np.repeat(ring, per_cell), np.repeat(sec, per_cell)
    rad = (ring + 0.5) * max_range / R
    ang = -np.pi + (sec + 0.5) * 2 * np.pi / S
    z = rng.uniform(-1.5, 6.0, ring.size)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), z, np.zeros_like(z)], axis=1)


def _rotate_z(cloud, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    out = cloud.copy()
    out[:, 0], out[:, 1] = c * cloud[:, 0] - s * cloud[:, 1], s * cloud[:, 0] + c * cloud[:, 1]
    return out


@pytest.mark.parametrize("m", [0, 1, 7, 30, 59])
def test_rotation_about_z_is_a_column_shift(m):
    """The sign convention, pinned on the CPU: a cloud turned by +m sectors about z has its descriptor moved m columns
    towards larger indices; queried with the original it is found at shift m, distance exactly 0, yaw = +m sectors wrapped."""
    rng = np.random.default_rng(100 + m)
    cloud = _centred_cloud(rng)
    d0 = pr.describe(cloud.astype(np.float32))
    d1 = pr.describe(_rotate_z(cloud, m * 2 * np.pi / 60).astype(np.float32))
    assert np.count_nonzero(d0) > 500
    assert np.array_equal(d1, np.roll(d0, m, axis=1))
    dist, shift = pr.best_shift(d0, d1[None])
    assert shift[0] == m and dist[0] == 0.0 and dist.dtype == np.float32
    want = m * 2 * np.pi / 60
    want = want - 2 * np.pi if want > np.pi + 1e-6 else want
    assert abs(float(pr.yaw_of(m, 60)) - want) < 1e-6 and -np.pi < pr.yaw_of(m, 60) <= pr.PI_F
    d64, s64 = pr.distance64(d0, d1)
    assert s64 == m and abs(d64) < 1e-12


def test_self_distance_is_zero_at_shift_zero_and_empty_is_one():
    from quatro_amd import synth
    s, t, _ = synth.kitti64_pair(1)
    ds, dt = pr.describe(s), pr.describe(t)
    dist, shift = pr.best_shift(ds, np.stack([ds, dt]))
    assert (dist[0], shift[0]) == (0.0, 0) and 0.0 < dist[1] < 1.0
    empty = pr.describe(np.zeros((0, 4), dtype=np.float32))
    assert not empty.any()
    for q, c in ((empty, ds), (ds, empty), (empty, empty)):
        dist, shift = pr.best_shift(q, c[None])
        assert (dist[0], shift[0]) == (1.0, 0)
    assert pr.distance64(empty, ds) == (1.0, 0)


def test_descriptor_ignores_what_the_contract_excludes():
    rng = np.random.default_rng(5)
    good = _centred_cloud(rng, fill=0.2).astype(np.float32)
    junk = np.array([[np.nan, 1, 1, 0], [1, np.inf, 1, 0], [1, 1, -np.inf, 0], [80.0, 0, 1, 0], [60, 60, 1, 0],
                     [3, 4, -2.0, 0], [3, 4, -7.5, 0]], dtype=np.float32)
    both = np.concatenate([junk, good, junk])
    assert np.array_equal(pr.describe(both), pr.describe(good))
    assert np.array_equal(pr.describe(good[::-1]), pr.describe(good))  # a function of the point set


def test_ranking_orders_by_distance_then_id():
    rng = np.random.default_rng(9)
    e = [pr.describe(_centred_cloud(rng).astype(np.float32)) for _ in range(6)]
    entries = np.stack([e[0], e[1], e[2], e[1], e[3], e[1]])  # 1, 3, 5 are duplicates
    got = pr.query(e[1], entries, 4)
    assert [g[0] for g in got[:3]] == [1, 3, 5] and all(g[2] == 0.0 for g in got[:3]) and got[3][2] > 0
    window = pr.query(e[1], entries, 64, 2, 5)
    assert window[0][0] == 3 and sorted(g[0] for g in window) == [2, 3, 4] and pr.query(e[1], entries, 3, 4, 4) == []


def test_restatement_equals_the_shared_header_compiled_for_the_host():
    """include/qtr_place_math.h is what the kernels call; compiled with g++ (-ffp-contract=off) it must give the
    restatement's bits: cells, column norms and every d(s)."""
    from quatro_amd import synth
    src = r'''
#include "qtr_place_math.h"
extern "C" {
void cells(const float* p, int n, int R, int S, float mr, float ho, int* cell, float* zh) {
  for (int i = 0; i < n; ++i) { zh[i] = 0; cell[i] = qtr_place_cell(p[4 * i], p[4 * i + 1], p[4 * i + 2], R, S, mr, ho, zh + i); }
}
void norms(const float* d, int R, int S, float* n2) { for (int j = 0; j < S; ++j) n2[j] = qtr_place_colnorm2(d, R, S, j); }
void dists(const float* q, const float* qn2, const float* c, const float* cn2, int R, int S, float* d) {
  for (int s = 0; s < S; ++s) d[s] = qtr_place_shift_distance(q, qn2, c, cn2, R, S, s);
}
float yaw(int shift, int S) { return qtr_place_yaw(shift, S); }
}
'''
    with tempfile.TemporaryDirectory() as tmp:
        cpp, so = os.path.join(tmp, "m.cpp"), os.path.join(tmp, "m.so")
        open(cpp, "w").write(src)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), cpp,
                               "-o", so])
        m = C.CDLL(so)
        m.yaw.restype = C.c_float
        fp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        s, t, _ = synth.kitti64_pair(0)
        for R, S in ((20, 60), (32, 64), (7, 9)):
            imgs = []
            for cloud in (s, t):
                cloud = np.ascontiguousarray(cloud, dtype=np.float32)
                n = cloud.shape[0]
                cell, zh = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
                m.cells(fp(cloud), n, R, S, C.c_float(80.0), C.c_float(2.0), fp(cell), fp(zh))
                img = np.zeros(R * S, dtype=np.float32)
                np.maximum.at(img, cell[cell >= 0], zh[cell >= 0])
                want = pr.describe(cloud, R, S)
                assert np.array_equal(img.reshape(R, S).view(np.uint32), want.view(np.uint32)), (R, S)
                n2 = np.zeros(S, dtype=np.float32)
                m.norms(fp(want), R, S, fp(n2))
                assert np.array_equal(n2.view(np.uint32), pr.colnorm2(want).view(np.uint32))
                imgs.append((want, n2))
            (q, qn2), (c, cn2) = imgs
            c = np.ascontiguousarray(np.roll(c, 11 % S, axis=1))
            c[:, 3] = 0  # an empty column on one side only
            cn2 = pr.colnorm2(c)
            d = np.zeros(S, dtype=np.float32)
            m.dists(fp(q), fp(qn2), fp(c), fp(cn2), R, S, fp(d))
            assert np.array_equal(d.view(np.uint32), pr.shift_distances(q, c[None])[0].view(np.uint32)), (R, S)
            assert all(np.float32(m.yaw(k, S)) == pr.yaw_of(k, S) for k in range(S))


def test_close_loop_registers_exactly_the_returned_candidates_in_order():
    from quatro_amd import api
    from quatro_amd import lib as ql

    class FakeIndex:
        def query(self, kf, k, id_lo, id_hi):
            self.args = (kf, k, id_lo, id_hi)
            return [{"id": i, "shift": 3 * i, "distance": 0.1 * n, "yaw": 0.0} for n, i in enumerate(self.ids[:k])]

    class FakeHandle:
        def register_batch_keyframes(self, pairs, fp, params, icp):
            self.pairs = pairs
            out = [{"valid": True, "n_final": {"kf4": 30, "kf9": 80, "kf2": 50}.get(p[1], 1)} for p in pairs]
            return out if icp is None else (out, [{"status": 0}] * len(pairs))

    h, ix = FakeHandle(), FakeIndex()
    ix.ids = [4, 9, 2, 7]
    kfs = [f"kf{i}" for i in range(12)]
    fp = ql.FrontendParams(0.3, 0.5, 0.75, 0.95, 1, 1, 5)
    r = api.close_loop(h, ix, kfs, "q", 3, id_lo=1, id_hi=10, fp=fp)
    assert ix.args == ("q", 3, 1, 10)
    assert h.pairs == [("q", "kf4", 5), ("q", "kf9", 5), ("q", "kf2", 5)]
    assert [m["id"] for m in r["matches"]] == [4, 9, 2] and len(r["records"]) == 3 and "refined" not in r
    assert (r["best"], r["best_id"]) == (1, 9)
    r = api.close_loop(h, ix, kfs, "q", 2, fp=fp, icp=object())
    assert h.pairs == [("q", "kf4", 5), ("q", "kf9", 5)] and len(r["refined"]) == 2 and r["best_id"] == 9
    ix.ids, h.pairs = [], None
    r = api.close_loop(h, ix, kfs, "q", 5, fp=fp)
    assert r == {"matches": [], "records": [], "best": -1, "best_id": -1} and h.pairs is None
