"""The place index on the MI355X, through the C ABI: descriptors, distances and rankings bit-equal to the restatement
(tests/place_restate.py), retrieval of revisited scenes with their yaw, api.close_loop end to end, and the contract's edges."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import place_restate as pr

pytestmark = pytest.mark.gpu

SECTOR = 2 * np.pi / 60


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _rotate_thin(rng, cloud):
    """A copy of the cloud turned about z by a random angle, moved a little, with a random half to all of its points kept."""
    yaw, keep = rng.uniform(-np.pi, np.pi), rng.uniform(0.5, 1.0)
    c, s = np.cos(yaw), np.sin(yaw)
    out = cloud[rng.random(cloud.shape[0]) < keep].astype(np.float64)
    x, y = out[:, 0].copy(), out[:, 1].copy()
    out[:, 0], out[:, 1] = c * x - s * y + rng.uniform(-1, 1), s * x + c * y + rng.uniform(-1, 1)
    return out.astype(np.float32)


def _triples(matches):
    return [(m["id"], m["shift"], int(bits32(m["distance"])[0])) for m in matches]


def _want(q, entries, k, lo=0, hi=None):
    return [(i, s, int(bits32(d)[0])) for i, s, d in pr.query(q, entries, k, lo, hi)]


@pytest.fixture(scope="module")
def twenty(hip):
    """The twenty scans of kitti64_pair(0..4) and kitti64_pair_16k(0..4) as keyframes, and an index they were added to."""
    from quatro_amd import synth
    scans = []
    for k in range(5):
        scans += list(synth.kitti64_pair(k)[:2]) + list(synth.kitti64_pair_16k(k)[:2])
    kfs = [hip.keyframe(s) for s in scans]
    ix = hip.place_index(240)
    ids = [ix.add(kf) for kf in kfs]
    assert ids == list(range(20)) and len(ix) == 20
    yield kfs, ix
    ix.close()
    for kf in kfs:
        kf.close()


def test_descriptor_parity_with_the_restatement(hip, twenty):
    import torch
    from quatro_amd import lib as ql
    kfs, ix = twenty
    for i, kf in enumerate(kfs):
        vox = kf.fetch(ql.KF_VOX)
        want = pr.describe(vox)
        # (the comparison is not vacuous: a 360-degree sweep leaves no sector of the image empty, so every column takes part)
        assert want.any(axis=0).all(), i
        assert np.array_equal(bits32(ix.fetch(i)), bits32(want)), f"entry {i}: stored descriptor"
        assert np.array_equal(bits32(ix.fetch(i, ql.PLACE_COLNORM2)), bits32(pr.colnorm2(want))), f"entry {i}: column norms"
        assert np.array_equal(bits32(hip.place_describe(vox)), bits32(want)), f"entry {i}: describe, host memory"
        dev = hip.place_describe(torch.from_numpy(vox).cuda().contiguous())
        assert dev.is_cuda and np.array_equal(bits32(dev.cpu().numpy()), bits32(want)), f"entry {i}: describe, device memory"


def test_descriptor_ignores_non_finite_far_and_low_points(hip):
    rng = np.random.default_rng(3)
    good = np.zeros((4000, 4), dtype=np.float32)
    r, a = rng.uniform(0.5, 79.0, 4000), rng.uniform(-np.pi, np.pi, 4000)
    good[:, 0], good[:, 1], good[:, 2] = r * np.cos(a), r * np.sin(a), rng.uniform(-1.9, 8.0, 4000)
    junk = np.array([[np.nan, 1, 1, 0], [1, np.inf, 1, 0], [1, 1, -np.inf, 0], [1, 1, np.nan, 0], [80.0, 0, 50, 0],
                     [60, 60, 50, 0], [-500, 3, 50, 0], [3, 4, -2.0, 0], [3, 4, -7.5, 0]], dtype=np.float32)
    both = np.concatenate([junk, good, junk])
    got = hip.place_describe(both)
    assert np.array_equal(bits32(got), bits32(pr.describe(good))) and got.max() < 10.5 and np.count_nonzero(got) > 800
    assert not hip.place_describe(junk).any() and not hip.place_describe(np.zeros((0, 4), dtype=np.float32)).any()


def test_distance_and_ranking_parity_with_the_restatement(hip, twenty):
    from quatro_amd import lib as ql
    kfs, ix = twenty
    rng = np.random.default_rng(11)
    vox = [kf.fetch(ql.KF_VOX) for kf in kfs]
    entries = [ix.fetch(i) for i in range(20)]
    while len(entries) < 220:
        if len(entries) in (57, 58, 140):  # duplicates: the descriptor of entry 30 again
            d = entries[30]
        else:
            d = pr.describe(_rotate_thin(rng, vox[int(rng.integers(20))]))
        assert ix.add_desc(d) == len(entries)
        entries.append(d)
    assert len(ix) == 220
    E = np.stack(entries)
    queries = [("desc", entries[30])] + [("desc", pr.describe(_rotate_thin(rng, vox[int(rng.integers(20))]))) for _ in range(6)]
    queries += [("kf", 4), ("kf", 13), ("kf", 18)]
    worst64 = 0.0
    for n, (kind, q) in enumerate(queries):
        qd = entries[q] if kind == "kf" else q
        for lo, hi in ((0, None), (37, 150)):
            full = _want(qd, E, 64, lo, hi)
            for k in (1, 5, 64):
                got = ix.query(kfs[q], k, lo, hi) if kind == "kf" else ix.query_desc(qd, k, lo, hi)
                assert _triples(got) == full[:k], f"query {n} ({kind}) k {k} range {lo, hi}"
                assert all(m["yaw"] == float(pr.yaw_of(m["shift"], 60)) for m in got)
        for m in ix.query_desc(qd, 5):
            d64, _ = pr.distance64(qd, E[m["id"]])
            print(f"query {n} entry {m['id']}: float32 {float(m['distance']):.9f} binary64 {d64:.9f}")
            worst64 = max(worst64, abs(float(m["distance"]) - d64))
            assert abs(float(m["distance"]) - d64) <= 1e-5
    print(f"largest |float32 - binary64| distance: {worst64:.3e}")
    dup = ix.query_desc(entries[30], 5)  # the duplicates come back in id order, at distance 0
    assert [m["id"] for m in dup[:4]] == [30, 57, 58, 140] and all(m["distance"] == 0 and m["shift"] == 0 for m in dup[:4])
    assert dup[4]["distance"] > 0


@pytest.mark.parametrize("R,S", [(32, 64), (4, 8), (9, 13)])
def test_other_shapes_are_bit_equal_too(hip, twenty, R, S):
    from quatro_amd import lib as ql
    kfs, _ = twenty
    p = ql.default_place_params(num_rings=R, num_sectors=S, max_range=60.0, height_offset=1.5)
    with hip.place_index(8, p) as ix:
        for kf in kfs[:8]:
            ix.add(kf)
        E = np.stack([pr.describe(kf.fetch(ql.KF_VOX), R, S, 60.0, 1.5) for kf in kfs[:8]])
        for i in range(8):
            assert np.array_equal(bits32(ix.fetch(i)), bits32(E[i])), i
        for q in (9, 10):
            qd = pr.describe(kfs[q].fetch(ql.KF_VOX), R, S, 60.0, 1.5)
            assert _triples(ix.query(kfs[q], 8)) == _want(qd, E, 8)
            assert np.array_equal(bits32(ix.describe(kfs[q].fetch(ql.KF_VOX))), bits32(qd))


@pytest.fixture(scope="module")
def revisits(hip):
    """Twelve scenes: the index holds the SOURCE scans of kitti64_pair(k, max_xy=2.0), the queries are the TARGET scans —
    the same scene from a pose up to 2 m away at any yaw."""
    from quatro_amd import synth
    pairs = [synth.kitti64_pair(k, max_xy=2.0) for k in range(12)]
    src = [hip.keyframe(p[0]) for p in pairs]
    tgt = [hip.keyframe(p[1]) for p in pairs]
    ix = hip.place_index(12)
    for kf in src:
        ix.add(kf)
    yield pairs, src, tgt, ix
    ix.close()
    for kf in src + tgt:
        kf.close()


def _yaw(T):
    return float(np.arctan2(T[1, 0], T[0, 0]))


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def test_revisits_are_retrieved_with_their_yaw(revisits):
    """Top-1 is the revisited scene for all twelve, and the descriptor's yaw is within one sector of inv(T_gt)'s."""
    pairs, _, tgt, ix = revisits
    for k in range(12):
        top = ix.query(tgt[k], 3)
        err = _wrap(top[0]["yaw"] - _yaw(np.linalg.inv(pairs[k][2])))
        print(f"scene {k}: " + ", ".join(f"id {m['id']} d {float(m['distance']):.3f}" for m in top) + f" | yaw error {err / SECTOR:+.2f} sectors")
        assert top[0]["id"] == k, (k, top)
        assert abs(err) <= SECTOR, (k, err)


def test_close_loop_equals_the_calls_made_by_hand_and_finds_the_scene(hip, revisits):
    """api.close_loop(k = 3): its records are bit-identical to register_batch_keyframes on the same three pairs in the same
    order, and its winner is the revisited scene.  The CPU oracle (oracle.register_pair, which the device equals bit for bit)
    ranks the true scene first for every one of the twelve pairs: 175 .. 545 final inliers (yaw error < 1e-3 rad,
    translation error < 0.09 m) against at most 4 for the query's two most similar wrong scenes — no pair is exempt."""
    from quatro_amd import api
    from quatro_amd import lib as ql
    pairs, src, tgt, ix = revisits
    fp = ql.default_frontend_params(seed=0)
    for k in range(12):
        r = api.close_loop(hip, ix, src, tgt[k], 3, fp=fp)
        ids = [m["id"] for m in r["matches"]]
        hand = hip.register_batch_keyframes([(tgt[k], src[i], 0) for i in ids], fp)
        assert len(r["records"]) == len(hand) == 3
        for a, b in zip(r["records"], hand):
            assert a["status"] == b["status"] and a["valid"] == b["valid"] and a["L"] == b["L"]
            assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64))
            assert np.array_equal(a["clique"], b["clique"]) and np.array_equal(a["final_inliers"], b["final_inliers"])
        w = r["records"][r["best"]]
        Ti = np.linalg.inv(pairs[k][2])
        print(f"scene {k}: candidates {ids}, final inliers {[len(x['final_inliers']) for x in r['records']]}, winner "
              f"{r['best_id']}: yaw error {_wrap(_yaw(w['T']) - _yaw(Ti)):+.2e} rad, translation error "
              f"{np.linalg.norm(w['T'][:3, 3] - Ti[:3, 3]):.3f} m; descriptor yaw {r['matches'][r['best']]['yaw']:+.3f} against "
              f"{_yaw(w['T']):+.3f}")
        assert r["best_id"] == k and api.best_candidate(r["records"]) == r["best"]
    rr = api.close_loop(hip, ix, src, tgt[2], 2, fp=fp, icp=ql.default_icp_params())
    assert len(rr["refined"]) == 2 and rr["best_id"] == 2
    assert api.close_loop(hip, ix, src, tgt[2], 3, id_lo=5, id_hi=5, fp=fp) == {"matches": [], "records": [], "best": -1,
                                                                              "best_id": -1}


@pytest.fixture(scope="module")
def h2():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


def test_contract_edges(hip, h2, twenty):
    from quatro_amd import lib as ql
    kfs, big = twenty
    d0, d1 = big.fetch(0), big.fetch(1)
    with hip.place_index(2) as ix:
        info = ix.info()
        assert (info["size"], info["capacity"]) == (0, 2) and info["device_bytes"] >= 2 * 21 * 60 * 4
        assert ix.query(kfs[0], 5) == [] and ix.query_desc(d0, 5) == []  # an empty index is an empty range
        assert ix.add(kfs[0]) == 0 and ix.add_desc(d1) == 1
        for add in (lambda: ix.add(kfs[2]), lambda: ix.add_desc(d0)):  # full: refused, nothing changes
            with pytest.raises(ql.QuatroHipError) as e:
                add()
            assert e.value.code == ql.QTR_ERR_CAPACITY
        assert len(ix) == 2 and np.array_equal(ix.fetch(0), d0) and np.array_equal(ix.fetch(1), d1)
        assert [m["id"] for m in ix.query(kfs[1], 64)] == [1, 0]
        for k in (0, -1, 65):
            with pytest.raises(ql.QuatroHipError):
                ix.query(kfs[0], k)
            with pytest.raises(ql.QuatroHipError):
                ix.query_desc(d0, k)
        assert ix.query(kfs[0], 5, 1, 1) == [] and ix.query(kfs[0], 5, 2, 9) == [] and ix.query_desc(d0, 5, 7, 3) == []
        assert [m["id"] for m in ix.query(kfs[0], 5, -4, 1)] == [0] and [m["id"] for m in ix.query_desc(d0, 5, 1)] == [1]
        for bad_id in (-1, 2):
            with pytest.raises(ql.QuatroHipError):
                ix.fetch(bad_id)
        # another handle's keyframe, and this index through another handle
        with h2.keyframe(np.ascontiguousarray(kfs[0].fetch(ql.KF_VOX))) as foreign:
            out, n, ident = (ql.PlaceMatch * 64)(), C.c_int(5), C.c_int(-1)
            lib, bad = hip._lib, ql.QTR_ERR_BAD_ARG
            assert lib.qtr_place_query(hip._h, 0, ix._ix, foreign._kf, 0, 9, 3, out, C.byref(n)) == bad and n.value == 0
            assert "another handle" in hip.last_error()
            assert lib.qtr_place_query(h2._h, 0, ix._ix, foreign._kf, 0, 9, 3, out, C.byref(n)) == bad
            assert lib.qtr_place_query_desc(h2._h, 0, ix._ix, d0.ctypes.data, ql.MEM_HOST, 0, 9, 3, out, C.byref(n)) == bad
            assert lib.qtr_place_index_fetch(h2._h, ix._ix, 0, ql.PLACE_DESC, None, 0) < 0
            with h2.place_index(2) as other:
                assert lib.qtr_place_index_add(hip._h, 0, other._ix, kfs[0]._kf, C.byref(ident)) == bad
                assert lib.qtr_place_index_add(h2._h, 0, other._ix, kfs[0]._kf, C.byref(ident)) == bad
                assert ident.value == -1 and len(other) == 0
                assert other.add(foreign) == 0
        for p in (dict(num_rings=3), dict(num_rings=33), dict(num_sectors=7), dict(num_sectors=65), dict(max_range=0.0),
                  dict(max_range=float("nan"))):
            with pytest.raises(ql.QuatroHipError):
                hip.place_index(4, ql.default_place_params(**p))
        with pytest.raises(ql.QuatroHipError):
            hip.place_index(0)


def test_two_threads_query_one_index_from_two_slots(h2, twenty):
    _, big = twenty
    rng = np.random.default_rng(21)
    base = [big.fetch(i) for i in range(20)]
    with h2.place_index(400) as ix:
        for i in range(400):
            ix.add_desc((np.roll(base[i % 20], i // 20, axis=1) * rng.uniform(0.5, 1.5, (20, 1))).astype(np.float32))
        qs = [base[3], np.roll(base[12], 7, axis=1)]
        single = [_triples(ix.query_desc(qs[t], 10 + t, 0, None, 0)) for t in range(2)]
        E = np.stack([ix.fetch(i) for i in range(400)])
        assert all(single[t] == _want(qs[t], E, 10 + t) for t in range(2))
        out = [[None] * 8, [None] * 8]

        def work(t):
            for r in range(8):
                out[t][r] = _triples(ix.query_desc(qs[t], 10 + t, 0, None, t))

        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        for t in range(2):
            for r in range(8):
                assert out[t][r] == single[t], (t, r)


def test_destroying_the_handle_frees_a_forgotten_index():
    import torch
    from quatro_amd import lib as ql
    torch.cuda.synchronize()
    h = ql.Handle(0)
    h.close()
    free0, _ = torch.cuda.mem_get_info()
    h = ql.Handle(0)
    ix = h.place_index(20000)
    assert ix.info()["device_bytes"] == 20000 * 5040
    ix.add_desc(np.ones((20, 60), dtype=np.float32))
    assert len(ix.query_desc(np.ones((20, 60), dtype=np.float32), 3)) == 1
    h.close()  # (the index was never closed)
    free1, _ = torch.cuda.mem_get_info()
    assert free1 >= free0 - (2 << 20), (free0, free1)


def test_cpp_place_demo_finds_and_registers_the_revisited_scene(hip, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "place_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "place_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    scans = [synth.kitti64_pair(3, max_xy=2.0)[1]] + [synth.kitti64_pair(k, max_xy=2.0)[0] for k in (2, 3, 4)]
    files = []
    for k, sc in enumerate(scans):
        files.append(str(tmp_path / f"{k}.bin"))
        synth.save_kitti_bin(files[-1], sc)
    out = subprocess.run([exe, "2"] + files, capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    kfs = [hip.keyframe(ql.read_kitti_bin(f)) for f in files]
    try:
        with hip.place_index(3) as ix:
            for kf in kfs[1:]:
                ix.add(kf)
            found = ix.query(kfs[0], 2)
            for r, m in enumerate(found):
                assert out[r] == f"match {r} id {m['id']} shift {m['shift']} distance_bits {int(bits32(m['distance'])[0]):08x}", out
            assert found[0]["id"] == 1
            recs = hip.register_batch_keyframes([(kfs[0], kfs[1 + m["id"]], 0) for m in found], ql.default_frontend_params())
            assert out[2].split()[:4] == ["best", "1", "valid", "1"], out
            T = np.array([int(w, 16) for ln in out[3:7] for w in ln.split()], dtype=np.uint64)
            assert np.array_equal(T.view(np.float64).reshape(4, 4), recs[0]["T"]), out
    finally:
        for kf in kfs:
            kf.close()
