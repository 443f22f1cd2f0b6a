"""Registration evaluation on the MI355X (qtr_evaluate / _pair / _keyframes / _keyframes_batch): every field of the record
bit-exact against the numpy restatement (tests/eval_restate.py, exhaustive search of tests/icp_brute.py), the
correspondences against icp_brute, the entry points against one another, the tie to one point-to-point ICP iteration, the
batch against the single calls, the refusals, api.close_loop end to end and the C++ demo.  Everything goes through the C ABI
binding."""
import os
import subprocess
import threading

import numpy as np
import pytest

import eval_restate as er
import icp_brute as ib

pytestmark = pytest.mark.gpu

DISTANCES = (0.3, 1.0, 3.0)
N_POOL = 10


def _check(got, want, what):
    assert got["status"] == 0, what
    bad = er.same_record(got, want)
    assert bad == [], (what, bad, {f: (got[f], want[f]) for f in bad if f not in ("information", "hessian_plane")})


def _same(a, b, what):
    assert a["status"] == b["status"] and er.same_record(a, b) == [], (what, er.same_record(a, b))
    assert np.array_equal(er.bits(a["T"]), er.bits(b["T"])), what


@pytest.fixture(scope="module")
def hip():
    from quatro_amd import lib as ql
    h = ql.Handle(0, n_slots=2)
    yield h
    h.close()


@pytest.fixture(scope="module")
def pool(hip):
    """Ten pairs of the 16k pool as keyframes: their voxels and the target's normals on the host, the registration's T, its
    point-to-plane refinement and the identity."""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    out = []
    fp = ql.default_frontend_params(seed=0)
    for k in range(N_POOL):
        s, t, _ = synth.kitti64_pair_16k(k)
        ks, kt = hip.keyframe(s, fp), hip.keyframe(t, fp)
        reg = hip.register_keyframes(ks, kt, fp)
        ref = hip.refine_pair()
        out.append({"ks": ks, "kt": kt, "vs": ks.fetch(ql.KF_VOX), "vt": kt.fetch(ql.KF_VOX), "nt": kt.fetch(ql.KF_NORMALS),
                    "Ts": {"registration": reg["T"].copy(), "refined": ref["T"].copy(), "identity": np.eye(4)}})
    yield out
    for p in out:
        p["ks"].close()
        p["kt"].close()


def test_every_field_is_bit_exact_on_the_pool_pairs(hip, pool):
    from quatro_amd import lib as ql
    seen = 0
    for k, p in enumerate(pool):
        for name, T in p["Ts"].items():
            near = er.nearest_any(p["vs"], p["vt"], T)
            for d in DISTANCES:
                got = hip.evaluate_keyframes(p["ks"], p["kt"], T, ql.default_eval_params(max_correspondence_distance=d))
                corr = hip.debug_fetch(ql.DBG_EVAL_CORR, np.int32)
                want = er.evaluate(p["vs"], p["vt"], T, d, p["nt"], near)
                what = f"pair {k} at the {name} T, {d} m"
                if d == 1.0:
                    print(f"{what}: overlap {got['overlap']:.4f} rmse {got['inlier_rmse']:.4f} plane rmse "
                          f"{got['plane_rmse']:.4f} n_corr {got['n_corr']} / {got['n_source']}")
                _check(got, want, what)
                assert np.array_equal(got["T"], np.asarray(T, np.float64)), what
                assert np.array_equal(corr, want["corr"]), what
                if k == 0 and d == 0.3:  # (the cached search thresholded is the search at that reach)
                    assert np.array_equal(corr, ib.search(p["vs"], p["vt"], T, d)[0]), what
                for M in (got["information"], got["hessian_plane"]):
                    assert np.array_equal(er.bits(M), er.bits(M.T)), what
                seen += got["n_corr"]
    assert seen > 100000


def _planted(p, seed=5):
    rng = np.random.default_rng(seed)
    s, t, n = p["vs"].copy(), p["vt"].copy(), p["nt"].copy()
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for a, frac in ((s, 0.02), (t, 0.02), (n, 0.05)):
        rows = rng.choice(a.shape[0], int(a.shape[0] * frac), replace=False)
        a[rows, rng.integers(0, 3, rows.size)] = bad[rng.integers(0, 3, rows.size)]
    return s, t, n


def test_raw_clouds_with_planted_non_finite_points(hip, pool):
    from quatro_amd import lib as ql
    p = pool[1]
    s, t, n = _planted(p)
    T = p["Ts"]["refined"]
    near = er.nearest_any(s, t, T)
    for d in DISTANCES:
        prm = ql.default_eval_params(max_correspondence_distance=d)
        for nrm in (n, None):
            want = er.evaluate(s, t, T, d, nrm, near)
            _check(hip.evaluate(s, t, T, nrm, prm), want, f"{d} m, normals {nrm is not None}")
            assert np.array_equal(hip.debug_fetch(ql.DBG_EVAL_CORR, np.int32), want["corr"])
            if nrm is not None:
                assert 0 < want["n_plane"] < want["n_corr"] < want["n_source"] < s.shape[0]
            else:
                assert want["n_plane"] == 0 and not want["hessian_plane"].any()
    # device-resident clouds take the same path
    import torch
    ds, dt, dn = (torch.from_numpy(a).cuda() for a in (s, t, n))
    _check(hip.evaluate(ds, dt, T, dn), er.evaluate(s, t, T, 1.0, n, near), "device tensors")
    # sizes around the chunk, and the empty outcomes
    for ns in (1, 63, 64, 257):
        _check(hip.evaluate(s[:ns], t, T, n), er.evaluate(s[:ns], t, T, 1.0, n), f"ns {ns}")
    empty = np.zeros((0, 4), np.float32)
    nan_t = t.copy()
    nan_t[:, 1] = np.nan
    for what, a, b, c in (("empty target", s, empty, None), ("empty source", empty, t, n), ("no finite target", s, nan_t, n)):
        got = hip.evaluate(a, b, T, c)
        _check(got, er.evaluate(a, b, T, 1.0, c), what)
        assert not got["valid"] and not got["information"].any() and not got["hessian_plane"].any(), what
    _check(hip.evaluate(s, t, T, n), er.evaluate(s, t, T, 1.0, n, near), "the slot is usable afterwards")


def test_evaluate_pair_equals_the_other_entries_and_leaves_the_registration_alone(hip):
    from quatro_amd import lib as ql
    from quatro_amd import synth
    s, t, _ = synth.kitti64_pair(3)
    fp = ql.default_frontend_params(seed=3)
    icp = ql.default_icp_params()
    r = hip.register_pair(s, t, fp)
    plain = hip.refine_pair(params=icp)
    r2 = hip.register_pair(s, t, fp)
    assert np.array_equal(r["T"], r2["T"])
    e0 = hip.evaluate_pair()
    after = hip.refine_pair(params=icp)
    e1 = hip.evaluate_pair(plain["T"], ql.default_eval_params(max_correspondence_distance=0.5))  # ... and it may follow one
    again = hip.refine_pair(params=icp)
    for x in (after, again):
        assert np.array_equal(er.bits(x["T"]), er.bits(plain["T"])) and er.bits(x["fitness"]) == er.bits(plain["fitness"])
        assert all(x[k] == plain[k] for k in ("iterations", "stop_reason", "n_corr", "valid", "converged"))
    vs, vt = hip.debug_fetch(ql.DBG_VOX_SRC, np.float32).reshape(-1, 4), hip.debug_fetch(ql.DBG_VOX_TGT, np.float32).reshape(-1, 4)
    with hip.keyframe(s, fp, slot=1) as ks, hip.keyframe(t, fp, slot=1) as kt:
        assert np.array_equal(vs, ks.fetch(ql.KF_VOX)) and np.array_equal(vt, kt.fetch(ql.KF_VOX))
        nt = kt.fetch(ql.KF_NORMALS)
        assert np.array_equal(er.bits(e0["T"]), er.bits(r["T"]))
        _same(e0, hip.evaluate(vs, vt, r["T"], nt, slot=1), "evaluate on the fetched clouds")
        _same(e0, hip.evaluate_keyframes(ks, kt, r["T"], slot=1), "evaluate_keyframes")
        _same(e1, hip.evaluate_keyframes(ks, kt, plain["T"], ql.default_eval_params(max_correspondence_distance=0.5), slot=1), "0.5 m")
        _check(e0, er.evaluate(vs, vt, r["T"], 1.0, nt), "restatement")
    # refused where qtr_refine_pair is: the slot's last call was not a registration; after a batch job
    hip.evaluate(vs, vt, r["T"])
    with pytest.raises(ql.QuatroHipError) as e:
        hip.evaluate_pair()
    assert e.value.code == ql.QTR_ERR_BAD_ARG
    hip.register_pair(s, t, fp)
    hip.register_batch([(s, t, 3)], fp)
    with pytest.raises(ql.QuatroHipError) as e:
        hip.evaluate_pair()
    assert e.value.code == ql.QTR_ERR_BAD_ARG


def test_sum_d2_and_n_corr_are_one_point_to_point_icp_iterations(hip, pool):
    from quatro_amd import lib as ql
    for k in (0, 4):
        p = pool[k]
        for name, T in p["Ts"].items():
            for d in (0.3, 1.0):
                ev = hip.evaluate_keyframes(p["ks"], p["kt"], T, ql.default_eval_params(max_correspondence_distance=d))
                hip.icp(p["vs"], p["vt"], guess=T, params=ql.default_icp_params(method=ql.ICP_POINT_TO_POINT, max_iterations=1,
                                                                               max_correspondence_distance=d))
                tr = hip.debug_fetch(ql.DBG_ICP_TRACE, np.float64).reshape(-1, 18)
                assert tr.shape[0] == 1 and int(tr[0, 17]) == ev["n_corr"] > 0, (k, name, d)
                assert er.bits(tr[0, 16]) == er.bits(ev["sum_d2"] / ev["n_corr"]), (k, name, d)


def _batch_pairs(pool, B):
    """B pairs: pool[0]'s source against the pool's targets in turn (a target repeats after ten), each at one of its own
    transforms moved a little — and every third pair another source."""
    out = []
    for b in range(B):
        p = pool[b % N_POOL]
        src = pool[(b // 3) % N_POOL]["ks"] if b % 3 == 2 else pool[0]["ks"]
        T = p["Ts"][("registration", "refined", "identity")[b % 3]] @ ib.rigid(ib.rot(0, 0, 0.001 * b), [0.01 * b, 0, 0])
        out.append((src, p["kt"], T))
    return out


@pytest.mark.parametrize("n_slots", [1, 16])
def test_batch_is_bit_identical_to_the_single_calls(pool, n_slots):
    from quatro_amd import lib as ql
    import torch
    ql.Handle(0, n_slots=n_slots).close()  # (what the runtime keeps of a handle's queues is there before the measurement)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    h = ql.Handle(0, n_slots=n_slots)
    try:
        # keyframes belong to a handle: this one gets its own, from the pool's stored voxels' scans
        from quatro_amd import synth
        fp = ql.default_frontend_params(seed=0)
        mine = []
        for k in range(N_POOL):
            s, t, _ = synth.kitti64_pair_16k(k)
            mine.append({"ks": h.keyframe(s, fp), "kt": h.keyframe(t, fp, slot=n_slots - 1), "Ts": pool[k]["Ts"]})
        prm = ql.default_eval_params(max_correspondence_distance=0.5)
        slot = n_slots - 1
        for B in (1, 5, 16, 64):
            pairs = _batch_pairs(mine, B)
            got = h.evaluate_keyframes_batch(pairs, prm, slot=slot)
            assert len(got) == B
            for b, (a, t, T) in enumerate(pairs):
                _same(got[b], h.evaluate_keyframes(a, t, T, prm, slot=0), f"B {B} pair {b}")
                if b % 3 != 2:  # (the query against a target of its own scene; the others may overlap little)
                    assert got[b]["valid"] and got[b]["n_corr"] > 100
        if n_slots == 16:  # two threads on two slots evaluate the same keyframes
            pairs = _batch_pairs(mine, 16)
            want = h.evaluate_keyframes_batch(pairs, prm)
            res = {}

            def work(sl):
                res[sl] = [h.evaluate_keyframes_batch(pairs, prm, slot=sl) for _ in range(3)]
            th = [threading.Thread(target=work, args=(sl,)) for sl in (3, 7)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            for sl in (3, 7):
                for run in res[sl]:
                    for a, b in zip(run, want):
                        _same(a, b, f"thread on slot {sl}")
    finally:
        h.close()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f"free device memory {free0} -> {free1} after destroy")
    assert free1 >= free0 - (2 << 20), (free0, free1)


def test_refusals_leave_the_slot_usable(hip, pool):
    from quatro_amd import lib as ql
    p = pool[2]
    T = p["Ts"]["registration"]
    good = hip.evaluate_keyframes(p["ks"], p["kt"], T)
    other = ql.Handle(0, n_slots=1)
    try:
        from quatro_amd import synth
        foreign = other.keyframe(synth.kitti64_pair(1)[0])
        badT = T.copy()
        badT[1, 2] = np.nan
        row3 = T.copy()
        row3[3, 0] = np.nan  # (row 3 is not read)
        calls = [lambda: hip.evaluate_keyframes(None, p["kt"], T), lambda: hip.evaluate_keyframes(p["ks"], None, T),
                 lambda: hip.evaluate_keyframes(foreign, p["kt"], T), lambda: hip.evaluate_keyframes(p["ks"], foreign, T),
                 lambda: hip.evaluate_keyframes(p["ks"], p["kt"], badT), lambda: hip.evaluate_keyframes(p["ks"], p["kt"], None),
                 lambda: hip.evaluate(p["vs"], p["vt"], badT), lambda: hip.evaluate_keyframes_batch([]),
                 lambda: hip.evaluate_keyframes_batch([(p["ks"], p["kt"], T)] * 65),
                 lambda: hip.evaluate_keyframes_batch([(p["ks"], p["kt"], T), (p["ks"], foreign, T)]),
                 lambda: hip.evaluate_keyframes_batch([(p["ks"], p["kt"], T), (p["ks"], p["kt"], badT)]),
                 lambda: hip.evaluate_keyframes_batch([(p["ks"], p["kt"], T), (None, p["kt"], T)])]
        for d in (0.0, -1.0, np.nan, np.inf):
            prm = ql.default_eval_params(max_correspondence_distance=d)
            calls += [lambda prm=prm: hip.evaluate_keyframes(p["ks"], p["kt"], T, prm),
                      lambda prm=prm: hip.evaluate(p["vs"], p["vt"], T, None, prm),
                      lambda prm=prm: hip.evaluate_keyframes_batch([(p["ks"], p["kt"], T)], prm)]
        for i, c in enumerate(calls):
            with pytest.raises(ql.QuatroHipError) as e:
                c()
            assert e.value.code == ql.QTR_ERR_BAD_ARG and hip.last_error(), i
            if i % 5 == 0:
                _same(hip.evaluate_keyframes(p["ks"], p["kt"], T), good, f"after refusal {i}")
        _same(hip.evaluate_keyframes(p["ks"], p["kt"], row3), dict(good, T=row3), "row 3")
        foreign.close()
    finally:
        other.close()
    small = ql.Handle(0, n_slots=1, max_voxels=8192)
    try:
        with pytest.raises(ql.QuatroHipError) as e:
            small.evaluate(p["vs"], p["vt"][:100], T)
        assert e.value.code == ql.QTR_ERR_CAPACITY and p["vs"].shape[0] > 8192
        _check(small.evaluate(p["vs"][:8192], p["vt"][:8192], T, p["nt"][:8192]),
               er.evaluate(p["vs"][:8192], p["vt"][:8192], T, 1.0, p["nt"][:8192]), "the slot is usable afterwards")
    finally:
        small.close()


def test_close_loop_evaluations_equal_the_restatement_at_the_refined_transforms():
    from quatro_amd import api
    from quatro_amd import lib as ql
    from quatro_amd import synth
    h = ql.Handle(0, n_slots=4)
    try:
        scans, poses = synth.kitti64_trajectory(0, 17, 1.0)
        kfs = [h.keyframe(s, slot=i % 4) for i, s in enumerate(scans)]
        fp = ql.default_frontend_params(seed=0)
        prm = ql.default_eval_params(max_correspondence_distance=0.5)
        with h.place_index(17) as ix:
            for kf in kfs[:17]:
                ix.add(kf)
            plain = api.close_loop(h, ix, kfs, kfs[17], 3, fp=fp, icp=ql.default_icp_params())
            r = api.close_loop(h, ix, kfs, kfs[17], 3, fp=fp, icp=ql.default_icp_params(), evaluate=prm, min_overlap=0.5)
        assert "evaluations" not in plain and len(r["evaluations"]) == 3
        q = kfs[17].fetch(ql.KF_VOX)
        for m, rec, ref, pl, ev in zip(r["matches"], r["records"], r["refined"], plain["refined"], r["evaluations"]):
            assert np.array_equal(ref["T"], pl["T"])
            if not rec["valid"]:
                assert ev is None
                continue
            t = kfs[m["id"]]
            want = er.evaluate(q, t.fetch(ql.KF_VOX), ref["T"], 0.5, t.fetch(ql.KF_NORMALS))
            print(f"candidate {m['id']}: overlap {ev['overlap']:.4f} inlier rmse {ev['inlier_rmse']:.4f} m")
            _check(ev, want, f"candidate {m['id']}")
            assert np.array_equal(ev["T"], ref["T"])
        ok = [rec if ev is not None and ev["overlap"] >= 0.5 else {} for rec, ev in zip(r["records"], r["evaluations"])]
        assert r["best"] == api.best_candidate(ok) and r["best"] >= 0 and r["best_id"] == r["matches"][r["best"]]["id"]
        assert r["evaluations"][r["best"]]["overlap"] >= 0.5
        if all(x for x in ok):  # (every candidate overlaps enough: the choice is the one without min_overlap)
            assert r["best"] == plain["best"]
        for kf in kfs:
            kf.close()
    finally:
        h.close()


def test_cpp_eval_demo_prints_the_python_paths_record(hip, tmp_path):
    from quatro_amd import build as qbuild
    from quatro_amd import lib as ql
    from quatro_amd import synth
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    libpath = qbuild.build(force=False, verbose=False)
    exe = str(tmp_path / "eval_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "eval_demo.cpp"), "-o", exe, "-L", os.path.dirname(libpath),
                           "-lquatro_hip", "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,-rpath,/opt/rocm/lib"])
    s, t, _ = synth.kitti64_pair(4)
    files = [str(tmp_path / "s.bin"), str(tmp_path / "t.bin")]
    synth.save_kitti_bin(files[0], s)
    synth.save_kitti_bin(files[1], t)
    out = subprocess.run([exe] + files + ["0.5"], capture_output=True, text=True, check=True, timeout=180).stdout.split("\n")
    with hip.keyframe(ql.read_kitti_bin(files[0])) as ks, hip.keyframe(ql.read_kitti_bin(files[1])) as kt:
        r = hip.register_keyframes(ks, kt, ql.default_frontend_params())
        e = hip.evaluate_keyframes(ks, kt, r["T"], ql.default_eval_params(max_correspondence_distance=0.5))
    assert out[0] == f"valid {int(e['valid'])} n_source {e['n_source']} n_corr {e['n_corr']} n_plane {e['n_plane']}", out
    words = np.array([int(w, 16) for ln in out[1:14] for w in ln.split()], dtype=np.uint64).view(np.float64)
    assert np.array_equal(er.bits(words[:4]), er.bits([e["overlap"], e["sum_d2"], e["inlier_rmse"], e["plane_rmse"]]))
    assert np.array_equal(er.bits(words[4:40]), er.bits(e["information"])) and e["valid"]
    assert np.array_equal(er.bits(words[40:76]), er.bits(e["hessian_plane"]))
