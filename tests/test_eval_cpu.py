"""Registration evaluation without a GPU: include/qtr_eval_math.h compiled by g++ equals the numpy float64 restatement
(tests/eval_restate.py) bit for bit; the information matrix is Open3D's sum of G^T G; the five entry points are declared,
exported, bound and refuse their arguments before they touch a device; api.close_loop keeps its calls with the defaults
and evaluates at the refined transforms otherwise."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import eval_restate as er
import icp_brute as ib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ["qtr_default_eval_params", "qtr_evaluate", "qtr_evaluate_pair", "qtr_evaluate_keyframes",
         "qtr_evaluate_keyframes_batch"]

# the largest |information - sum G^T G| / max|sum G^T G| measured over CASES on the CPU (printed by the test): 2.1e-15;
# the two differ only by the order of summation.  Asserted: ten times that.
INFORMATION_REL_MEASURED = 2.1e-15

HOST_SRC = r'''
#include "qtr_eval_math.h"
#include <vector>
extern "C" {
// the header's terms for given correspondences, summed in the header's shape, finished
void run(const double* T, const float* src, int ns, const float* tgt, const float* nrm, const int* corr, QtrEvalRecord* rec,
         double* S_out, double* plane_out /* [22]: qtr_icp_terms(0, ..) summed the same way: 21 J^T J, r^2 */) {
  const int nchunk = (ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  double S[QTR_EVAL_NT], P[QTR_ICP_NT];
  for (int k = 0; k < QTR_EVAL_NT; ++k) S[k] = 0.0;
  for (int k = 0; k < QTR_ICP_NT; ++k) P[k] = 0.0;
  std::vector<double> e((size_t)QTR_ICP_CHUNK * QTR_EVAL_NT), o((size_t)QTR_ICP_CHUNK * QTR_ICP_NT);
  for (int c = 0; c < nchunk; ++c) {
    for (size_t k = 0; k < e.size(); ++k) e[k] = 0.0;
    for (size_t k = 0; k < o.size(); ++k) o[k] = 0.0;
    for (int l = 0; l < QTR_ICP_CHUNK; ++l) {
      const int i = c * QTR_ICP_CHUNK + l;
      if (i >= ns) break;
      const float* p = src + 4 * i;
      if (!qtr_icp_finite3(p[0], p[1], p[2])) continue;
      double q[3];
      qtr_icp_transform(T, p[0], p[1], p[2], q);
      const int j = corr[i];
      float t[3] = {0, 0, 0}, n[3] = {0, 0, 0};
      int plane = 0;
      double d2 = 0.0;
      if (j >= 0) {
        for (int a = 0; a < 3; ++a) t[a] = tgt[4 * j + a];
        d2 = qtr_icp_d2(q, t[0], t[1], t[2]);
        if (nrm) {
          for (int a = 0; a < 3; ++a) n[a] = nrm[4 * j + a];
          plane = qtr_icp_finite3(n[0], n[1], n[2]) ? 1 : 0;
        }
      }
      qtr_eval_terms(q, j >= 0, t[0], t[1], t[2], plane, n[0], n[1], n[2], d2, &e[(size_t)l * QTR_EVAL_NT]);
      if (plane) qtr_icp_terms(0, q, t[0], t[1], t[2], n[0], n[1], n[2], d2, &o[(size_t)l * QTR_ICP_NT]);
    }
    for (int pass = 0; pass < 2; ++pass) {
      const int nt = pass ? QTR_ICP_NT : QTR_EVAL_NT;
      const std::vector<double>& v = pass ? o : e;
      double* acc = pass ? P : S;
      for (int k = 0; k < nt; ++k) {
        double w[4];
        for (int wv = 0; wv < 4; ++wv) {
          double lanes[64];
          for (int l = 0; l < 64; ++l) lanes[l] = v[(size_t)(64 * wv + l) * nt + k];
          w[wv] = qtr_icp_fold64(lanes);
        }
        const double cs = qtr_icp_chunk_sum(w);
        acc[k] = c == 0 ? cs : acc[k] + cs;
      }
    }
  }
  qtr_eval_finish(S, rec);
  for (int k = 0; k < QTR_EVAL_NT; ++k) S_out[k] = S[k];
  for (int k = 0; k < 21; ++k) plane_out[k] = P[k];
  plane_out[21] = P[QTR_ICP_T_R2];
}
int nt_terms() { return QTR_EVAL_NT; }
}
'''


class Record(C.Structure):
    _fields_ = [("valid", C.c_int), ("n_source", C.c_int), ("n_corr", C.c_int), ("n_plane", C.c_int),
                ("overlap", C.c_double), ("sum_d2", C.c_double), ("inlier_rmse", C.c_double), ("plane_rmse", C.c_double),
                ("information", C.c_double * 36), ("hessian_plane", C.c_double * 36)]


@pytest.fixture(scope="module")
def host():
    with tempfile.TemporaryDirectory() as tmp:
        cpp, so = os.path.join(tmp, "e.cpp"), os.path.join(tmp, "e.so")
        open(cpp, "w").write(HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), cpp,
                               "-o", so])
        yield C.CDLL(so)


@pytest.fixture(scope="module")
def lib():
    from quatro_amd import build as qbuild
    qbuild.build(force=False, verbose=False)
    from quatro_amd import lib as ql
    return ql.load()


def _rigid(rng, scale=3.0, angle=0.2):
    return ib.rigid(ib.rot(*rng.uniform(-angle, angle, 3)), rng.uniform(-scale, scale, 3))


def _cases():
    """(name, src, tgt, tgt normals or None, T, max_d): a cluttered box of points seen twice under a random rigid T, with NaN
    / inf points and normals planted in both clouds, at 1, 63, 64, 257 and 1000 source points; a source with no partner; an
    empty target; a target without a finite point; no normals."""
    rng = np.random.default_rng(31)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    out = []
    for ns in (1, 63, 64, 257, 1000):
        T = _rigid(rng)
        tgt = ib.f4(rng.uniform(-8, 8, (1500, 3)) * np.array([1.0, 1.0, 0.25]))
        pick = rng.integers(0, 1500, ns)
        p = (tgt[pick, :3].astype(np.float64) - T[:3, 3]) @ T[:3, :3] + rng.normal(0, 0.05, (ns, 3))  # R^T (t - tr)
        src = ib.f4(p)
        nrm = ib.unit_normals(1500, ns)
        for a, frac in ((src, 0.05), (tgt, 0.03), (nrm, 0.1)):
            rows = rng.choice(a.shape[0], max(1, int(a.shape[0] * frac)), replace=False) if a.shape[0] > 1 else []
            for r in rows:
                a[r, rng.integers(0, 3)] = bad[rng.integers(0, 3)]
        for max_d in (0.1, 0.5):
            out.append((f"ns_{ns}_max_d_{max_d}", src, tgt, nrm, T, max_d))
        out.append((f"ns_{ns}_no_normals", src, tgt, None, T, 0.5))
    far = ib.f4(rng.uniform(-1, 1, (300, 3)) + 500.0)
    out.append(("no_partner", far, out[-1][2], out[-2][3], np.eye(4), 0.5))
    out.append(("empty_target", far, np.zeros((0, 4), np.float32), None, np.eye(4), 0.5))
    out.append(("empty_source", np.zeros((0, 4), np.float32), out[-3][2], out[-4][3], np.eye(4), 0.5))
    nan_t = out[0][2].copy()
    nan_t[:, 0] = np.nan
    out.append(("target_all_non_finite", out[-5][1], nan_t, out[-6][3], _rigid(rng), 0.5))
    return out


CASES = _cases()


def _host_record(host, src, tgt, nrm, T, corr):
    rec, S, P = Record(), np.zeros(er.NT), np.zeros(22)
    T16 = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    corr = np.ascontiguousarray(corr, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    host.run(vp(T16), vp(src), src.shape[0], vp(tgt), None if nrm is None else vp(nrm), vp(corr), C.byref(rec), vp(S), vp(P))
    got = {f: getattr(rec, f) for f in er.FIELDS_INT + er.FIELDS_F64[:4]}
    got["information"] = np.array(rec.information[:]).reshape(6, 6)
    got["hessian_plane"] = np.array(rec.hessian_plane[:]).reshape(6, 6)
    return got, S, P


def test_header_compiled_for_the_host_equals_the_float64_restatement(host):
    assert host.nt_terms() == er.NT
    seen = {"corr": 0, "plane": 0, "dropped_normals": 0}
    for name, src, tgt, nrm, T, max_d in CASES:
        want = er.evaluate(src, tgt, T, max_d, nrm)
        got, S, P = _host_record(host, src, tgt, nrm, T, want["corr"])
        assert np.array_equal(er.bits(S), er.bits(want["S"])), name
        assert er.same_record(got, want) == [], (name, er.same_record(got, want))
        # the plane sums are qtr_icp_terms(0, ..) summed the same way
        H = want["hessian_plane"]
        assert np.array_equal(er.bits(P[:21]), er.bits(H[np.triu_indices(6)])), name
        assert np.array_equal(er.bits(P[21]), er.bits(want["S"][er.T_R2])), name
        for M in (got["information"], got["hessian_plane"]):
            assert np.array_equal(er.bits(M), er.bits(M.T)), name  # exactly symmetric
        assert want["n_source"] == int(ib.finite3(src).sum()) and want["n_corr"] == int((want["corr"] >= 0).sum()), name
        if nrm is None:
            assert want["n_plane"] == 0 and not H.any(), name
        seen["corr"] += want["n_corr"]
        seen["plane"] += want["n_plane"]
        seen["dropped_normals"] += (want["n_corr"] - want["n_plane"]) if nrm is not None else 0
    assert seen["corr"] > 2000 and seen["plane"] > 1000 and seen["dropped_normals"] > 20, seen  # (the cases are not vacuous)
    by = {c[0]: er.evaluate(*c[1:3], c[4], c[5], c[3]) for c in CASES[-4:]}
    assert by["no_partner"]["n_source"] == 300 and by["empty_target"]["n_source"] == 300
    for r in by.values():
        assert not r["valid"] and r["n_corr"] == 0 and r["overlap"] == 0.0 and not r["information"].any()


def test_information_is_open3ds_sum_of_gtg(host):
    """Against the explicit per-correspondence sum of G^T G (eval_restate.open3d_information): measured relative difference
    over CASES 2.1e-15 of the largest entry; asserted at ten times that."""
    worst = 0.0
    for name, src, tgt, nrm, T, max_d in CASES:
        want = er.evaluate(src, tgt, T, max_d, nrm)
        if not want["valid"]:
            continue
        got, _, _ = _host_record(host, src, tgt, nrm, T, want["corr"])
        ref = er.open3d_information(tgt, want["corr"])
        rel = float(np.abs(got["information"] - ref).max() / np.abs(ref).max())
        worst = max(worst, rel)
    print(f"largest relative difference information vs sum G^T G: {worst:.3e}")
    assert worst <= 10 * INFORMATION_REL_MEASURED, worst


def test_entry_points_are_declared_exported_and_bound(lib):
    from quatro_amd import lib as ql
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    declared = set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*\(", hdr))
    listed = set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*;", open(os.path.join(ROOT, "quatro_amd", "csrc", "exports.map")).read()))
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    for n in NAMES:
        assert n in declared and n in listed and n in ql.EXPORTS and re.search(rf"\bT {n}\b", dyn), n
        assert getattr(lib, n).argtypes is not None, n
    assert "#define QTR_EVAL_MAX_PAIRS 64" in hdr and ql.EVAL_MAX_PAIRS == 64
    assert "#define QTR_DBG_EVAL_CORR 18" in hdr and ql.DBG_EVAL_CORR == 18
    assert "qtr_eval_math.h" in " ".join(__import__("quatro_amd.build", fromlist=["SOURCES"]).SOURCES)


def test_struct_sizes_match_a_compiled_c_program():
    from quatro_amd import lib as ql
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "quatro_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(qtr_eval_params), sizeof(qtr_eval_result), sizeof(qtr_eval_kf_pair),
         offsetof(qtr_eval_result, T), offsetof(qtr_eval_result, information), offsetof(qtr_eval_kf_pair, T),
         sizeof(qtr_icp_result));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(ql.EvalParams), C.sizeof(ql.EvalResult), C.sizeof(ql.EvalKfPair), ql.EvalResult.T.offset,
                   ql.EvalResult.information.offset, ql.EvalKfPair.T.offset, C.sizeof(ql.IcpResult)]
    assert got[:3] == [16, 24 + 8 * (16 + 4 + 72), 16 + 128]


def test_the_abi_refuses_its_arguments_without_a_device(lib):
    from quatro_amd import lib as ql
    bad = ql.QTR_ERR_BAD_ARG
    prm = ql.default_eval_params()
    assert prm.max_correspondence_distance == 1.0 and list(prm.reserved) == [0, 0]
    lib.qtr_default_eval_params(None)  # (a NULL is ignored)
    res, T = ql.EvalResult(), np.eye(4).reshape(16)
    res.status = 77
    pts = np.zeros((8, 4), np.float32)
    assert lib.qtr_evaluate(None, 0, pts.ctypes.data, 8, pts.ctypes.data, 8, None, T.ctypes.data, C.byref(prm), C.byref(res), 0) == bad
    assert lib.qtr_evaluate_pair(None, 0, T.ctypes.data, C.byref(prm), C.byref(res)) == bad
    assert lib.qtr_evaluate_keyframes(None, 0, None, None, T.ctypes.data, C.byref(prm), C.byref(res)) == bad
    pairs, out = (ql.EvalKfPair * 65)(), (ql.EvalResult * 65)()
    for B in (0, 1, 64, 65):
        assert lib.qtr_evaluate_keyframes_batch(None, 0, pairs, B, C.byref(prm), out) == bad, B
    assert res.status == 77  # (a call without a handle writes nothing)


# ---- close_loop against a handle that records its calls ---------------------------------------------------------------------
class FakeHandle:
    def __init__(self, overlaps):
        self.pairs, self.evals, self.overlaps = None, [], overlaps

    def register_batch_keyframes(self, pairs, fp, params, icp):
        self.pairs = pairs
        out = [{"valid": k != 2, "n_final": 10 + 5 * (k == 1), "T": np.eye(4) * (k + 1)} for k in range(len(pairs))]
        ref = [{"status": 0 if k != 3 else 7, "valid": True, "T": np.eye(4) * (10 + k)} for k in range(len(pairs))]
        return out if icp is None else (out, ref)

    def evaluate_keyframes_batch(self, pairs, params=None, slot=0):
        self.evals.append((pairs, params, slot))
        return [{"overlap": self.overlaps[t], "T": T} for _, t, T in pairs]


class FakeIndex:
    def __init__(self, ids):
        self.ids = ids

    def __len__(self):
        return 12

    def query(self, kf, k, id_lo, id_hi):
        return [{"id": i, "shift": 0, "distance": 0.1 * n, "yaw": 0.0} for n, i in enumerate(self.ids[:k])]


def test_close_loop_defaults_make_the_calls_they_made_before():
    from quatro_amd import api
    h, ix = FakeHandle({}), FakeIndex([4, 9, 2, 7])
    kfs = [f"kf{i}" for i in range(12)]
    r = api.close_loop(h, ix, kfs, "q", 4)
    assert h.evals == [] and [p[:2] for p in h.pairs] == [("q", "kf4"), ("q", "kf9"), ("q", "kf2"), ("q", "kf7")]
    assert sorted(r) == ["best", "best_id", "matches", "records"] and (r["best"], r["best_id"]) == (1, 9)
    r = api.close_loop(h, ix, kfs, "q", 4, icp=object())
    assert h.evals == [] and sorted(r) == ["best", "best_id", "matches", "records", "refined"]


def test_close_loop_evaluates_at_the_refined_transforms_and_applies_min_overlap():
    from quatro_amd import api
    kfs = [f"kf{i}" for i in range(12)]
    ov = {"kf4": 0.9, "kf9": 0.2, "kf2": 0.95, "kf7": 0.6}
    prm = object()
    # without icp: the registration's T of every VALID record (candidate 2 is not valid: not evaluated)
    h = FakeHandle(ov)
    r = api.close_loop(h, FakeIndex([4, 9, 2, 7]), kfs, "q", 4, evaluate=prm)
    (pairs, seen, _), = h.evals
    assert seen is prm and [(a, b) for a, b, _ in pairs] == [("q", "kf4"), ("q", "kf9"), ("q", "kf7")]
    assert [T[0, 0] for _, _, T in pairs] == [1.0, 2.0, 4.0]
    assert [None if e is None else e["overlap"] for e in r["evaluations"]] == [0.9, 0.2, None, 0.6]
    assert (r["best"], r["best_id"]) == (1, 9)  # (evaluate alone does not change the choice)
    # with icp: the refined T where the refinement ran (candidate 3's status is not QTR_OK: its registration T)
    h = FakeHandle(ov)
    r = api.close_loop(h, FakeIndex([4, 9, 2, 7]), kfs, "q", 4, icp=object(), evaluate=True, min_overlap=0.5)
    (pairs, seen, _), = h.evals
    assert seen is None and [T[0, 0] for _, _, T in pairs] == [10.0, 11.0, 4.0]
    assert (r["best"], r["best_id"]) == (0, 4)  # candidate 1 has the most inliers but overlaps too little
    h = FakeHandle(ov)
    r = api.close_loop(h, FakeIndex([4, 9, 2, 7]), kfs, "q", 4, min_overlap=0.99)  # (implies evaluate)
    assert len(h.evals) == 1 and (r["best"], r["best_id"]) == (-1, -1)
    r = api.close_loop(FakeHandle(ov), FakeIndex([]), kfs, "q", 4, evaluate=True)
    assert r["evaluations"] == [] and r["best"] == -1


def test_overlap_of_the_twelve_revisits_separates_the_true_scene_from_the_wrong_ones():
    """The retrieval case of tests/test_gpu_place.py on the CPU: the twelve queries (the TARGET scans of kitti64_pair(k,
    max_xy=2.0)) against their true scene and the two most similar wrong scenes of the place search, each evaluated by the
    restatement at the oracle's registration T, leaf 0.3 m, max_d 0.5 m.  Recorded with this test: the true scene overlaps
    0.945 .. 0.980 (inlier RMSE 0.112 .. 0.171 m), the wrong ones 0.007 .. 0.098 (0.287 .. 0.338 m) — a gap on all twelve,
    so exactly that ordering is asserted.  (A synthetic scene; it says nothing yet about real ground-dominated sweeps.)"""
    from oracle import oracle as qo
    from quatro_amd import synth
    import place_restate as pr
    qo.build()
    qo.set_threads(min(8, qo.max_threads()))
    pairs = [synth.kitti64_pair(k, max_xy=2.0) for k in range(12)]
    scenes = [qo.voxelize(p[0], 0.3) for p in pairs]
    queries = [qo.voxelize(p[1], 0.3) for p in pairs]
    E = np.stack([pr.describe(v) for v in scenes])
    for k in range(12):
        wrong = [i for i, _, _ in pr.query(pr.describe(queries[k]), E, 12) if i != k][:2]
        ev = []
        for i in [k] + wrong:
            o = qo.register_pair(pairs[k][1], pairs[i][0], seed=0)
            ev.append(er.evaluate(queries[k], scenes[i], np.asarray(o["T"], np.float64), 0.5))
        print(f"scene {k}: true overlap {ev[0]['overlap']:.4f} rmse {ev[0]['inlier_rmse']:.4f} | wrong {wrong}: "
              + ", ".join(f"{e['overlap']:.4f} / {e['inlier_rmse']:.4f}" for e in ev[1:]))
        assert ev[0]["overlap"] > max(e["overlap"] for e in ev[1:]), k
