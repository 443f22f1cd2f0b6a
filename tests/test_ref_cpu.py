"""Anchors of the CPU oracle that the repository's own code did not produce.

* the REFERENCE's teaser::Matcher, compiled from the reference's own text (oracle/Makefile target `ref`): live comparison
  when oracle/_ref/libref_matcher.so is present, and the committed outputs it generated (tests/golden/matcher_ref.npz);
* the REFERENCE's Eigen-only back-end functions (computeTIMs, solveForScale, solveForRotation2D, solveForTranslation,
  estimate of include/quatro.hpp; target `ref_solver`): live, and their committed outputs (tests/golden/solver_ref.npz);
* the "live" tests' seeded calls replay the answers the compiled reference gave to them (tests/golden/ref_live_*.npz)
  where it cannot be compiled, and check those stored answers against it where it can;
* library cross-checks of the third-party semantics the oracle restates: scipy's cKDTree for the radius sets,
  numpy's eigh for pcl::eigen33, and a known answer of the published FPFH definition (Rusu 2009) on a plane.
"""
import hashlib
import os

import numpy as np
import pytest

from quatro_amd import synth

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def qo():
    from oracle import oracle as o
    o.build()
    o.set_threads(min(4, o.max_threads()))
    return o


class _Ref:
    """The compiled reference's functions (qo.ref_*) when it is there — each answer also checked against the one stored
    for the same call — else the stored answers, in call order: tests/golden/ref_live_<tag>.npz, written by these tests
    with QTR_REF_LIVE_WRITE=1 where the reference can be compiled.  Each answer is stored with a digest of the call's
    arguments, so that inputs which changed since the recording (synth, the tests' draws) fail as such, in both modes,
    rather than as a disagreement of oracle and reference.  `extra` adds test-local compositions of them."""

    def __init__(self, qo, tag, available, **extra):
        self.qo, self.live, self.extra, self.k = qo, available, extra, 0
        self.path = os.path.join(G, f"ref_live_{tag}.npz")
        self.stored = dict(np.load(self.path)) if os.path.exists(self.path) else None
        self.new = {}
        if not available and self.stored is None:
            pytest.fail(f"{self.path} is missing and the reference is not compiled "
                        "(QTR_REF_LIVE_WRITE=1: tests/golden/make_golden.py)")

    def __getattr__(self, name):
        def call(*a, **kw):
            key = f"{name}.{self.k}"
            self.k += 1
            digest = _digest(a, kw)
            if self.stored is not None and not (self.live and os.environ.get("QTR_REF_LIVE_WRITE")):
                if str(self.stored.get(key + ":args", "")) != digest:
                    pytest.fail(f"the arguments of call {key} are not those its stored answer in {self.path} was recorded "
                                "for: the inputs changed, record the file again (tests/golden/make_golden.py)")
            if not self.live:
                return _unflat(self.stored, key)
            r = (self.extra[name] if name in self.extra else getattr(self.qo, name))(*a, **kw)
            self.new.update(_flat(key, r))
            self.new[key + ":args"] = np.array(digest)
            if self.stored is not None and not os.environ.get("QTR_REF_LIVE_WRITE"):
                for k, v in _flat(key, r).items():
                    assert k in self.stored and np.array_equal(self.stored[k], v), ("stored answer differs", k)
            return r
        return call

    def save(self):
        if self.live and os.environ.get("QTR_REF_LIVE_WRITE"):
            np.savez_compressed(self.path, **self.new)


def _digest(args, kw):
    """sha256 of a call's arguments: arrays and numpy scalars by dtype, shape and bytes, Python values by repr"""
    hh = hashlib.sha256()
    for v in list(args) + [x for k in sorted(kw) for x in (k, kw[k])]:
        if isinstance(v, (np.ndarray, np.generic)):
            v = np.ascontiguousarray(v)
            hh.update(repr((v.dtype.str, v.shape)).encode())
            hh.update(v.tobytes())
        else:
            hh.update(repr(v).encode())
        hh.update(b"|")
    return hh.hexdigest()


def _flat(key, r):
    items = r.items() if isinstance(r, dict) else enumerate(r if isinstance(r, tuple) else (r,))
    kind = "dict" if isinstance(r, dict) else "tuple" if isinstance(r, tuple) else "one"
    return {key: np.array(kind), **{f"{key}.{k}": np.asarray(v) for k, v in items}}


def _unflat(stored, key):
    kind = str(stored[key])
    vals = {k[len(key) + 1:]: (v.item() if v.ndim == 0 else v) for k, v in stored.items() if k.startswith(key + ".")}
    if kind == "dict":
        return vals
    out = tuple(vals[str(i)] for i in range(len(vals)))
    return out if kind == "tuple" else out[0]


CASES = {"ab": ("a", "b", True, True, 11), "ba": ("b", "a", True, True, 12), "ab_nocross": ("a", "b", False, True, 13),
         "ba_nocross_notuple": ("b", "a", False, False, 14), "ab_notuple": ("a", "b", True, False, 15)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matcher_equals_reference_generated_golden(qo, name):
    """tests/golden/matcher_ref.npz holds what the reference's own advancedMatching returned (source larger / smaller,
    cross-check on / off, tuple test on / off): the oracle's restatement has to return the same lists."""
    g = np.load(os.path.join(G, "matcher_ref.npz"))
    s, t, cross, tup, seed = CASES[name]
    got = qo.match(g["xyz_" + s], g["desc_" + s], g["xyz_" + t], g["desc_" + t], crosscheck=cross, tuple_test=tup,
                   seed=seed)
    assert np.array_equal(got, g["corr_" + name])
    assert got.shape[0] > 20


def test_oracle_matcher_equals_compiled_reference_live(qo):
    """The same comparison against the compiled reference itself, on inputs with exact ties (duplicated descriptors),
    clouds of very different size and the degenerate single-point cloud."""
    ref = _Ref(qo, "matcher", bool(qo.build_ref() and qo.ref_available()))
    rng = np.random.default_rng(3)
    for trial in range(6):
        na, nb = int(rng.integers(1, 700)), int(rng.integers(1, 700))
        xa = rng.uniform(-20, 20, size=(na, 4)).astype(np.float32)
        xb = rng.uniform(-20, 20, size=(nb, 4)).astype(np.float32)
        da = rng.uniform(0, 100, size=(na, 33)).astype(np.float32)
        db = rng.uniform(0, 100, size=(nb, 33)).astype(np.float32)
        if trial % 2 and na > 10 and nb > 10:  # ties: copies inside a cloud and across the two clouds
            da[na // 2:na // 2 + 5] = da[0]
            db[:7] = da[0]
            db[nb // 2] = db[nb - 1]
        for cross in (True, False):
            for tup in (True, False):
                want = ref.ref_match(xa, da, xb, db, crosscheck=cross, tuple_test=tup, seed=trial)
                got = qo.match(xa, da, xb, db, crosscheck=cross, tuple_test=tup, seed=trial)
                assert np.array_equal(want, got), (trial, na, nb, cross, tup)
    s, t, _ = synth.kitti64_pair(5)
    vs, vt = qo.voxelize(s, 0.45), qo.voxelize(t, 0.45)
    _, _, ds = qo.fpfh(vs, 0.7, 1.0)
    _, _, dt = qo.fpfh(vt, 0.7, 1.0)
    for (a, da, b, db, seed) in ((vs, ds, vt, dt, 1), (vt, dt, vs, ds, 2)):
        assert np.array_equal(ref.ref_match(a, da, b, db, seed=seed), qo.match(a, da, b, db, seed=seed))
    ref.save()


def _graph_from_reference_mask(L, mp, mask):
    A = np.zeros((L, L), dtype=bool)
    A[mp[:, 0], mp[:, 1]] = mask
    return A | A.T


def _oracle_adjacency(qo, src, tgt, noise_bound=0.3, cbar2=1.0):
    L = src.shape[0]
    bm = qo.build_graph(src, tgt, noise_bound, cbar2)
    return np.unpackbits(bm.view(np.uint8), axis=1, bitorder="little")[:, :L].astype(bool)


def test_oracle_back_end_equals_reference_generated_golden(qo):
    """tests/golden/solver_ref.npz holds what the reference's OWN computeTIMs / solveForScale / solveForRotation2D /
    solveForTranslation / estimate returned (include/quatro.hpp, compiled from its text by `make -C oracle ref_solver`).
    The oracle's restatements have to agree: the consistency graph edge for edge, COTE and the translation bit for bit,
    the GNC-TLS yaw with the same inlier set and the rotation / cost to rounding (the oracle sums in a fixed 64-lane
    order and uses a closed-form 2 x 2 rotation — declared divergence D6)."""
    g = np.load(os.path.join(G, "solver_ref.npz"))
    A = _oracle_adjacency(qo, g["graph_src"], g["graph_tgt"])
    assert np.array_equal(A, _graph_from_reference_mask(A.shape[0], g["tims_map"], g["scale_mask"]))
    assert g["scale_mask"].sum() > 100
    nb = float(g["gnc_noise_bound"])
    for k in range(4):
        R, cost, iters, inl = qo.gnc_rotation2d(g[f"gnc{k}_src"], g[f"gnc{k}_dst"], nb)
        assert np.array_equal(inl, g[f"gnc{k}_inl"]), k
        assert np.abs(R - g[f"gnc{k}_R"]).max() < 1e-12, k
        rc = float(g[f"gnc{k}_cost"])
        assert (cost == rc) or abs(cost - rc) <= 1e-9 * abs(rc) + 1e-18, k
    for k in range(5):
        X, rg = g[f"cote{k}_X"], g[f"cote{k}_ranges"]
        for tag, ranges in (("u", np.full(X.shape[0], 0.3)), ("r", rg)):
            for median in (1, 0):
                e, m, _ = qo.cote_estimate_ranges(X, ranges, bool(median))
                assert e == float(g[f"cote{k}_{tag}{median}_est"]), (k, tag, median)
                assert np.array_equal(m, g[f"cote{k}_{tag}{median}_inl"]), (k, tag, median)
    a, b = g["trans_src"], g["trans_dst"]
    t, inl = [], np.ones(a.shape[0], dtype=bool)
    for ax in range(3):
        e, m, _ = qo.cote_estimate(b[:, ax] - a[:, ax], 0.3, True)
        t.append(e)
        inl &= m
    assert np.array_equal(np.array(t), g["trans_t"]) and np.array_equal(inl, g["trans_inl"])


def _ct_params(g, k):
    return dict(cote_median=int(g[f"ct{k}_cote_median"]), using_rot_inliers_when_estimating_cote=int(g[f"ct{k}_use_rot"]),
                inlier_selection_mode=int(g[f"ct{k}_mode"]))


def test_oracle_solve_equals_reference_compute_transformation_golden(qo):
    """Quatro::computeTransformation of the reference, compiled from its text with only PMC's clique search answered by the
    oracle's (on the graph the reference code built): chain TIMs, yaw, the rotation-inlier rule, COTE, final inliers and
    the 4 x 4 (tests/golden/solver_ref.npz, ct* entries).  The oracle's solve() has to return the same clique, the same
    rotation / final inlier lists and the same transform to rounding — including the invalid case (clique of one)."""
    g = np.load(os.path.join(G, "solver_ref.npz"))
    for k in range(6):
        o = qo.solve(g[f"ct{k}_src"], g[f"ct{k}_tgt"], qo.default_params(**_ct_params(g, k)))
        assert o["valid"] == bool(g[f"ct{k}_valid"]), k
        if not o["valid"]:
            assert g[f"ct{k}_clique"].size <= 1  # "Clique size too small. Abort." (include/quatro.hpp:809-813)
            continue
        assert np.array_equal(np.sort(o["clique"]), g[f"ct{k}_clique"]), k
        assert np.array_equal(o["rot_inliers"], g[f"ct{k}_rot"]) and np.array_equal(o["final_inliers"], g[f"ct{k}_final"]), k
        assert np.abs(o["T"] - g[f"ct{k}_T"]).max() < 1e-12, k
    assert not bool(g["ct5_valid"]) and bool(g["ct1_valid"])


def test_oracle_back_end_equals_compiled_reference_live(qo):
    """The same comparisons against the compiled reference functions themselves, on fresh random inputs."""
    def ref_graph(src, tgt, nb, cbar2):  # computeTIMs of both clouds, then solveForScale's mask: (index map, mask)
        ts, mp = qo.ref_compute_tims(src[:, :3].astype(np.float64))
        tt, _ = qo.ref_compute_tims(tgt[:, :3].astype(np.float64))
        return mp, qo.ref_scale_mask(ts, tt, nb, cbar2)
    ref = _Ref(qo, "solver", bool(qo.build_ref_solver() and qo.ref_solver_available()), ref_graph=ref_graph)
    g = np.random.default_rng(77)
    for L in (2, 3, 40, 260):
        src, tgt, _, _ = synth.correspondences(L, 0.3, seed=100 + L, noise=0.05)
        for nb, cbar2 in ((0.3, 1.0), (0.1, 2.0)):
            mp, mask = ref.ref_graph(src, tgt, nb, cbar2)
            assert np.array_equal(_oracle_adjacency(qo, src, tgt, nb, cbar2), _graph_from_reference_mask(L, mp, mask)), (L, nb)
    for trial in range(12):
        M = int(g.integers(3, 500))
        ang = g.uniform(-3, 3)
        Rt = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        a = g.normal(0, 5, (M, 2))
        b = a @ Rt.T + g.normal(0, g.choice([0.0, 0.02, 0.2]), (M, 2))
        bad = g.random(M) > g.choice([0.2, 0.6, 1.0])
        b[bad] = g.normal(0, 5, (int(bad.sum()), 2))
        Rr, cr, ir = ref.ref_gnc_rotation2d(a, b)
        Ro, co, _, io = qo.gnc_rotation2d(a, b, qo.REF_GNC_NOISE_BOUND)
        assert np.array_equal(io, ir), trial
        assert np.abs(Ro - Rr).max() < 1e-11, trial
        assert (co == cr) or abs(co - cr) <= 1e-9 * abs(cr) + 1e-18, trial  # (noise-free pairs: costs of 1e-29)
    for trial in range(40):
        N = int(g.integers(2, 400))
        X = g.normal(0, g.choice([0.1, 1.0, 30.0]), N)
        if trial % 3 == 0:
            X[:max(2, N // 2)] = g.normal(0.5, 0.05, max(2, N // 2))
        ranges = g.uniform(0.05, 0.6, N) if trial % 2 else np.full(N, float(g.choice([0.1, 0.3, 0.6])))
        for median in (True, False):
            er, mr = ref.ref_cote_estimate(X, ranges, median)
            eo, mo, nc = qo.cote_estimate_ranges(X, ranges, median)
            if median and nc < 2:
                continue  # the reference reads past its candidate list for a consensus set of one (declared divergence D4)
            assert eo == er and np.array_equal(mo, mr), (trial, N, median)
    for trial in range(10):  # the whole back end
        L = int(g.integers(2, 260))
        src, tgt, _, _ = synth.correspondences(L, float(g.choice([0.0, 0.1, 0.4, 1.0])), seed=300 + trial,
                                               noise=float(g.choice([0.0, 0.05, 0.2])))
        kw = [{}, {"cote_median": 0}, {"using_rot_inliers_when_estimating_cote": 1}, {"inlier_selection_mode": 2}][trial % 4]
        o = qo.solve(src, tgt, qo.default_params(**kw))
        r = ref.ref_compute_transformation(src, tgt, cote_median=bool(kw.get("cote_median", 1)),
                                           use_rot_inliers=bool(kw.get("using_rot_inliers_when_estimating_cote", 0)),
                                           inlier_selection_mode=kw.get("inlier_selection_mode", 1))
        assert o["valid"] == r["valid"], (trial, L)
        if o["valid"] and kw.get("cote_median", 1) and min(o["n_card"]) < 2:
            continue  # a consensus set of one: the reference reads candidates[-1] (declared divergence D4)
        if o["valid"]:
            assert np.array_equal(np.sort(o["clique"]), r["clique"]), (trial, L)
            assert np.array_equal(o["rot_inliers"], r["rot_inliers"]), (trial, L)
            assert np.array_equal(o["final_inliers"], r["final_inliers"]), (trial, L)
            assert np.abs(o["T"] - r["T"]).max() < 1e-11, (trial, L)
    for d in (2, 3):  # teaser::utils::svdRot2d / svdRot against numpy's SVD construction
        X = g.normal(0, 1, (60, d))
        Q, _ = np.linalg.qr(g.normal(0, 1, (d, d)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] *= -1
        Y = X @ Q.T + g.normal(0, 0.01, (60, d))
        W = g.random(60)
        U, _, Vt = np.linalg.svd((X * W[:, None]).T @ Y)
        V = Vt.T
        if np.linalg.det(U) * np.linalg.det(V) < 0:
            V[:, -1] *= -1
        assert np.abs(ref.ref_svd_rot(X, Y, W) - V @ U.T).max() < 1e-12
    ref.save()


def test_radius_sets_against_scipy_ckdtree(qo):
    """pcl::search::KdTree::radiusSearch restated (sorted (d^2, index) lists, query included) vs scipy's cKDTree: the same
    sets, up to points within rounding of the radius."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    pts = np.zeros((3000, 4), dtype=np.float32)
    pts[:, :3] = rng.uniform(-6, 6, size=(3000, 3))
    pts[:50, :3] = pts[50:100, :3]  # duplicates
    r = 0.75
    off, idx, d2 = qo.radius_neighbors(pts, r)
    tree = cKDTree(pts[:, :3].astype(np.float64))
    inner = tree.query_ball_point(pts[:, :3].astype(np.float64), r * (1 - 1e-5))
    outer = tree.query_ball_point(pts[:, :3].astype(np.float64), r * (1 + 1e-5))
    for i in range(pts.shape[0]):
        mine = idx[off[i]:off[i + 1]]
        assert set(inner[i]) <= set(mine.tolist()) <= set(outer[i])
        dd = d2[off[i]:off[i + 1]]
        assert np.all(np.diff(dd) >= 0) and i in mine
        exact = ((pts[mine, :3].astype(np.float64) - pts[i, :3].astype(np.float64)) ** 2).sum(axis=1)
        assert np.allclose(dd, exact, rtol=1e-5, atol=1e-9)


def test_eigen33_against_numpy_eigh_on_random_covariances(qo):
    """pcl::eigen33 (closed-form smallest eigenpair, float) vs numpy.linalg.eigh (float64) on 100 000 random covariance
    matrices: eigenvalue to float accuracy (99.9 % below 2e-5 relative, all below 5e-4), eigenvector to 2e-3 rad whenever the smallest eigenvalue is separated."""
    rng = np.random.default_rng(5)
    n = 100000
    pts = rng.normal(size=(n, 12, 3)) * rng.uniform(0.05, 2.0, size=(n, 1, 3))
    rot = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    pts = pts @ rot
    c = pts - pts.mean(axis=1, keepdims=True)
    cov = (c.transpose(0, 2, 1) @ c / 12.0)
    ev, vec = qo.eigen33(cov.astype(np.float32))
    w, v = np.linalg.eigh(cov.astype(np.float32).astype(np.float64))
    scale = np.abs(cov).max(axis=(1, 2))
    err = np.abs(ev - w[:, 0]) / scale  # the closed form (trigonometric roots in float) is not an iterative solver:
    assert np.quantile(err, 0.999) < 2e-5 and err.max() < 5e-4  # a few ill-conditioned cases lose 3 more digits
    sep = (w[:, 1] - w[:, 0]) / scale
    ok = sep > 0.05
    assert ok.mean() > 0.8
    cosang = np.abs((vec.astype(np.float64) * v[:, :, 0]).sum(axis=1))
    assert np.all(np.arccos(np.clip(cosang[ok], -1, 1)) < 2e-3)
    assert np.allclose(np.linalg.norm(vec, axis=1), 1.0, atol=1e-5)


def test_fpfh_known_answer_on_a_plane(qo):
    """Published definition (Rusu et al. 2009; PCL's 11-bin layout): on a plane every Darboux frame gives
    f1 = atan2(w.n2, n1.n2) = 0, f2 = v.n2 = 0, f3 = n1.d/|d| = 0, i.e. the centre bin (5) of each 11-bin block.  The SPFH
    and the FPFH of every interior point are therefore (0,...,0,100,0,...,0) per block — exactly."""
    xs, ys = np.meshgrid(np.arange(-4, 4.001, 0.25), np.arange(-4, 4.001, 0.25))
    pts = np.zeros((xs.size, 4), dtype=np.float32)
    pts[:, 0] = xs.ravel()
    pts[:, 1] = ys.ravel()
    pts[:, 2] = -1.5  # below the viewpoint: every normal flips to +z
    nrm, sp, de = qo.fpfh(pts, 0.6, 0.9)
    assert np.allclose(np.abs(nrm[:, 2]), 1.0, atol=1e-5) and np.all(nrm[:, 2] > 0)
    interior = (np.abs(pts[:, 0]) < 2.5) & (np.abs(pts[:, 1]) < 2.5)
    want = np.zeros(33, dtype=np.float32)
    want[[5, 16, 27]] = 100.0
    assert np.allclose(sp[interior], want[None, :], atol=2e-3)
    assert np.allclose(de[interior], want[None, :], atol=2e-3)
