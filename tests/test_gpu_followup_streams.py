"""What follows the solver's mail — PMC_EXACT's two searches and the second estimate from the larger clique
(solve_followup / exact_phase / solver_refinalize in quatro_amd/csrc/capi.hip) — on a stream that is NOT the slot's own: the
lane's stream of a batch, the third stream of qtr_register_pair_corr.  Every record equals qtr_solve's with PMC_EXACT, T
bit for bit, clique and final inliers included.  The hard sets are the ones of test_exact_mode_through_the_solver on which
the exact clique beats the heuristic's, so no case passes without the follow-up having run.  No timing is a pass condition.
(No input is known that leaves the solver's state undone after its first chain: the solver_continue branch is not reached.)"""
import contextlib
import os

import numpy as np
import pytest

from quatro_amd import lib as ql
from quatro_amd import synth

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=65536, max_voxels=16384, max_corr=8192)
HARD = ((120, 1.5, 1), (200, 2.0, 3))  # (L, box size, seed): uniform points in a box of a few noise bounds


def _exact():
    return ql.demo_params(inlier_selection_mode=ql.INLIER_PMC_EXACT)


def _box(L, size, seed):
    rng = np.random.default_rng(seed)
    src = np.zeros((L, 4), dtype=np.float32)
    tgt = np.zeros((L, 4), dtype=np.float32)
    src[:, :3] = rng.uniform(0, size, (L, 3))
    tgt[:, :3] = rng.uniform(0, size, (L, 3))
    return src, tgt


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


def _handle(overlap=True, block=False, **kw):
    with _env(QTR_CORR_OVERLAP=None if overlap else "0", QTR_HOST_WAIT="block" if block else None):
        return ql.Handle(0, **LIMITS, **kw)


@pytest.fixture(scope="module")
def tiny():
    """the `tiny` scans of tests/test_gpu_corr_overlap.py: 250 points on a 0.8 m patch and their moved copy"""
    g = np.random.default_rng(3)
    g.uniform(0, 5.0, 2000), g.uniform(0, 5.0, 2000), g.normal(0, 0.01, 2000)
    e = np.zeros((250, 4), dtype=np.float32)
    e[:, 0], e[:, 1] = g.uniform(0, 0.8, 250), g.uniform(0, 0.8, 250)
    e[:, 2] = 0.1 * np.sin(5.0 * e[:, 0]) * np.cos(4.0 * e[:, 1]) + g.normal(0, 0.002, 250)
    f = e.copy()
    f[:, :3] = (e[:, :3].astype(np.float64) @ synth.yaw_matrix(0.2).T + np.asarray((0.05, -0.03, 0.01))).astype(np.float32)
    f[:, :3] += np.random.default_rng(13).normal(0, 0.0005, (250, 3)).astype(np.float32)
    return e, f


@pytest.fixture(scope="module")
def sets():
    """[easy, hard, hard]: (src, tgt) correspondence clouds"""
    return [synth.correspondences(300, 0.3, seed=1, noise=0.05)[:2]] + [_box(*h) for h in HARD]


@pytest.fixture(scope="module")
def want(sets, tiny):
    """qtr_solve with PMC_EXACT per set (computed once, shared, never changed), the front end's counts of the tiny pair, and
    the proof that the follow-up has work to do on the hard sets: the exact clique is larger than PMC_HEU's."""
    h = _handle()
    try:
        front = h.feature_pair(*tiny, _fp())
        recs = [h.solve(cs, ct, _exact()) for cs, ct in sets]
        heu = [h.solve(cs, ct) for cs, ct in sets]
    finally:
        h.close()
    for k in (1, 2):
        assert recs[k]["clique"].size > heu[k]["clique"].size, (k, recs[k]["clique"].size, heu[k]["clique"].size)
    return {"solve": recs, "front": front}


def _fp():
    return ql.default_frontend_params(seed=2)


def _record(r):
    return (r["status"], r["valid"], r["clique"].size, r["final_inliers"].size, r["cost"], r["L"])


def _same(got, rec, front=None):
    """the whole record, T bit for bit; front: the counts a call with scans reports beside it"""
    assert _record(got) == _record(rec)
    assert np.array_equal(got["T"].view(np.uint64), rec["T"].view(np.uint64))
    assert np.array_equal(got["clique"], rec["clique"]) and np.array_equal(got["final_inliers"], rec["final_inliers"])
    assert (got["n_src"], got["n_tgt"]) == ((front["n_src"], front["n_tgt"]) if front else (0, 0))
    if front and "n_matched" in got:
        assert got["n_matched"] == front["L"]


# the hard sets never sit first in their lane's group: four slots are two lanes of two, so pairs 1 and 3 run on a slot whose
# own stream is not the lane's
ORDER = (0, 1, 0, 2)


@pytest.mark.parametrize("block", [False, True])
def test_batch_of_correspondence_only_pairs(sets, want, block):
    h = _handle(block=block, n_slots=4)
    try:
        got = h.register_batch([(None, None, 2, *sets[k]) for k in ORDER], _fp(), _exact())
    finally:
        h.close()
    for g, k in zip(got, ORDER):
        _same(g, want["solve"][k])


def test_batch_pairs_with_scans_and_given_correspondences(sets, want, tiny):
    h = _handle(n_slots=4)
    try:
        got = h.register_batch([(*tiny, 2, *sets[k]) for k in ORDER], _fp(), _exact())
    finally:
        h.close()
    for g, k in zip(got, ORDER):
        _same(g, want["solve"][k], want["front"])


@pytest.mark.parametrize("overlap,block", [(True, False), (False, False), (True, True)])
def test_register_pair_corr(sets, want, tiny, overlap, block):
    """overlap: the back end beside the front end, its follow-up on the third stream; else the serial order of
    QTR_CORR_OVERLAP=0, on the slot's own"""
    h = _handle(overlap=overlap, block=block)
    try:
        got = [h.register_pair_corr(*tiny, cs, ct, _fp(), _exact()) for cs, ct in sets]
    finally:
        h.close()
    for g, rec in zip(got, want["solve"]):
        _same(g, rec, want["front"])
