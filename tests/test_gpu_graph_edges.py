"""The consistency-graph kernels (quatro_amd/csrc/solver.hip: k_graph_build_tiles, k_graph_build, k_graph_build_mfma) on
the adversarial inputs of tests/graph_cases.py: bit matrices equal to the oracle's binary64 evaluation of the reference
expression, word for word, where the screens' margins, range guards and the squared-form shortcut of pair_consistent()
have to work — pairs at the threshold at every distance, exact ties, subnormal binary16 halves, short and zero-length
TIMs, norms on both sides of the MFMA kernel's range limit, map coordinates, non-finite rows, noise bounds that switch
the screens off.  Nothing here has a tolerance.

Sizes: 2048 is the first L of the MFMA kernel and 2047 the last of the tile kernel in the product library; 2111 gives 33
row blocks — a last row block of 63 rows and a last column group with one live tile of four; 130 and 257 (three and
five row blocks: a single partial column group, a diagonal-only strip) run through all three kernels in the comparison
build (QTR_GRAPH)."""
import os
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_cases as gc  # noqa: E402
from test_gpu_parity import _assert_same_solution  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(gc.CASES)
_ref = {}


def _oracle(qo, name, L):
    """(case, oracle bit matrix, oracle solve) — computed once per (case, L), shared, left unchanged"""
    if (name, L) not in _ref:
        c = gc.case(name, L)
        bm = qo.build_graph(c.src, c.tgt, c.noise_bound, c.cbar2)
        bm.setflags(write=False)
        _ref[(name, L)] = (c, bm, qo.solve(c.src, c.tgt, qo.default_params(noise_bound=c.noise_bound, cbar2=c.cbar2)))
    return _ref[(name, L)]


def _assert_same_graph(h, c, bm_o):
    L = c.src.shape[0]
    bm = h.debug_fetch(ql.DBG_GRAPH_BITMAP, np.uint64)
    assert bm.size == bm_o.size
    bm = bm.reshape(L, -1)
    if not np.array_equal(bm, bm_o):
        d = gc.bits_of(bm, ((L + 63) // 64) * 64) != gc.bits_of(bm_o, ((L + 63) // 64) * 64)
        ij = np.argwhere(d)
        raise AssertionError(f"{c.name} L={L}: {len(ij)} bits differ, first (row, column) {ij[:6].tolist()}, "
                             f"block {c.block}")
    bad = ~(np.isfinite(c.src).all(1) & np.isfinite(c.tgt).all(1))
    assert not bm[bad].any()
    if L % 64:
        assert not (bm[:, -1] >> np.uint64(L % 64)).any()


@pytest.mark.parametrize("name,L", [(n, L) for n in NAMES for L in (2048, 2111)] +
                         [("band_0.6", 2047), ("exact_ties", 2047)])
def test_product_graph_and_solution_equal_the_oracle(hip, qo, name, L):
    c, bm_o, o = _oracle(qo, name, L)
    r = hip.solve(c.src, c.tgt, ql.demo_params(noise_bound=c.noise_bound, cbar2=c.cbar2))
    _assert_same_graph(hip, c, bm_o)
    _assert_same_solution(r, o)
    assert r["n_edges"] == o["n_edges"]


@pytest.fixture(scope="module")
def engines():
    """a handle on the comparison build (-DQTR_TEST_ENGINES), where QTR_GRAPH picks the graph kernel at every launch"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    h = ql.Handle(0, lib_path=ql.TEST_ENGINES_LIB_PATH)
    yield h
    h.close()


@pytest.mark.parametrize("L", [130, 257, 2111])
@pytest.mark.parametrize("name", NAMES)
def test_all_three_graph_kernels_equal_the_oracle(engines, qo, name, L):
    """the MFMA kernel below its product threshold, the binary32 kernels above it"""
    c, bm_o, _ = _oracle(qo, name, L)
    prm = ql.demo_params(noise_bound=c.noise_bound, cbar2=c.cbar2)
    for engine in ("tiles", "strips", "mfma"):
        os.environ["QTR_GRAPH"] = engine
        try:
            engines.solve(c.src, c.tgt, prm)
        finally:
            os.environ.pop("QTR_GRAPH", None)
        try:
            _assert_same_graph(engines, c, bm_o)
        except AssertionError as e:
            raise AssertionError(f"QTR_GRAPH={engine}: {e}") from None


@pytest.mark.parametrize("name", ["band_0.6", "exact_ties", "short_tims"])
def test_pair_consistent_alone_on_the_block(hip, qo, name):
    """qtr_compute_tims + qtr_scale_mask run pair_consistent() on every TIM pair without any screen in front of it: a
    mismatch here is the binary64 path's (the squared-form shortcut, a division that is not IEEE), not a screen's."""
    L = 2111
    c, bm_o, _ = _oracle(qo, name, L)
    lo, hi = c.block
    ts, _ = hip.compute_tims(c.src[lo:hi, :3].T.astype(np.float64))
    tt, mp = hip.compute_tims(c.tgt[lo:hi, :3].T.astype(np.float64))
    mask = hip.scale_mask(ts, tt, c.noise_bound, c.cbar2)
    want = gc.bits_of(bm_o, L)[lo + mp[0], lo + mp[1]]
    assert mask.size == (hi - lo) * (hi - lo - 1) // 2
    bad = np.nonzero(mask != want)[0]
    assert bad.size == 0, (bad.size, (lo + mp[:, bad[:5]]).T.tolist())


@pytest.mark.parametrize("beta", [0.6, 0.5, 6.0, 0.004])
def test_pair_consistent_at_extreme_length_ratios(hip, beta):
    """qtr_scale_mask on binary64 TIMs with one length tiny and the other beta + tiny (1 + eps) (graph_cases.
    extreme_ratio_tims): a/b - 1 of the reference expression is rounded at ~2^-52 a/b, so at ratios beyond ~1e6 the
    reference's decision is made by its roundings far outside any fixed relative band of the squared form — the shortcut
    must leave such pairs to the verbatim expression.  Against the numpy restatement of solveForScale (pinned to the
    oracle by tests/test_graph_cases_cpu.py)."""
    ts, tt = gc.extreme_ratio_tims(beta)
    mask = hip.scale_mask(ts, tt, beta / 2, 1.0)
    want = gc.restate_mask(ts, tt, beta)
    bad = np.nonzero(mask != want)[0]
    assert want.any() and not want.all()
    assert bad.size == 0, (bad.size, ts[:, bad[:3]].T.tolist(), tt[:, bad[:3]].T.tolist())


_BATCH_L = (130, 2048, 2111, 257)
_BOUNDS = sorted({gc.case(n, 130).noise_bound for n in NAMES})


@pytest.mark.parametrize("noise_bound", _BOUNDS)
def test_batched_graph_kernels_on_mixed_sizes(qo, noise_bound):
    """The EXT = true instantiations: correspondence-only pairs of mixed L in ONE lane group of qtr_submit_batch (kernel
    variants are picked from the group's largest pair, so the small pairs go through the MFMA kernel here).  The solver's
    parameters belong to a batch, so there is one batch per noise bound: every case with that bound, sizes 130 / 2048 /
    2111 / 257 in turn (a bound with a single case: that case at all four).  Every record equals the oracle's."""
    names = [n for n in NAMES if gc.case(n, 130).noise_bound == noise_bound]
    items = [(n, _BATCH_L[k % 4]) for k, n in enumerate(names)] if len(names) >= 4 else \
        [(n, L) for n in names for L in _BATCH_L]
    assert len(items) <= 16
    refs = [_oracle(qo, n, L) for n, L in items]
    hb = ql.Handle(0, n_slots=32, max_points=65536, max_voxels=32768, max_corr=4096)  # two lanes of 16 pairs
    try:
        got = hb.register_batch([(None, None, 0, c.src, c.tgt) for c, _, _ in refs],
                                params=ql.demo_params(noise_bound=noise_bound))
    finally:
        hb.close()
    for (n, L), g, (c, _, o) in zip(items, got, refs):
        assert g["status"] == o["status"] and g["L"] == L, (n, L, g["status"])
        try:
            _assert_same_solution(g, o)
        except AssertionError as e:
            raise AssertionError(f"{n} L={L}: {e}") from None
        assert g["n_edges"] == o["n_edges"] and g["max_core"] == o["max_core"], (n, L)
        assert g["cost"] == o["cost"] or (np.isinf(g["cost"]) and np.isinf(o["cost"])), (n, L)
