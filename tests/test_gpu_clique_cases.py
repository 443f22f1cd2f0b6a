"""The clique stage (quatro_amd/csrc/solver.hip: k_kcore_levels, k_kcore_collect_rank, k_hcore_async, d_kcore, k_rank_sort,
k_permute_scatter, the clique rounds; exact.hip) on the named graphs of tests/clique_cases.py, each of which sits on a
size or a core number where the host code or a kernel changes route: clique, largest core, core numbers and the
(core, id) order equal to the oracle's, through qtr_max_clique, through lane groups of qtr_submit_batch and under the
comparison engines.  Nothing here has a tolerance.  tests/test_clique_cases_cpu.py holds the oracle to an independent
restatement on the same graphs and shows which wrong variant each graph catches.

The order (QTR_DBG_PERM) is compared on the vertices whose core number is at or above the floor the run worked with
(QTR_DBG_SOLVER_STATE[29]): below a floor the device's numbers are upper bounds by design.  The floor and the
second-run flag ([22]) depend on timing above 1280 vertices; they are printed, not asserted.

The exact search is skipped by the reference and by the device when the heuristic's clique already has max_core + 1
members (reference src/graph.cc:100-102), which is the case on every `planted` graph: there exact_stats()["nodes"] is
asserted to be 0, on the `block` graphs (heuristic < exact) it is asserted to be positive."""
import os
import subprocess
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql
from quatro_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clique_cases as cc  # noqa: E402
from test_gpu_parity import _assert_same_solution, assert_cores  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODES = ((1, 0.5), (2, 0.5), (2, 0.0), (2, 1.0))
EXACT_NAMES = [f"block_{L}" for L, _, _ in cc.BLOCK_SHAPES] + ["planted_4097", "planted_8193", "planted_16385"]
_refs = {}


def _clean(name):
    return name[6:] if name.startswith("dirty_") else name


def _oracle(qo, name):
    """core numbers, largest core and the clique of every mode: computed once per graph, shared, left unchanged (the
    oracle reads the bits as they are, so a dirty twin is held to its clean case)"""
    name = _clean(name)
    if name not in _refs:
        bm = cc.case(name).bitmap
        core, _, mc = qo.kcore(bm)
        ref = {"core": np.asarray(core), "max_core": int(mc)}
        for mode, thr in MODES:
            ref[(mode, thr)] = qo.max_clique(bm, mode, thr)
        ref["core"].setflags(write=False)
        _refs[name] = ref
    return _refs[name]


@pytest.fixture(scope="module")
def hip32k():
    """the largest handle qtr_create admits: max_corr = 32768"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    h = ql.Handle(0, max_points=65536, max_voxels=32768, max_corr=32768)
    yield h
    h.close()


def check_case(h, c, ref, modes=MODES, say=print):
    """one graph through qtr_max_clique in every mode (shared with tests/gpu_clique_engines.py)"""
    L = c.claims["L"]
    for mode, thr in modes:
        got, max_core = h.max_clique(c.bitmap, mode, thr)
        st = h.debug_fetch(ql.DBG_SOLVER_STATE, np.int32)
        say(f"{c.name} mode {mode} thr {thr}: clique {got.size} floor {int(st[29])} second run {int(st[22])}")
        assert np.array_equal(got, ref[(mode, thr)]), (c.name, mode, thr, got[:8], ref[(mode, thr)][:8])
        assert max_core == ref["max_core"], (c.name, mode, thr)
        floor = assert_cores(h, ref["core"])
        if mode == 1:
            core = ref["core"]
            n_hi = int(np.sum(core >= floor))
            if c.claims["kind"] in ("tie", "complete"):
                # every vertex of positive degree has the one non-zero core number, and a floor is at most half of it
                assert np.all(core[core > 0] >= floor), (c.name, floor)
            perm = h.debug_fetch(ql.DBG_PERM, np.int32)[:L]
            want = cc.restate_perm(core)
            assert np.array_equal(perm[L - n_hi:], want[L - n_hi:]), (c.name, floor, n_hi)


@pytest.mark.parametrize("name", cc.NAMES)
def test_clique_stage_equals_the_oracle(hip, hip32k, qo, name):
    c = cc.case(name)
    check_case(hip32k if c.claims["L"] > hip.limits.max_corr else hip, c, _oracle(qo, name))


@pytest.mark.parametrize("name", EXACT_NAMES + ["dirty_" + n for n in cc.DIRTY_OF])
def test_exact_search_equals_the_oracle(hip, qo, name):
    c = cc.case(name)
    clean = cc.case(_clean(name)).bitmap
    ref = _oracle(qo, name)
    want = np.sort(qo.max_clique(clean, 0))
    got, max_core = hip.max_clique(c.bitmap, 0)
    stats = hip.exact_stats()
    print(f"{name}: exact {got.size} heuristic {ref[(1, 0.5)].size} nodes {stats['nodes']} width {cc.exact_nw(c.claims['L'])}")
    assert np.array_equal(got, want) and max_core == ref["max_core"]
    assert cc.is_clique(clean, got)
    assert not stats["aborted"]
    if 1 <= ref[(1, 0.5)].size < ref["max_core"] + 1:
        assert stats["nodes"] > 0
    else:  # the heuristic reached the bound, or a graph without an edge: no search (see the module docstring)
        assert stats["nodes"] == 0
    if c.claims["kind"] == "block":
        heu, _ = hip.max_clique(c.bitmap, 1)
        assert got.size == c.claims["exact"] > heu.size == c.claims["heuristic"] and stats["nodes"] > 0


# ---------------------------------------------------------------------------------------------- lane groups
def _all_inliers(L, seed):
    """tgt = a rigid copy of src, no noise: every pair of correspondences is consistent, the graph is K_L"""
    src, _, T, _ = synth.correspondences(L, 0.0, seed, noise=0.0)
    tgt = np.zeros_like(src)
    tgt[:, :3] = (src[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return src, tgt


@pytest.mark.parametrize("largest", [1024, 1280, 1281])
def test_lane_group_members_beside_a_largest_pair(hip, qo, largest):
    """Correspondence-only pairs in ONE lane group of qtr_submit_batch: every pair runs the kernels chosen for the
    largest (the EXT instantiations) — the levels path at 1024 and 1280, k_hcore_async at 1281, whose control words sit
    at perm[64 .. 1088) of pairs with 1, 2, 64, 65, 1088 and 1089 correspondences.  Every record equals the oracle's and
    the single qtr_solve call's."""
    sizes = [s for s in (1, 2, 64, 65, 1088, 1089) if s < largest] + [largest]
    sets = [synth.correspondences(s, frac, 40 + k, 0.1)[:2] for k, s in enumerate(sizes) for frac in (0.0, 0.3)]
    sets += [_all_inliers(65, 7), _all_inliers(largest, 8)]
    assert len(sets) <= 16  # one lane of a 32-slot handle
    hb = ql.Handle(0, n_slots=32, max_points=65536, max_voxels=32768, max_corr=4096)
    try:
        got = hb.register_batch([(None, None, 0, a, b) for a, b in sets])
    finally:
        hb.close()
    for j, ((a, b), g) in enumerate(zip(sets, got)):
        o = qo.solve(a, b)
        one = hip.solve(a, b)
        for r in (g, one):
            # (the oracle numbers its outcomes itself: 0 solved, 1 no clique of two — QTR_ERR_CLIQUE_TOO_SMALL in the C ABI)
            assert r["status"] == {0: ql.QTR_OK, 1: ql.QTR_ERR_CLIQUE_TOO_SMALL}[o["status"]], (j, a.shape[0], r["status"])
            assert (r["n_edges"], r["max_core"]) == (o["n_edges"], o["max_core"]), (j, a.shape[0])
            try:
                _assert_same_solution(r, o)
            except AssertionError as e:
                raise AssertionError(f"pair {j} of {a.shape[0]} correspondences beside {largest}: {e}") from None
        assert g["L"] == a.shape[0]
    assert got[-1]["clique"].size == largest and got[-2]["clique"].size == 65  # the complete graphs from points


# ---------------------------------------------------------------------------------------------- comparison engines
ENGINE_SETTINGS = (("QTR_KCORE", "peel"), ("QTR_KCORE", "sweeps"), ("QTR_RANK_QUADRATIC", "1"), ("QTR_CLIQUE_ROUND0", "1"))
_engine_child_died = []


@pytest.mark.parametrize("var,value", ENGINE_SETTINGS)
def test_comparison_engines_on_the_same_cases(var, value):
    """tests/gpu_clique_engines.py under the -DQTR_TEST_ENGINES build: the peeling workgroup, the h-index sweeps, the
    quadratic ranking and the separate round 0 on every case of at most 4097 vertices (and the path of 16385 vertices
    under `peel`: the global-queue form).  One fresh child per setting — the library reads its variables once — one after
    another; after a child that ended on a signal or its time limit no further child is started: the settings behind it
    fail without running."""
    assert not _engine_child_died, f"not started: the child of {_engine_child_died[0]} ended on a signal or its time limit"
    env = dict(os.environ)
    env[var] = value
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_clique_engines.py"), f"{var}={value}"], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _engine_child_died.append(f"{var}={value}")
        raise
    if p.returncode < 0:
        _engine_child_died.append(f"{var}={value}")
    print(p.stdout[-400:])
    assert p.returncode == 0 and "CLIQUE_ENGINES_OK" in p.stdout, (var, value, p.returncode, p.stdout[-1500:], p.stderr[-1500:])
