"""No-GPU checks of tests/clique_cases.py, the inputs of tests/test_gpu_clique_cases.py:

  * the oracle (qo.kcore, qo.max_clique: what the device is held to) equals the numpy / pure-Python restatement on every
    case: core numbers, the (core, id) order, the heuristic's clique with its acceptance rules, and on the small cases
    the exact search; a dirty twin restates to what its clean case does;
  * the oracle's maximum clique has the size an independent computation finds (networkx when it imports, else
    Bron-Kerbosch) on the cases of at most 300 vertices;
  * every graph is where it claims to be: size and words, largest core, number of distinct core values, degree == core
    and two distinct maximum cliques for the tie cases, heuristic < exact and the exact_small_lds verdict for `block`,
    the side of 1024 / 2048 for `big_core`;
  * every graph can catch what it lists: each wrong variant of the restatement changes the order, the clique or the
    largest core number there, and every variant is caught by a case of at most 4097 vertices.  The table is printed.

Rows of the variant table that arithmetic does not allow as first worded (see clique_cases.py): rank16_wrap changes
nothing at any admitted size and is asserted EQUAL at L = 32768, perm_for_rank stands in for it; keep_tail_bits moves
every core number by the same amount, so it shows in the largest core number, not in the order.
"""
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clique_cases as cc  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SMALL = [n for n in cc.NAMES if cc.size_of(n) <= 300]
_refs, _rest = {}, {}


def _clean(name):
    return name[6:] if name.startswith("dirty_") else name


def _ref(qo, name):
    """(core, max_core, heuristic clique) of the oracle, computed once per graph; the oracle reads the bits as they are, so
    a dirty twin is held to its clean case"""
    name = _clean(name)
    if name not in _refs:
        bm = cc.case(name).bitmap
        core, _, mc = qo.kcore(bm)
        _refs[name] = (np.asarray(core, dtype=np.int64), int(mc), qo.max_clique(bm, 1))
    return _refs[name]


def _restated(name):
    if name not in _rest:
        _rest[name] = cc.restate(cc.case(name).bitmap)
    return _rest[name]


def test_mirrored_constants():
    src = open(os.path.join(ROOT, "quatro_amd", "csrc", "solver.hip")).read()
    hdr = open(os.path.join(ROOT, "quatro_amd", "csrc", "solver.h")).read()
    ex = open(os.path.join(ROOT, "quatro_amd", "csrc", "exact.hip")).read()
    capi = open(os.path.join(ROOT, "quatro_amd", "csrc", "capi.hip")).read()
    define = lambda text, name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, text).group(1))
    assert 256 * define(src, "KCL_VPT") == cc.KCL_MAX_L
    assert define(hdr, "CLIQUE_BATCH") == cc.CLIQUE_BATCH and define(src, "RS_BINS") == cc.RS_BINS
    assert define(src, "HCA_MAXITER") == cc.HCA_MAXITER and define(src, "PM2_MAXL") == cc.PM2_MAXL
    assert (define(src, "HCA_CTL_VER"), define(src, "HCA_CTL_VER") + 2 * define(src, "HCA_MAXWG")) == cc.HCA_CTL_WORDS
    for text in ("return max(1280, e ? atoi(e) : 1280);", "return e ? atoi(e) : 8192;", "(size_t)128 * 1024;",
                 "if (W <= 4) LAUNCH_SV_T(k_kcore_levels, 1,", "else if (W <= 16) LAUNCH_SV_T(k_kcore_levels, 4,",
                 "const int npass = NB > RS_BINS ? 2 : 1;", "if (W <= 128) return greedy_descent<2>(",
                 "if (W <= 256) return greedy_descent<4>(", "if (W <= 128) fetch_rows(", "else if (W <= 320) fetch_rows("):
        assert text in src, text
    assert "return W <= 64 ? 1 : W <= 128 ? 2 : W <= 256 ? 4 : W <= 512 ? 8 : 0;" in ex
    assert "return bytes <= (size_t)60 * 1024 ? bytes : 0;" in ex and "((size_t)768 << 20)" in capi
    # the sizes on the edges of the route table take the routes the module's docstring gives them
    assert [cc.levels_vt(L) for L in (256, 257, 512, 513, 768, 769, 1024, 1025, 1280)] == [1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert cc.rows_fit_lds(1024) and not cc.rows_fit_lds(1025) and not cc.rows_fit_lds(1281)
    assert [cc.greedy_width(L) for L in (8192, 8193, 16384, 16385, 20481)] == [2, 4, 4, 8, 8]
    assert [cc.exact_nw(L) for L in (300, 4096, 4097, 8193, 16385, 32768)] == [1, 1, 2, 4, 8, 8]


@pytest.mark.parametrize("name", cc.NAMES)
def test_restatement_equals_the_oracle(qo, name):
    core, mc, heu = _ref(qo, name)
    r = _restated(name)
    assert np.array_equal(r.core, core) and int(r.core.max(initial=0)) == mc
    # the order: core numbers ascending, ids ascending among equals — what the oracle's stable sort by K gives
    assert np.array_equal(r.perm, np.argsort(core, kind="stable"))
    key = core[r.perm] * (core.size + 1) + r.perm
    assert np.all(np.diff(key) > 0)
    assert np.array_equal(r.clique, heu)
    if name.startswith("dirty_"):
        clean = _restated(_clean(name))
        assert all(np.array_equal(a, b) for a, b in zip(r, clean))


@pytest.mark.parametrize("name", SMALL)
def test_exact_restatement_and_an_independent_maximum(qo, name):
    c = cc.case(name)
    want = np.sort(qo.max_clique(cc.case(_clean(name)).bitmap, 0))
    off, nbr = cc.neighbour_lists(c.bitmap)
    r = _restated(name)
    got = cc.restate_exact(off, nbr, r.core + 1, r.perm, r.clique)
    assert np.array_equal(got, want) and cc.is_clique(c.bitmap, want)
    if "omega" in c.claims:
        # complete multipartite (20 ** 6 maximal cliques, beyond enumeration): the parts are independent sets, so a clique
        # takes one vertex of each at the most, and any two vertices of different parts are joined
        for p in range(6):
            part = np.arange(p, 120, 6)
            assert all(not cc.is_clique(c.bitmap, [a, b]) for a in part[:3] for b in part if a != b)
        assert np.array_equal(r.deg, np.full(120, 100))  # 100 = 120 - 20: joined to everything outside its part
        omega = c.claims["omega"]
    else:
        try:
            import networkx as nx
            G = nx.Graph()
            G.add_nodes_from(range(c.claims["L"]))
            G.add_edges_from((v, int(w)) for v in range(c.claims["L"]) for w in nbr[off[v]:off[v + 1]])
            omega = max((len(q) for q in nx.find_cliques(G)), default=0)
        except ImportError:
            omega = cc.bron_kerbosch_omega(c.bitmap)
        omega = omega if omega >= 2 else 0  # (without an edge the reference returns no clique)
    assert want.size == omega


@pytest.mark.parametrize("name", cc.NAMES)
def test_every_case_holds_its_claims(qo, name):
    c = cc.case(name)
    cl = c.claims
    core, mc, heu = _ref(qo, name)
    L = c.bitmap.shape[0]
    assert (L, c.bitmap.shape[1]) == (cl["L"], cl["W"]) == (cc.size_of(name), cc.words(L)) and cl["route"] == cc.route(L)
    assert mc == cl["max_core"]
    assert np.unique(core).size == cl["n_core_values"]
    if "clique" in cl:
        assert np.array_equal(heu, np.sort(cl["clique"]))
    r = _restated(name)
    kind = cl["kind"]
    if kind in ("tie", "complete") or cl.get("degree_is_core"):
        assert np.array_equal(r.deg, core)
    if kind == "tie":
        omega = qo.max_clique(cc.case(_clean(name)).bitmap, 0).size
        wit = [tuple(np.sort(w).tolist()) for w in cl["witnesses"]]
        assert len(set(wit)) >= 2 and omega == heu.size
        assert all(len(w) == omega and cc.is_clique(c.bitmap, w) for w in wit)
        pos = core[core > 0]
        assert pos.size and np.all(pos == mc)  # (the device test's condition: one non-zero core value, above any floor)
    if kind == "complete":
        assert np.all(core == L - 1) and cl["passes"] == (2 if L > cc.RS_BINS else 1)
    if kind == "ladder":
        assert set(np.unique(core[core > 0]).tolist()) == set(range(1, mc + 1))
    if kind == "big_core":
        assert cl["passes"] == (2 if mc + 1 > cc.RS_BINS else 1) and cl["digit_values"] == (mc >> 10) + 1
        assert (mc + 1 > 2048) == (cl["digit_values"] == 3) and L > cc.KCL_MAX_L
    if kind == "fallback" and "hindex_rounds" in cl:
        assert (cl["hindex_rounds"] > cc.HCA_MAXITER) == (L == 16385) and (L > cc.Q_IN_LDS_MAX_L) == (L == 16385)
    if kind == "block":
        exact = qo.max_clique(c.bitmap, 0)
        tail = int(np.sum(core + 1 > heu.size))
        assert heu.size == cl["heuristic"] < cl["exact"] == exact.size and cc.is_clique(c.bitmap, exact)
        assert tail == cl["tail"]
        assert (cc.exact_small_lds(L, L - tail, mc) > 0) == cl["small_lds"]
    if name.startswith("dirty_"):
        clean = cc.case(_clean(name)).bitmap
        i = np.arange(L)
        assert L % 64 in (1, 63) and not np.array_equal(clean, c.bitmap)
        assert np.all((c.bitmap[i, i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1))
        assert np.all(c.bitmap[:, -1] >> np.uint64(L % 64) == (np.uint64(1) << np.uint64(64 - L % 64)) - np.uint64(1))
        assert not np.any((clean[i, i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1))
        assert not np.any(clean[:, -1] >> np.uint64(L % 64))


def _variant(name, v):
    """what the wrong variant v makes of the case, and what the right operation does"""
    c = cc.case(name)
    r = _restated(name)
    if v == "first_maximum_not_canonical":
        off, nbr = cc.neighbour_lists(c.bitmap)
        right = cc.restate_exact(off, nbr, r.core + 1, r.perm, r.clique)
        wrong = cc.restate_exact(off, nbr, r.core + 1, r.perm, r.clique, v)
        assert wrong.size == right.size and cc.is_clique(c.bitmap, wrong)  # a maximum clique, only not the first
        return not np.array_equal(right, wrong)
    return cc.differs(cc.restate(c.bitmap, v), r)


def test_every_case_changes_under_the_variants_it_lists(capsys):
    names = [n for n in cc.NAMES if cc.case(n).variants]
    assert all(cc.size_of(n) <= 4097 for n in names)
    table = {n: {v: _variant(n, v) for v in cc.case(n).variants} for n in names}
    with capsys.disabled():
        print("\nvariant by case (x: the case lists the variant and changes under it)")
        print(" " * 28 + " ".join(f"{i:>2d}" for i in range(len(cc.VARIANTS))) + "   " +
              ", ".join(f"{i} {v}" for i, v in enumerate(cc.VARIANTS)))
        for n in names:
            print(f"{n:28s}" + " ".join(" x" if table[n].get(v) else " ." for v in cc.VARIANTS))
    missed = [(n, v) for n in names for v, hit in table[n].items() if not hit]
    assert not missed, missed
    for v in cc.VARIANTS:
        assert any(table[n].get(v) for n in names), v


def test_rank16_wrap_cannot_show_at_any_admitted_size():
    """ranks end at 32767 where qtr_create's largest max_corr ends: int16 holds them all"""
    c = cc.case("planted_32768")
    assert c.claims["L"] == cc.PM2_MAXL == 32768
    assert not cc.differs(cc.restate(c.bitmap, "rank16_wrap"), _restated("planted_32768"))


def test_oracle_time_on_the_largest_case(qo, capsys):
    c = cc.case("planted_32768")
    t = time.perf_counter()
    qo.kcore(c.bitmap)
    heu = qo.max_clique(c.bitmap, 1)
    dt = time.perf_counter() - t
    with capsys.disabled():
        print(f"\noracle on planted_32768 (core numbers + heuristic): {dt:.2f} s, clique {heu.size}")
    assert heu.size == cc.PLANTED_K
