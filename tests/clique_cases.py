"""Named graphs for the clique stage of quatro_amd/csrc/solver.hip and exact.hip (core numbers, the (core, id) ranking,
the rank-relabelled matrix, the PMC heuristic, the exact search), each placed at a constant the host code or a kernel
branches on.  A plain module: deterministic numpy generators with fixed seeds, no fixtures, no GPU work.  Used by
tests/test_clique_cases_cpu.py (the restatement below against the oracle, every graph against what it claims, every graph
against the wrong variants it was built to catch), tests/test_gpu_clique_cases.py (the device against the oracle through
qtr_max_clique and through lane groups of qtr_submit_batch) and tests/gpu_clique_engines.py (the comparison engines).

    case(name) -> Case(name, bitmap uint64 [L][ceil(L / 64)], claims dict, variants tuple)

The stage is exact by contract: nothing here has a tolerance.  Graphs are built from edge lists straight into the bit
matrix (np.bitwise_or.at on (row, column word), both directions; a clique ORs its member mask into its members' rows);
no dense L x L array is ever made.

Thresholds, re-read from the code, and the sizes that sit on them (W = ceil(L / 64)):

  clique_stage_launch (solver.hip)
    kc_single_wave = L <= 256 * KCL_VPT = 1280: k_kcore_levels<VT> + k_kcore_collect_rank, else k_hcore_async (L > 1280,
      hcore_min_l) + k_rank_sort with the peeling workgroup d_kcore riding in it             -> 1280 | 1281
    k_kcore_levels<VT>: VT = 1 for W <= 4, 2 for W <= 8, 3 for W <= 12, 4 for W <= 16, else 5
                                                                  -> 256 | 257, 512 | 513, 768 | 769, 1024 | 1025
    merged_first_round = kc_single_wave and L * W * 8 + 16 * L <= 150 KB: 1024 (147 456 bytes) holds, 1025 (155 800)
      does not; a second k_clique_batch_lds round only for L > CLIQUE_BATCH = 1024            -> 1024 | 1025
    lds_rows (k_clique_batch_lds) under the same 150 KB formula: for 1025 <= L <= 1280 the levels path is followed by
      k_clique_first + k_clique_batch                                                         -> 1025, 1280
    scout workgroup of k_hcore_async: G == 1 and 8192 < L <= 32768                            -> 8192 | 8193
    q_in_lds = 8 * L <= 128 KB (the peeling workgroup's queue; the global-queue form above)   -> 16384 | 16385
    k_permute_scatter for L <= PM2_MAXL = 32768, 16-bit ranks; qtr_create admits max_corr <= 32768, so k_permute is
      not reachable                                                                           -> 32768
  k_rank_sort: NB = max_core + 1; two radix passes of ten bits when NB > RS_BINS = 1024; the second pass has
    ((NB - 1) >> 10) + 1 digit values    -> cliques of 1023, 1024 (NB = 1024, one pass), 1025, 1026 (two passes, two
    digit values), 2049 (NB = 2049: three digit values), K_1281 (NB = 1281, one occupied bin per pass)
  greedy_dispatch<2 | 4 | 8>: W <= 128, <= 256, above; k_clique_first's row fetch: W <= 128, <= 320, above
                                                      -> 8192 | 8193, 16384 | 16385, 20480 | 20481
  k_hcore_async gives up after HCA_MAXITER = 4096 iterations: a path needs L / 2 of them      -> path(16385)
  exact_nw (exact.hip): words of the FULL row W <= 64 -> 1, <= 128 -> 2, <= 256 -> 4, <= 512 -> 8
                                     -> block at 300 (1), 4097 (2), 8193 (4), 16385 (8, and the 768 MB scratch cap)
  exact_small_lds: with w0 = t0 >> 6, Wq = W - w0, n = L - 64 * w0, depth = max_core + 2: the LDS kernel runs when
    Wq <= 64 and (n * Wq + depth * Wq) * 8 + (depth + 2) * 4 <= 60 KB                         -> block(300) yes, others no

Where the issue's text and the code disagree the code wins; two places did.  (1) At every size it names for last_word
(65, 1025, 1281, 8193) the last, partial column word holds ONE vertex, L - 1, so no clique can lie inside it: last_word(L)
is two cliques of twelve instead, ids 0 .. 11 and ids L - 12 .. L - 1, whose tie is decided by the one column that lives
in the last word (the canonical order starts from L - 1 and finds the second; without the last word the second has eleven
members and the first wins).  (2) The inverse permutation of k_permute_scatter holds RANKS, at most 32767: they fit
int16 as well as uint16, so `rank16_wrap` cannot show at any size qtr_create admits; the CPU test asserts exactly that at
L = 32768, and `perm_for_rank` (the permutation used where its inverse belongs, the other way to get that table wrong)
takes its place in the table of variants that must be caught.

restate() restates the stage in numpy / pure Python, with the order as an input: restate_cores (peeling by levels),
restate_perm (np.lexsort((ids, core))), restate_heuristic (the oracle's heu_search with its acceptance rules: starts from
the back of perm, candidates with K > mc only, a start needs more candidates than mc, picks by highest rank, a clique is
accepted only when strictly larger, the search ends at max_core + 1) and restate_exact (roots ascending in rank,
children descending, the incumbent changes on a strictly larger clique only).  `variant` names deliberately wrong forms.
"""
from collections import namedtuple

import numpy as np

u64 = np.uint64
Case = namedtuple("Case", "name bitmap claims variants")

# ---------------------------------------------------------------------------------------------- mirrored constants
KCL_MAX_L = 1280          # solver.hip: 256 * KCL_VPT, the levels path; k_hcore_async above
CLIQUE_BATCH = 1024
RS_BINS = 1024
HCA_MAXITER = 4096
HCA_CTL_WORDS = (64, 1088)  # k_hcore_async's control words in perm[]
SCOUT_MIN_L = 8192
Q_IN_LDS_MAX_L = 16384
PM2_MAXL = 32768
LDS_BUDGET = 150 * 1024
EXACT_SMALL_LDS_BYTES = 60 * 1024

VARIANTS = ("ties_descending", "ties_by_degree", "core_low10", "core_low11", "drop_last_word", "keep_tail_bits",
            "self_loops_count", "first_maximum_not_canonical", "start_top_only", "perm_for_rank")
UNCATCHABLE = ("rank16_wrap",)  # see the module docstring


def words(L):
    return (L + 63) // 64


def levels_vt(L):
    W = words(L)
    return 1 if W <= 4 else 2 if W <= 8 else 3 if W <= 12 else 4 if W <= 16 else 5


def rows_fit_lds(L):
    return L * words(L) * 8 + 16 * L <= LDS_BUDGET


def rank_sort_passes(max_core):
    return 2 if max_core + 1 > RS_BINS else 1


def greedy_width(L):
    W = words(L)
    return 2 if W <= 128 else 4 if W <= 256 else 8


def exact_nw(L):
    W = words(L)
    return 1 if W <= 64 else 2 if W <= 128 else 4 if W <= 256 else 8 if W <= 512 else 0


def exact_small_lds(L, t0, max_core):
    """bytes of the LDS kernel of the exact search (0: the wide kernel runs); t0 = the first rank with core + 1 above the
    heuristic's size, depth_cap = ub + 1 = max_core + 2"""
    W, depth = words(L), max_core + 2
    w0 = t0 >> 6
    Wq, n = W - w0, L - (w0 << 6)
    if Wq < 1 or Wq > 64:
        return 0
    b = (n * Wq + depth * Wq) * 8 + (depth + 2) * 4
    return b if b <= EXACT_SMALL_LDS_BYTES else 0


def route(L):
    """the kernels clique_stage_launch enqueues for one graph of L vertices handed to qtr_max_clique"""
    if L <= KCL_MAX_L:
        cores = f"k_kcore_levels<{levels_vt(L)}> + k_kcore_collect_rank"
        if rows_fit_lds(L):
            rounds = "k_clique_batch_lds x 1 (merged)" if L <= CLIQUE_BATCH else "k_clique_batch_lds x 2 (merged)"
        else:
            rounds = "k_clique_first + k_clique_batch"
    else:
        cores = "k_hcore_async" + (" + scout" if SCOUT_MIN_L < L <= 32768 else "") + " + k_rank_sort (d_kcore " + \
            ("LDS queue" if L <= Q_IN_LDS_MAX_L else "global queue") + " if it gives up)"
        rounds = "k_clique_batch_lds x 2" if rows_fit_lds(L) else f"k_clique_first + k_clique_batch, greedy<{greedy_width(L)}>"
    return f"{cores}; k_permute_scatter; {rounds}; exact width {exact_nw(L)}"


# ---------------------------------------------------------------------------------------------- building
def _seed(name):
    return [ord(c) for c in name]


def _empty(L):
    return np.zeros((L, words(L)), dtype=u64)


def add_edges(bm, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    for a, b in ((e[:, 0], e[:, 1]), (e[:, 1], e[:, 0])):
        np.bitwise_or.at(bm, (a, b >> 6), u64(1) << (b & 63).astype(u64))
    return bm


def add_clique(bm, members):
    m = np.asarray(members, dtype=np.int64)
    mask = np.zeros(bm.shape[1], dtype=u64)
    np.bitwise_or.at(mask, m >> 6, u64(1) << (m & 63).astype(u64))
    bm[m] |= mask
    bm[m, m >> 6] &= ~(u64(1) << (m & 63).astype(u64))
    return bm


def _background(bm, n_edges, rng):
    L = bm.shape[0]
    if L >= 2 and n_edges > 0:
        add_edges(bm, rng.integers(0, L, size=(n_edges, 2)))
    return bm


def _members(L, k, rng):
    """k seeded ids that always include vertex 0 and vertex L - 1"""
    k = min(k, L)
    if k <= 1:
        return np.arange(k)
    if k == L:
        return np.arange(L)
    inner = rng.choice(np.arange(1, L - 1), size=k - 2, replace=False)
    return np.sort(np.r_[0, inner, L - 1])


def is_clique(bm, ids):
    ids = np.asarray(ids, dtype=np.int64)
    if len(set(ids.tolist())) != ids.size:
        return False
    sub = (bm[np.ix_(ids, ids >> 6)] >> (ids & 63).astype(u64)[None, :]) & u64(1)
    return int(sub.sum() - np.trace(sub)) == ids.size * (ids.size - 1)  # (a dirty twin's diagonal does not count)


def dirty_bitmap(bm):
    """the same graph with every diagonal bit set and the bits past column L of the last word set: both are ignored by
    contract (test_max_clique_entry_hygiene_and_errors)"""
    L = bm.shape[0]
    d = bm.copy()
    i = np.arange(L)
    d[i, i >> 6] |= u64(1) << (i & 63).astype(u64)
    if L & 63:
        d[:, -1] |= ~((u64(1) << u64(L & 63)) - u64(1))
    return d


# ---------------------------------------------------------------------------------------------- the cases
LADDER = (1, 2, 3, 63, 64, 65, 256, 257, 512, 513, 768, 769, 1024, 1025, 1280, 1281, 4096, 4097, 8192, 8193, 16384, 16385,
          20480, 20481)
PLANTED_K = 24
# distinct core values of the seeded backgrounds: counted once with the oracle and fixed here (the generators are
# deterministic: np.random.default_rng on the case's name)
N_CORE_VALUES = {
    "planted_63": 5, "planted_64": 6, "planted_65": 6, "planted_256": 6, "planted_257": 6, "planted_512": 5, "planted_513": 5,
    "planted_768": 6, "planted_769": 6, "planted_1024": 6, "planted_1025": 6, "planted_1280": 6, "planted_1281": 6,
    "planted_4096": 6, "planted_4097": 6, "planted_8192": 6, "planted_8193": 6, "planted_16384": 6, "planted_16385": 6,
    "planted_20480": 6, "planted_20481": 6, "planted_32768": 6, "big_core_1023_1400": 7, "big_core_1024_1400": 8,
    "big_core_1025_1400": 9, "big_core_1026_1400": 7, "big_core_2049_2200": 8, "block_300": 10, "block_4097": 18,
    "block_8193": 18, "block_16385": 14}
BLOCK_SEED = {300: 0, 4097: 0, 8193: 0, 16385: 0}
BLOCK_SHAPES = ((300, 120, 0.5), (4097, 1200, 0.1), (8193, 1200, 0.1), (16385, 1200, 0.1))
# heuristic size, exact size, #{core + 1 > heuristic}: counted once with the oracle and fixed here
BLOCK_CLAIMS = {300: dict(max_core=50, heuristic=9, exact=10, tail=120, small_lds=True),
                4097: dict(max_core=100, heuristic=5, exact=6, tail=2569, small_lds=False),
                8193: dict(max_core=100, heuristic=5, exact=6, tail=1222, small_lds=False),
                16385: dict(max_core=99, heuristic=5, exact=6, tail=1200, small_lds=False)}

_builders = {}
_cache = {}


def _case(name, variants=()):
    def deco(f):
        _builders[name] = (f, tuple(variants))
        return f
    return deco


def _base_claims(L, **kw):
    c = dict(L=L, W=words(L), route=route(L))
    c.update(kw)
    return c


def _planted(L):
    name = f"planted_{L}"
    rng = np.random.default_rng(_seed(name))
    bm = _background(_empty(L), 3 * L, rng)
    k = min(PLANTED_K, L)
    mem = _members(L, k, rng)
    add_clique(bm, mem)
    # (a single vertex: no start has more candidates than the bound 0, the reference returns no clique)
    claims = _base_claims(L, max_core=k - 1, clique=mem if L >= 2 else mem[:0], kind="planted")
    if L <= 3:  # 3 L random pairs on two or three vertices give every edge (checked by the claim itself)
        claims["n_core_values"] = 1
    return bm, claims


for _L in LADDER + (32768,):
    _v = () if _L < 2 or _L > 4097 else ("ties_descending",) if _L <= 3 else ("ties_descending", "ties_by_degree")
    if 2 <= _L <= 4097 and _L % 64 != 1:
        _v += ("drop_last_word",)
    _case(f"planted_{_L}", _v)(lambda L=_L: _planted(L))


def _last_word(L):
    assert L % 64 == 1 and L >= 65
    bm = _empty(L)
    a, b = np.arange(12), np.arange(L - 12, L)
    add_clique(bm, a)
    add_clique(bm, b)
    return bm, _base_claims(L, max_core=11, n_core_values=2, clique=b, kind="tie", witnesses=(a, b))


for _L in (65, 1025, 1281, 8193):
    _case(f"last_word_{_L}", ("drop_last_word", "ties_descending") if _L <= 4097 else ())(lambda L=_L: _last_word(L))


def _big_core(L, k):
    name = f"big_core_{k}_{L}"
    rng = np.random.default_rng(_seed(name))
    bm = _background(_empty(L), L, rng)
    mem = _members(L, k, rng)
    add_clique(bm, mem)
    return bm, _base_claims(L, max_core=k - 1, clique=mem, kind="big_core", passes=rank_sort_passes(k - 1),
                            digit_values=((k - 1) >> 10) + 1 if k > RS_BINS else 1)


for _k, _L in ((1023, 1400), (1024, 1400), (1025, 1400), (1026, 1400), (2049, 2200)):
    _v = ("ties_descending", "ties_by_degree", "drop_last_word") + \
        (() if _k <= 1024 else ("core_low10", "core_low11") if _k == 2049 else ("core_low10",))
    _case(f"big_core_{_k}_{_L}", _v)(lambda L=_L, k=_k: _big_core(L, k))


def _complete(L):
    bm = add_clique(_empty(L), np.arange(L))
    return bm, _base_claims(L, max_core=L - 1, n_core_values=1, clique=np.arange(L), kind="complete",
                            passes=rank_sort_passes(L - 1))


for _L in (65, 1025, 1281):
    _case(f"complete_{_L}", ("ties_descending",))(lambda L=_L: _complete(L))


def _equal_cliques(L, m, k):
    """m disjoint k-cliques at interleaved ids spread over [0, L - 1] among isolated vertices: member i of clique j is the
    (i * m + j)-th of m * k evenly spaced ids, so clique m - 1 holds L - 1, the top of the canonical order"""
    ids = np.round(np.arange(m * k) * ((L - 1) / (m * k - 1))).astype(np.int64)
    assert np.unique(ids).size == m * k and ids[-1] == L - 1
    bm = _empty(L)
    cl = [ids[j::m] for j in range(m)]
    for c in cl:
        add_clique(bm, c)
    return bm, _base_claims(L, max_core=k - 1, n_core_values=2, clique=cl[-1], kind="tie", witnesses=tuple(cl))


for _m, _k, _Ls in ((5, 12, (1024, 1280, 1281, 1600)), (3, 40, (1281, 4097))):
    for _L in _Ls:
        _case(f"equal_cliques_{_m}x{_k}_{_L}", ("ties_descending", "drop_last_word"))(
            lambda L=_L, m=_m, k=_k: _equal_cliques(L, m, k))


def _cycle(L):
    i = np.arange(L)
    bm = add_edges(_empty(L), np.stack([i, (i + 1) % L], 1))
    # the start at the top of the order, L - 1, ranks its two neighbours L - 2 above 0
    return bm, _base_claims(L, max_core=2, n_core_values=1, clique=np.array([L - 2, L - 1]), kind="tie",
                            witnesses=(np.array([0, 1]), np.array([L - 2, L - 1])), n_maximum=L)


def _bipartite(L):
    """even ids against odd ids, a = L // 2 a side; an odd L leaves its last vertex isolated"""
    a = L // 2
    ev, od = np.arange(0, 2 * a, 2), np.arange(1, 2 * a, 2)
    bm = _empty(L)
    for side, other in ((ev, od), (od, ev)):
        mask = np.zeros(bm.shape[1], dtype=u64)
        np.bitwise_or.at(mask, other >> 6, u64(1) << (other & 63).astype(u64))
        bm[side] |= mask
    top = 2 * a - 1
    return bm, _base_claims(L, max_core=a, n_core_values=1 if L == 2 * a else 2, clique=np.array([top - 1, top]), kind="tie",
                            witnesses=(np.array([0, 1]), np.array([top - 1, top])), n_maximum=a * a)


for _L in (64, 65, 1025, 1281):
    _case(f"cycle_{_L}", ("ties_descending",) + (("drop_last_word",) if _L == 64 else ()))(lambda L=_L: _cycle(L))
    _case(f"bipartite_{_L}", ("ties_descending",) + (("drop_last_word",) if _L == 64 else ("perm_for_rank",)))(
        lambda L=_L: _bipartite(L))


@_case("multipartite_6x20", ("ties_descending", "drop_last_word"))
def _multipartite():
    """complete 6-partite, part p = ids p, p + 6, ...: a clique takes at most one vertex of a part, and one of each is a
    clique, so omega = 6 with 20 ** 6 maximum cliques; the canonical search returns the six highest ids"""
    L = 120
    bm = add_clique(_empty(L), np.arange(L))
    for p in range(6):
        part = np.arange(p, L, 6)
        mask = np.zeros(bm.shape[1], dtype=u64)
        np.bitwise_or.at(mask, part >> 6, u64(1) << (part & 63).astype(u64))
        bm[part] &= ~mask
    return bm, _base_claims(L, max_core=100, n_core_values=1, clique=np.arange(114, 120), kind="tie", omega=6,
                            witnesses=(np.arange(6), np.arange(114, 120)), n_maximum=20 ** 6)


def _ladder(m, L):
    """disjoint K_2, K_3, ..., K_m at consecutive ids, isolated vertices behind them: every core value 1 .. m - 1 (and 0
    where L leaves room) is occupied"""
    bm = _empty(L)
    at = 0
    for j in range(2, m + 1):
        add_clique(bm, np.arange(at, at + j))
        at += j
    assert at == m * (m + 1) // 2 - 1 <= L
    return bm, _base_claims(L, max_core=m - 1, n_core_values=m - 1 + (1 if L > at else 0), clique=np.arange(at - m, at),
                            kind="ladder", degree_is_core=True)


for _L in (1225, 1280, 1281):
    _case(f"ladder_49_{_L}", ("ties_descending",) + (("drop_last_word",) if _L != 1281 else ()))(lambda L=_L: _ladder(49, L))


def _path(L):
    i = np.arange(L - 1)
    bm = add_edges(_empty(L), np.stack([i, i + 1], 1))
    return bm, _base_claims(L, max_core=1, n_core_values=1, clique=np.array([L - 2, L - 1]), kind="fallback",
                            hindex_rounds=L // 2)


def _star(L, centre):
    leaves = np.setdiff1d(np.arange(L), [centre])
    bm = add_edges(_empty(L), np.stack([np.full(L - 1, centre), leaves], 1))
    # every core number is 1: the top of the order is L - 1; from a leaf the only candidate is the centre
    other = L - 2 if centre == L - 1 else centre
    return bm, _base_claims(L, max_core=1, n_core_values=1, clique=np.array([other, L - 1]), kind="fallback")


def _matching(L):
    i = np.arange(0, L - 1, 2)
    bm = add_edges(_empty(L), np.stack([i, i + 1], 1))
    top = i[-1] + 1
    return bm, _base_claims(L, max_core=1, n_core_values=1 if L % 2 == 0 else 2, clique=np.array([top - 1, top]),
                            kind="fallback")


def _no_edges(L):
    return _empty(L), _base_claims(L, max_core=0, n_core_values=1, clique=np.zeros(0, dtype=np.int64), kind="fallback")


for _L in (1281, 4097):
    _case(f"path_{_L}", ("ties_descending", "ties_by_degree"))(lambda L=_L: _path(L))
    _case(f"star_first_{_L}", ("ties_descending", "ties_by_degree"))(lambda L=_L: _star(L, 0))
    _case(f"star_last_{_L}", ("ties_descending",))(lambda L=_L: _star(L, L - 1))
    _case(f"matching_{_L}", ("ties_descending",))(lambda L=_L: _matching(L))
    _case(f"empty_{_L}", ("ties_descending",))(lambda L=_L: _no_edges(L))
_case("path_16385")(lambda: _path(16385))


def _block(L, n, p):
    """n vertices at sorted random ids carry G(n, p); 3 L random edges surround them"""
    name = f"block_{L}"
    rng = np.random.default_rng(_seed(name) + [BLOCK_SEED[L]])
    bm = _background(_empty(L), 3 * L, rng)
    ids = np.sort(rng.choice(L, size=n, replace=False))
    iu = np.triu_indices(n, 1)
    keep = rng.random(iu[0].size) < p
    add_edges(bm, np.stack([ids[iu[0][keep]], ids[iu[1][keep]]], 1))
    return bm, _base_claims(L, kind="block", block_ids=ids, **BLOCK_CLAIMS.get(L, {}))


for _L, _n, _p in BLOCK_SHAPES:
    _v = () if _L > 4097 else ("ties_descending", "ties_by_degree", "drop_last_word", "start_top_only", "perm_for_rank") + \
        (("first_maximum_not_canonical",) if _L == 300 else ())
    _case(f"block_{_L}", _v)(lambda L=_L, n=_n, p=_p: _block(L, n, p))

DIRTY_OF = [f"planted_{L}" for L in LADDER if L % 64 in (1, 63)] + [f"last_word_{L}" for L in (65, 1025, 1281, 8193)]
CLEAN_NAMES = list(_builders)
NAMES = CLEAN_NAMES + ["dirty_" + n for n in DIRTY_OF]
DIRTY_VARIANTS = ("keep_tail_bits", "self_loops_count")


def case(name):
    if name in _cache:
        return _cache[name]
    if name.startswith("dirty_"):
        base = case(name[6:])
        L = base.claims["L"]
        # a single vertex has no neighbour whatever the bits say, but both variants count some
        c = Case(name, dirty_bitmap(base.bitmap), dict(base.claims, dirty_of=base.name),
                 DIRTY_VARIANTS if L <= 4097 else ())
    else:
        f, variants = _builders[name]
        bm, claims = f()
        if "n_core_values" not in claims and name in N_CORE_VALUES:
            claims["n_core_values"] = N_CORE_VALUES[name]
        c = Case(name, bm, claims, variants)
    c.bitmap.setflags(write=False)
    if c.claims["L"] <= 4097:
        _cache[name] = c
    return c


def size_of(name):
    """L of a case without building it"""
    return int(name.rsplit("_", 1)[1]) if not name.startswith("multipartite") else 120


# ---------------------------------------------------------------------------------------------- the restatement
def neighbour_lists(bm, variant=None):
    """-> (offsets int64 [L + 1], neighbour ids int64) of the graph the bit matrix stands for: the diagonal and the bits
    past column L do not count.  drop_last_word: the last column word is not read; keep_tail_bits: bits past column L
    are neighbours (that nobody ever removes); self_loops_count: a diagonal bit is a neighbour"""
    L, W = bm.shape
    off = np.zeros(L + 1, dtype=np.int64)
    parts = []
    step = max(1, (1 << 25) // max(1, W * 64))
    for r0 in range(0, L, step):
        blk = bm[r0:r0 + step]
        bits = np.unpackbits(np.ascontiguousarray(blk).view(np.uint8), axis=1, bitorder="little")
        if variant == "drop_last_word":
            bits[:, (W - 1) * 64:] = 0
        if variant != "keep_tail_bits":
            bits[:, L:] = 0
        if variant != "self_loops_count":
            r = np.arange(blk.shape[0])
            bits[r, r0 + r] = 0
        rr, cc = np.nonzero(bits)
        off[r0 + 1:r0 + 1 + blk.shape[0]] = np.bincount(rr, minlength=blk.shape[0])
        parts.append(cc.astype(np.int64))
    return np.cumsum(off), (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64))


def _gather(off, nbr, vs):
    """the neighbour ids of every vertex of vs, concatenated"""
    cnt = off[vs + 1] - off[vs]
    tot = int(cnt.sum())
    if tot == 0:
        return np.zeros(0, dtype=np.int64)
    start = np.repeat(off[vs] - np.r_[0, np.cumsum(cnt)[:-1]], cnt)
    return nbr[start + np.arange(tot)]


def restate_cores(off, nbr):
    """core numbers by peeling level by level -> (core int64 [L], degree int64 [L])"""
    L = off.size - 1
    n = max(L, int(nbr.max()) + 1 if nbr.size else 0)  # (keep_tail_bits: ids past L, never removed)
    deg0 = np.diff(off)
    deg = np.zeros(n, dtype=np.int64)
    deg[:L] = deg0
    alive = np.zeros(n, dtype=bool)
    alive[:L] = True
    core = np.zeros(L, dtype=np.int64)
    left, k = L, 0
    while left:
        k = max(k, int(deg[alive].min()))
        front = np.nonzero(alive & (deg <= k))[0]
        while front.size:
            core[front] = k
            alive[front] = False
            left -= front.size
            deg -= np.bincount(_gather(off, nbr, front), minlength=n)
            front = np.nonzero(alive & (deg <= k))[0]
    return core, deg0


def restate_perm(core, variant=None, deg=None):
    """vertex id at each rank of the (core, id) order"""
    core = np.asarray(core, dtype=np.int64)
    ids = np.arange(core.size)
    if variant == "ties_descending":
        return np.lexsort((-ids, core))
    if variant == "ties_by_degree":
        return np.lexsort((ids, deg, core))
    if variant == "core_low10":
        return np.lexsort((ids, core & 1023))
    if variant == "core_low11":
        return np.lexsort((ids, core & 2047))
    return np.lexsort((ids, core))


def restate_heuristic(off, nbr, K, perm, variant=None):
    """the oracle's heu_search (K = core + 1) -> the clique's ids, ascending"""
    L = K.size
    rank = np.empty(L, dtype=np.int64)
    rank[perm] = np.arange(L)
    if variant == "rank16_wrap":
        rank = rank.astype(np.int16).astype(np.int64)
    if variant == "perm_for_rank":
        rank = np.asarray(perm, dtype=np.int64)
    Kp = K[perm]
    ub = int(K.max()) if L else 0
    mc, best = 0, np.zeros(0, dtype=np.int64)
    mark = np.zeros(max(L, int(nbr.max()) + 1 if nbr.size else 0), dtype=bool)
    i = L - 1
    while i >= 0 and mc < ub:
        live = np.nonzero(Kp[:i + 1] > mc)[0]  # the starts left under the current bound, in rank order
        if variant == "start_top_only":
            live = live[live == L - 1]
        i = -1
        for j in live[::-1]:  # (the bound stands until a start is accepted)
            v = perm[j]
            P = nbr[off[v]:off[v + 1]]
            P = P[P < L]
            P = P[K[P] > mc]
            if P.size <= mc:
                continue
            P = P[np.argsort(rank[P], kind="stable")]
            picks = []
            while P.size:
                u = P[-1]
                picks.append(int(u))
                nu = nbr[off[u]:off[u + 1]]
                mark[nu] = True
                P = P[:-1]
                P = P[mark[P] & (K[P] > mc)]
                mark[nu] = False
            if 1 + len(picks) > mc:
                mc = 1 + len(picks)
                best = np.sort(np.array(picks + [int(v)], dtype=np.int64))
                i = j - 1
                break
    return best


def restate_exact(off, nbr, K, perm, heu, variant=None):
    """the oracle's exact_improve: the heuristic's clique unless a strictly larger one exists among the vertices with
    K > |heu|, then the FIRST of the largest size in the order roots ascending in rank, children descending
    (first_maximum_not_canonical: the last).  Sorted ids.  Python integers as bit sets: for tails of a few hundred."""
    lb = heu.size
    if lb >= int(K.max()):
        return np.sort(heu)
    verts = [int(v) for v in perm if K[v] > lb]
    n = len(verts)
    pos = {v: i for i, v in enumerate(verts)}
    adj = [0] * n
    for i, v in enumerate(verts):
        for w in nbr[off[v]:off[v + 1]].tolist():
            j = pos.get(w)
            if j is not None and j != i:
                adj[i] |= 1 << j
    last = variant == "first_maximum_not_canonical"
    best, bestC, C = lb, None, []

    def colours(P, limit):
        c = 0
        while P:
            c += 1
            if c > limit:
                return c
            q = P
            while q:
                v = q.bit_length() - 1
                q &= ~(1 << v) & ~adj[v]
                P &= ~(1 << v)
        return c

    def expand(P):
        nonlocal best, bestC
        while P:
            room = best - len(C) - (1 if last and bestC is not None else 0)
            if bin(P).count("1") <= room or colours(P, room) <= room:
                return
            u = P.bit_length() - 1
            P &= ~(1 << u)
            C.append(u)
            R = P & adj[u]
            if not R:
                if len(C) > best or (last and bestC is not None and len(C) == best):
                    best, bestC = len(C), list(C)
            else:
                expand(R)
            C.pop()

    for r in range(n):
        if K[verts[r]] <= best - (1 if last and bestC is not None else 0):
            continue
        C[:] = [r]
        P = adj[r] >> (r + 1) << (r + 1)
        if P:
            expand(P)
    if bestC is None:
        return np.sort(heu)
    return np.sort(np.array([verts[c] for c in bestC], dtype=np.int64))


Restated = namedtuple("Restated", "core deg perm clique")


def differs(a, b):
    """a variant is caught when it changes something the device test asserts: the order, the clique or the largest core"""
    return not (np.array_equal(a.perm, b.perm) and np.array_equal(a.clique, b.clique) and
                int(a.core.max(initial=0)) == int(b.core.max(initial=0)))


def restate(bm, variant=None):
    """-> Restated(core, degree, perm, heuristic clique) of the right operation, or of a wrong variant of it"""
    assert variant is None or variant in VARIANTS + UNCATCHABLE
    off, nbr = neighbour_lists(bm, variant)
    core, deg = restate_cores(off, nbr)
    perm = restate_perm(core, variant, deg)
    clique = restate_heuristic(off, nbr, core + 1, perm, variant)
    return Restated(core, deg, perm, clique)


def bron_kerbosch_omega(bm):
    """size of a largest clique by Bron-Kerbosch with pivoting over every maximal clique (for a few hundred vertices)"""
    off, nbr = neighbour_lists(bm)
    N = [set(nbr[off[v]:off[v + 1]].tolist()) for v in range(bm.shape[0])]
    best = 0
    stack = [(set(), set(range(bm.shape[0])), set())]
    while stack:
        R, P, X = stack.pop()
        if not P and not X:
            best = max(best, len(R))
            continue
        if not P:
            continue
        piv = max(P | X, key=lambda u: len(N[u] & P))
        for v in list(P - N[piv]):
            stack.append((R | {v}, P & N[v], X & N[v]))
            P = P - {v}
            X = X | {v}
    return best
