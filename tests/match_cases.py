"""Named cloud pairs for the matcher of quatro_amd/csrc/match.hip (k_half_tables, k_nn_f16, k_nn_finish_f16,
k_recheck_filter, k_hit_compact, the fused tail k_cross_multi / k_tuple / k_pairs_multi, the six-launch tail above
TAIL_MAXWG * 512 rows) and clouds for the matcher mean (d_seq_mean of frontend.hip): sizes on both sides of every tile,
slice, list and workgroup boundary, ties and duplicates that are exact by construction, rows without a candidate.  A plain
module: deterministic numpy generators, no fixtures, no GPU work.  Used by tests/test_match_cases_cpu.py (the oracle
against the restatement of tests/match_restate.py, the pairs against what they claim) and tests/test_gpu_match_cases.py
(the device against the oracle, no tolerance anywhere).

    case(name) -> MatchCase(xyz_s, desc_s, xyz_t, desc_t, params, claims)

xyz_* is [n, 4] binary32, desc_* [n, 33] binary32; params is a tuple of settings to run the pair under (dicts with
crosscheck, tuple_test, tuple_scale, seed); claims says what the case is there for, and the CPU test asserts every entry:

    n_large, n_small, swapped   sizes of the larger / smaller cloud; swapped: the target is the larger one
    nhit                        rows of the larger cloud that some row of the smaller cloud answers
    hidden_large, hidden_small  rows whose 33 values repeat an earlier row of the same cloud bit for bit
    device_hidden_large         ... of which the device hides fewer where two different rows collide in its duplicate table
    unsafe                      some value lies outside the f16 filter's guard (|v| <= 255, |row|^2 < 65000; a NaN does)
    plan256                     the two plan words of k_nn_f16 (slices | tiles per slice << 8) with 256 workgroups, written
                                out by hand from PLAN_256; the mirror of nn_plan_single must give the same
    nn_large_of_small           {row of the smaller cloud: its answer}                (where the case builds it)
    nn_small_of_large           {row of the larger cloud: its answer, -1 not asked}   (where the case builds it)
    attain0, attain1            {query row: how many base rows attain its minimum} for direction 0 (queries: the smaller
                                cloud) and direction 1 (queries: rows of the larger cloud); 0: no candidate
    mutual_rows                 the rows of the larger cloud that are in a mutual pair, ascending
    mutual_per_block            how many of them fall into each block of 512 rows (CM_ROWS), written out by hand
    recheck                     (regime of MC_RECHECK0, of MC_RECHECK1): "zero", "some" (> 0), "many" (> RC_SMALL_ROWS)
                                or None (not claimed); claimed only where the margin is wide (see _steered)
    L                           {index into params: number of correspondences}        (where the case builds it)

The descriptors are small integers (or a constant plus a few units in the last place), so every distance below is an
exact binary32 number and ties, duplicates and runner-ups are what they are by construction, not by luck.
"""
from collections import namedtuple

import numpy as np

f32 = np.float32

# ---------------------------------------------------------------------------------------------- mirrored constants
NN_QPB = 512            # match.hip: queries per workgroup of k_nn_f16; the tables are padded to multiples of it
NN_TILE_ROWS = 32       # base rows per tile of the f16 engine
NN_MAXSPLIT = 32        # slices of the base cloud per query block, at most
NN_FINH_Q = 64          # queries per workgroup of k_nn_finish_f16 (four lanes each; candidates: one aligned quad of a tile)
HT_ROWS_SINGLE = 64     # rows per workgroup of k_half_tables, one pair at a time
RC_ROWS = 128           # listed rows per wave of k_recheck_filter's four-block form
RC_SMALL_ROWS = 2048    # listed rows up to which k_recheck_filter takes the one-block form
RCW_CAP = 1024          # pairs a wave's list holds before it is evaluated
CM_ROWS = 512           # rows of the larger cloud per workgroup of k_cross_multi
PM_SRC = 512            # source indices per workgroup of k_pairs_multi
TAIL_MAXWG = 256        # frontend.h: look-back words of the fused tail; above TAIL_MAXWG * 512 rows the six-launch tail
MEAN_CHUNK = 2048       # frontend.hip: points per staged chunk of d_seq_mean (unrolled by 32 inside)
F16_MAX_ABS = 255.0     # the f16 filter's guard: every |value| <= 255 ...
F16_MAX_NORM2 = 65000.0  # ... and every |row|^2 < 65000

# enum of frontend.h: the words of DBG_MATCH_STATS
MC_NCORR, MC_HIDDEN_I, MC_HIDDEN_J, MC_NCROSS, MC_NTUPLE, MC_SWAPPED, MC_NQ0, MC_NHIT = range(8)
MC_RECHECK0, MC_RECHECK1, MC_NSPLIT0, MC_NSPLIT1, MC_UNSAFE, MC_TAILERR = range(8, 14)

MatchCase = namedtuple("MatchCase", "xyz_s desc_s xyz_t desc_t params claims")


def dedup_slots(max_voxels):
    """Mirror of dedup_slots (frontend.hip): slots of a handle's duplicate table, a power of two"""
    m = 1024
    while m < 2 * max_voxels:
        m <<= 1
    return m


def _mix64(x):
    x = np.array(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def desc_hash33(desc):
    """Mirror of desc_hash33 (frontend.hip) over the BIT PATTERNS of the 33 values -> uint64 [n].  The duplicate table is
    entered at hash & (slots - 1) and compares the high 32 bits (the tag)."""
    b = np.ascontiguousarray(desc, dtype=f32).reshape(-1, 33).view(np.uint32).astype(np.uint64)
    h = np.zeros(b.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(33):
            h += _mix64((b[:, k] | np.uint64((k + 1) << 32)) * np.uint64(0x9E3779B97F4A7C15))
    return _mix64(h)


def nn_plan_single(qb, nt, X):
    """Mirror of nn_plan_single (match.hip): qb query blocks, nt base tiles, X workgroups -> slices | tiles per slice << 8"""
    if qb <= X:
        sp = X // (qb if qb > 1 else 1)
    else:
        T = max(64, (qb * nt + X * 8 - 1) // (X * 8))
        sp = (nt + T - 1) // T
    sp = max(1, min(sp, NN_MAXSPLIT, nt))
    tps = (nt + sp - 1) // sp
    sp = (nt + tps - 1) // tps
    return sp | (tps << 8)


def padded(n):
    return (n + NN_QPB - 1) // NN_QPB * NN_QPB


def plan_words(n_small, n_large, nhit, X):
    """(MC_NSPLIT0, MC_NSPLIT1) of a single pair: direction 0 asks the larger cloud for every row of the smaller one,
    direction 1 the smaller cloud for the hit rows"""
    return (nn_plan_single((n_small + NN_QPB - 1) // NN_QPB, padded(n_large) // NN_TILE_ROWS, X),
            nn_plan_single((nhit + NN_QPB - 1) // NN_QPB, padded(n_small) // NN_TILE_ROWS, X))


# by hand, for 256 workgroups and at most 256 query blocks: padded base rows -> (slices, tiles per slice).  512 rows are
# 16 tiles, one each; 1024: 32 tiles, one each; 1536: 48 tiles over at most 32 slices is two each, so 24 slices; 2048: 64
# tiles, two each; 2560: 80 tiles, three each, 27 slices, the last one short (two tiles)
PLAN_256 = {512: (16, 1), 1024: (32, 1), 1536: (24, 2), 2048: (32, 2), 2560: (27, 3)}


def _plan256(n_small, n_large, nhit):
    a, b = PLAN_256[padded(n_large)], PLAN_256[padded(n_small)]
    return (a[0] | (a[1] << 8), b[0] | (b[1] << 8))


def variant(crosscheck=True, tuple_test=True, tuple_scale=0.95, seed=0):
    return dict(crosscheck=bool(crosscheck), tuple_test=bool(tuple_test), tuple_scale=float(f32(tuple_scale)), seed=int(seed))


BIG_SEED = (1 << 32) + 12345
V_MAIN = (variant(seed=7),)
V_TWO = (variant(seed=0), variant(tuple_test=False))
V_ALL = (variant(seed=0), variant(tuple_test=False), variant(crosscheck=False, seed=BIG_SEED),
         variant(crosscheck=False, tuple_test=False), variant(seed=BIG_SEED))


def _seed(name):
    return [ord(c) for c in name]


# ---------------------------------------------------------------------------------------------- descriptors
def _code(rows):
    """Row r -> its four base-16 digits times 4 in values 0..3, zeros elsewhere: two different rows are at least 16 apart
    (squared), every value is at most 60 and |row|^2 at most 14400"""
    rows = np.asarray(rows, dtype=np.int64)
    assert rows.size == 0 or (rows.min() >= 0 and rows.max() < 65536)
    d = np.zeros((rows.size, 33), dtype=f32)
    for k in range(4):
        d[:, k] = (4 * ((rows >> (4 * k)) & 15)).astype(f32)
    return d


def _ranks(pi):
    """rank of j among the rows with the same pi, in ascending j"""
    pi = np.asarray(pi, dtype=np.int64)
    order = np.lexsort((np.arange(pi.size), pi))
    rank = np.zeros(pi.size, dtype=np.int64)
    start = np.r_[0, np.nonzero(np.diff(pi[order]))[0] + 1]
    first = np.repeat(start, np.diff(np.r_[start, pi.size]))
    rank[order] = np.arange(pi.size) - first
    return rank


def _steered(n_large, n_small, pi, dup=False):
    """The larger cloud is _code(0 .. n_large - 1).  Row j of the smaller cloud is _code(pi[j]) + e4 + the base-8 digits of
    its rank in values 5..8 (dup: without the digits, so rows with the same pi repeat each other bit for bit).  Values 4..8
    are zero in the larger cloud, hence for every row j and every row i != pi[j]
        d(j, i) = |_code(pi[j]) - _code(i)|^2 + |offset|^2 >= 16 + d(j, pi[j]):
    j answers pi[j]; a hit row i answers the lowest j with pi[j] = i (distance 1, the next rank 2, or hidden duplicates),
    and is in a mutual pair with it.  All distances are integers below 2^24: exact.  The f16 filter's bound on these values
    is u (76 + 108) 14600 + ... < 0.2, every gap between a winner and its runner-up is at least 1: nothing is listed for
    the re-check (regime "zero") with a margin of five."""
    pi = np.asarray(pi, dtype=np.int64)
    assert pi.size == n_small and pi.min() >= 0 and pi.max() < n_large
    large = _code(np.arange(n_large))
    small = _code(pi)
    small[:, 4] = 1
    if not dup:
        rank = _ranks(pi)
        assert rank.max() < 4096
        for k in range(4):
            small[:, 5 + k] = ((rank >> (3 * k)) & 7).astype(f32)
    return large, small


def _spread(n_large, hit):
    """hit distinct rows spread over the larger cloud, the first and the last row among them (for hit >= 2)"""
    if hit == 1:
        return np.array([n_large // 2], dtype=np.int64)
    return (np.arange(hit, dtype=np.int64) * (n_large - 1)) // (hit - 1)


def _hidden(desc):
    b = np.ascontiguousarray(desc, dtype=f32).view(np.uint32)
    return int(b.shape[0] - np.unique(b, axis=0).shape[0])


def _unsafe(*descs):
    out = False
    for d in descs:
        d64 = d.astype(np.float64)
        with np.errstate(all="ignore"):
            out = out or bool(np.any(~(np.abs(d) <= f32(F16_MAX_ABS)))) or bool(np.any(~((d64 * d64).sum(1).astype(f32) < f32(F16_MAX_NORM2))))
    return out


# ---------------------------------------------------------------------------------------------- geometry
def _rigid(xyz):
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return xyz @ R.T + np.array([1.0, 2.0, 0.5])


def _geometry(name, n_large, n_small, pi, mode="rigid"):
    """Points of the larger cloud in a 40 m box; row j of the smaller cloud is the rigid image of row pi[j] of the larger one
    plus 2 cm of noise ("rigid": nearly every triple of matched pairs passes the tuple test), a random point for every
    second j ("half": a good share passes), or twice the rigid image ("scaled": every length is off by a factor of two
    and no triple passes)"""
    rng = np.random.default_rng(_seed("geo:" + name))
    pl = rng.uniform(-20, 20, (n_large, 3))
    ps = _rigid(pl[np.asarray(pi, dtype=np.int64) % n_large]) + rng.normal(0, 0.02, (n_small, 3))
    if mode == "half":
        odd = np.arange(n_small) % 2 == 1
        ps[odd] = rng.uniform(-20, 20, (int(odd.sum()), 3))
    elif mode == "scaled":
        ps = 2.0 * ps
    out = []
    for p in (pl, ps):
        c = np.zeros((p.shape[0], 4), dtype=f32)
        c[:, :3] = p.astype(f32)
        out.append(c)
    return out


def _assemble(name, large, small, pi, params, claims, large_is_target, mode="rigid"):
    n_large, n_small = large.shape[0], small.shape[0]
    assert n_small <= n_large
    if n_small == n_large:
        large_is_target = False  # (equal sizes: no swap, the source is "the larger" cloud)
    xl, xs = _geometry(name, n_large, n_small, pi, mode)
    base = dict(n_large=n_large, n_small=n_small, swapped=bool(large_is_target), hidden_large=_hidden(large),
                hidden_small=_hidden(small), unsafe=_unsafe(large, small))
    base.update(claims)
    if large_is_target:
        return MatchCase(xs, small, xl, large, tuple(params), base)
    return MatchCase(xl, large, xs, small, tuple(params), base)


def _steered_case(name, n_small, n_large, pi, params, large_is_target, dup=False, mode="rigid", extra=None):
    pi = np.asarray(pi, dtype=np.int64)
    large, small = _steered(n_large, n_small, pi, dup)
    hit, first = np.unique(pi, return_index=True)
    nn_sl = np.full(n_large, -1, dtype=np.int64)
    nn_sl[hit] = first
    npre = np.bincount(pi, minlength=n_large)
    claims = dict(nhit=int(hit.size), nn_large_of_small={j: int(pi[j]) for j in range(n_small)},
                  nn_small_of_large={i: int(nn_sl[i]) for i in range(n_large)},
                  attain0={j: 1 for j in range(n_small)},
                  attain1={int(i): (int(npre[i]) if dup else 1) for i in hit},
                  mutual_rows=[int(i) for i in hit], recheck=("zero", "zero"))
    if padded(n_large) in PLAN_256 and padded(n_small) in PLAN_256:
        claims["plan256"] = _plan256(n_small, n_large, int(hit.size))
    claims.update(extra or {})
    return _assemble(name, large, small, pi, params, claims, large_is_target, mode)


# ---------------------------------------------------------------------------------------------- plan edges
# (rows of the smaller cloud, of the larger cloud, hit rows): direction 0 has the smaller cloud's rows as queries and the
# larger cloud as base, direction 1 the hit rows as queries and the smaller cloud as base.  Together: queries on both sides
# of 512 (one block, two) against a base on both sides of 512, 1024 and 2048 rows, in both directions; 1 hit row; bases of
# 1, 31, 32, 33 rows; 64 / 65 queries (one workgroup of k_nn_finish_f16, two)
PLAN_SHAPES = [
    (512, 512, 512), (512, 513, 1), (513, 513, 513), (512, 1024, 512), (513, 1024, 512), (512, 1025, 1), (513, 1025, 513),
    (512, 2048, 512), (513, 2048, 513), (512, 2049, 512), (513, 2049, 513),
    (1024, 1024, 512), (1024, 1025, 513), (1025, 1025, 512), (1025, 1026, 513), (2048, 2048, 512), (2048, 2049, 513),
    (2049, 2049, 512), (2049, 2050, 513), (2048, 2049, 1), (1025, 2049, 1025),
    (1, 1, 1), (1, 31, 1), (31, 32, 31), (32, 33, 32), (33, 33, 33), (1, 700, 1), (64, 65, 64), (65, 65, 65), (65, 700, 64),
]


def _plan_name(s, l, h):
    return f"plan_s{s}_l{l}_h{h}"


PLAN_NAMES = [_plan_name(*t) for t in PLAN_SHAPES]


def _plan_case(name, s, l, h, k):
    pi = _spread(l, h)[np.arange(s) % h]
    # (every other case: the rows that share an answer repeat each other bit for bit, across the 64-row workgroups of
    # k_half_tables; the target is the larger cloud in every second case that has a larger cloud)
    return _steered_case(name, s, l, pi, V_TWO if k % 3 else V_MAIN, large_is_target=(k % 2 == 0), dup=(k % 2 == 1),
                         mode="half" if k % 2 else "rigid")


# ---------------------------------------------------------------------------------------------- candidates and ties
def _cand_rows():
    """(kind, centre row w, partner row p): the base cloud is _code(rows) with row p overwritten by a vector next to row w.
    With 2049 base rows and 256 workgroups a slice is three tiles, 96 rows (PLAN_256)."""
    return [
        ("runner", 100, 104),    # winner and runner-up in adjacent quads of one tile (rows 100..103, 104..107)
        ("runner", 204, 200),    # ... the runner-up in the lower quad
        ("runner", 319, 320),    # adjacent tiles of one slice (rows 288..383)
        ("runner", 383, 384),    # adjacent tiles, adjacent slices
        ("runner", 50, 2000),    # slices 0 and 20
        ("runner", 2040, 60),    # the winner in slice 21, the runner-up in slice 0
        ("runner", 2048, 2047),  # the winner is the last row, alone in its tile; the runner-up closes the tile before
        ("tie", 500, 1500),      # an exact tie of two rows that are not bit-identical, slices 5 and 15
        ("tie", 700, 701),       # ... in one quad
        ("tie", 831, 832),       # ... across a tile boundary
        ("tie", 1151, 1152),     # ... across a slice boundary (1152 = 12 * 96)
        ("zero", 900, 1900),     # +0.0 / -0.0 twins, slices 9 and 19
        ("zero", 940, 941),      # ... in one quad
        ("dup", 10, 1200),       # a bit-duplicate whose original is in another 64-row group and another slice
        ("dup", 1300, 1301),     # ... in the same quad
        ("dup", 62, 66),         # ... across the 64-row boundary of k_half_tables, adjacent quads
    ]


def _cand_base(n):
    """-> (base [n, 33], queries {centre row: vector}, attain {centre row: rows attaining the minimum})"""
    base = _code(np.arange(n))
    queries, attain = {}, {}
    for kind, w, p in _cand_rows():
        c = _code([w])[0]
        q = c.copy()
        if kind == "runner":      # d(q, w) = 1, d(q, p) = 1 + 2^-10: inside the filter's bound, the re-check decides
            base[p] = c
            base[p, 5] = f32(2.0 ** -5)
            q[4] = 1
            attain[w] = 1
        elif kind == "tie":       # rows w and p symmetric about the query: d = 1 to both, the lower row wins
            base[w], base[p] = c, c
            base[w, 5], base[p, 5] = 1, -1
            attain[w] = 2
        elif kind == "zero":      # p repeats w with -0.0 where w has +0.0: equal values, different bits
            base[p] = c
            base[p, 4:] = f32(-0.0)
            q[4] = 1
            attain[w] = 2
        else:                     # p repeats w bit for bit
            base[p] = c
            q[4] = 1
            attain[w] = 2
        queries[w] = q
    return base, queries, attain


def _cands_dir0(name):
    """direction 0: the structured cloud is the larger one (2049 rows), the queries are rows of the smaller one (65)"""
    n_large, n_small = 2049, 65
    large, queries, attain = _cand_base(n_large)
    centres = [w for _, w, _ in _cand_rows()]
    pi = np.array(centres + [1003 + 7 * k for k in range(n_small - len(centres))], dtype=np.int64)
    _, small = _steered(n_large, n_small, pi)
    for j, w in enumerate(centres):
        small[j] = queries[w]
    winner = {w: min(w, p) if kind != "runner" else w for kind, w, p in _cand_rows()}
    claims = dict(nhit=n_small, nn_large_of_small={j: int(winner.get(int(pi[j]), pi[j])) for j in range(n_small)},
                  attain0={j: int(attain.get(int(pi[j]), 1)) for j in range(n_small)},
                  plan256=_plan256(n_small, n_large, n_small), recheck=("some", None))
    return _assemble(name, large, small, pi, V_TWO, claims, large_is_target=True)


def _cands_dir1(name):
    """direction 1: the structured cloud is the smaller one (2049 rows); row r of the larger cloud (2050 rows) is
    _code(r) + 2 e12, which row r of the smaller cloud answers (distance 4), except the centre rows, which hold the queries
    (distance 1 from their centre): every query is a hit row"""
    n_small, n_large = 2049, 2050
    small, queries, attain = _cand_base(n_small)
    large = _code(np.arange(n_large))
    large[:, 12] = 2
    for w, q in queries.items():
        large[w] = q
    winner = {w: min(w, p) if kind != "runner" else w for kind, w, p in _cand_rows()}
    claims = dict(nn_small_of_large={int(w): int(winner[w]) for w in queries}, attain1={int(w): int(attain[w]) for w in queries},
                  recheck=(None, "some"))
    return _assemble(name, large, small, np.arange(n_small), V_TWO, claims, large_is_target=False)


def _all_identical(name, which):
    """every row of one cloud is the same vector, the other cloud is distinct (700 and 65 rows)"""
    n_large, n_small = 700, 65
    pi = _spread(n_large, n_small)
    large, small = _steered(n_large, n_small, pi)
    if which == "large":   # every query ties over all 700 rows and answers row 0; row 0 answers the row next to the vector
        large[:] = _code([333])[0]
        nn = {j: 0 for j in range(n_small)}
        claims = dict(nhit=1, nn_large_of_small=nn, attain0={j: n_large for j in range(n_small)}, mutual_rows=[0])
    else:                  # every query answers the row next to the vector; that row ties over all 65 rows: row 0
        small[:] = _code([333])[0]
        small[:, 4] = 1
        claims = dict(nhit=1, nn_large_of_small={j: 333 for j in range(n_small)}, nn_small_of_large={333: 0},
                      attain1={333: n_small}, mutual_rows=[333])
    return _assemble(name, large, small, pi, V_ALL, claims, large_is_target=(which == "small"))


# two values (bit patterns, found by a search over 2^24 of them) that give _code(40) + v e20 the same hash tag AND the same
# slot in a duplicate table of 16384 slots — what a handle with 4096 < max_voxels <= 8192 has
HASH_TWINS = (0x400ebc4d, 0x402cd171)  # 2.230243, 2.7002833
HASH_CASE_MAX_VOXELS = 8192


def _hash_collision(name):
    """Rows 40 and 700 of the larger cloud differ in value 20 only and collide in the duplicate table (same slot, same tag);
    row 1500 repeats row 700 bit for bit.  The table names row 40 for all three: rows 700 and 1500 are compared with it,
    differ, and stay — a collision costs the merge of 700 and 1500, never a wrongly hidden row.  The query next to them then
    has an exact tie of two rows that are not hidden (re-check, the lower row), the query next to row 40 its own row."""
    n_large, n_small = 2049, 65
    pi = np.array([700, 40] + [1003 + 7 * k for k in range(n_small - 2)], dtype=np.int64)
    large, small = _steered(n_large, n_small, pi)
    x, y = np.array(HASH_TWINS, dtype=np.uint32).view(f32)
    c = _code([40])[0]
    large[40], large[700], large[1500] = c, c, c
    large[40, 20], large[700, 20], large[1500, 20] = x, y, y
    small[0], small[1] = large[700], large[40]
    small[0, 4], small[1, 4] = 1, 1
    claims = dict(nhit=n_small, nn_large_of_small={j: int(pi[j]) for j in range(n_small)}, attain0={0: 2, 1: 1},
                  nn_small_of_large={700: 0, 40: 1, 1500: -1}, device_hidden_large=0, plan256=_plan256(n_small, n_large, n_small))
    return _assemble(name, large, small, pi, V_TWO, claims, large_is_target=True)


CAND_NAMES = ["cands_dir0", "cands_dir1", "identical_large", "identical_small", "hash_collision"]


# ---------------------------------------------------------------------------------------------- re-check
def _recheck_ties(name, K):
    """K rows of the smaller cloud — distinct: the base-8 digits of k in values 5..8 — at the same distance from two rows of
    the larger cloud (100 and 400: c + e4 and c - e4), which no gap separates: exactly these K rows cannot be certified in
    direction 0.  Row 100 is the only hit row; its answer is the row with digits 0, the next one is 1 farther."""
    n_small = max(K, 2)
    n_large = max(700, n_small + 1)
    pi = np.full(n_small, 100, dtype=np.int64)
    large, small = _steered(n_large, n_small, pi)
    c = _code([100])[0]
    large[100], large[400] = c, c
    large[100, 4], large[400, 4] = 1, -1
    small[:, 4] = 0
    att = {j: 2 for j in range(n_small)}
    if K < n_small:  # (K = 1: the second row of the smaller cloud is on row 100's side, 1 from it and 5 from row 400)
        small[K:, 4] = 1
        att.update({j: 1 for j in range(K, n_small)})
    claims = dict(nhit=1, nn_large_of_small={j: 100 for j in range(n_small)}, attain0=att, nn_small_of_large={100: 0},
                  recheck=("many" if K > RC_SMALL_ROWS else "some", None), listed0=K)
    return _assemble(name, large, small, pi, V_MAIN, claims, large_is_target=True)


def _recheck_cluster(name):
    """3001 and 3000 rows that differ in the last places of value 0 only: y_i = 100 + 4 i ulp, x_j = 100 + (4 j + 1) ulp,
    ulp = 2^-17.  Every difference is a small multiple of the ulp and its square exact: x_j answers y_j (one ulp away, the
    next is three), y_i answers x_i, every row of the smaller cloud is in a mutual pair.  The filter's bound at |row|^2 =
    10000 is about 0.1, twelve orders of magnitude above any of these distances: every query of either direction is listed,
    with thousands of base rows under its threshold — the four-block form, and a wave's list overflows in every slice."""
    n_large, n_small = 3001, 3000
    ulp = 2.0 ** -17
    large = np.zeros((n_large, 33), dtype=f32)
    small = np.zeros((n_small, 33), dtype=f32)
    large[:, 0] = (100.0 + 4 * np.arange(n_large) * ulp).astype(f32)
    small[:, 0] = (100.0 + (4 * np.arange(n_small) + 1) * ulp).astype(f32)
    large[:, 1:12], small[:, 1:12] = 3, 3
    assert np.array_equal(large[:, 0].astype(np.float64), 100.0 + 4 * np.arange(n_large) * ulp)
    pi = np.arange(n_small)
    claims = dict(nhit=n_small, nn_large_of_small={j: j for j in range(n_small)}, nn_small_of_large={i: i for i in range(n_small)},
                  attain0={j: 1 for j in range(n_small)}, attain1={i: 1 for i in range(n_small)},
                  mutual_rows=list(range(n_small)), recheck=("many", "many"))
    return _assemble(name, large, small, pi, V_TWO, claims, large_is_target=True)


def _unsafe_case(name, what):
    """one row outside the f16 filter's guard — a value of 300, or 33 values of 45 (|row|^2 = 66825) — in an otherwise steered
    pair: MC_UNSAFE, every row goes to the exact re-check with an infinite threshold, the tables stay exact"""
    n_large, n_small = 700, 600
    pi = _spread(n_large, n_small)
    large, small = _steered(n_large, n_small, pi)
    row = np.zeros(33, dtype=f32)
    if what == "value":
        row[20] = 300
    else:
        row[:] = 45
    free = sorted(set(range(n_large)) - set(pi.tolist()))[50]  # (a row that is nobody's answer)
    large[free] = row
    hit, first = np.unique(pi, return_index=True)
    claims = dict(nhit=n_small, nn_large_of_small={j: int(pi[j]) for j in range(n_small)}, unsafe=True,
                  nn_small_of_large={int(i): int(j) for i, j in zip(hit, first)}, mutual_rows=[int(i) for i in hit],
                  recheck=("some", "some"))
    return _assemble(name, large, small, pi, V_TWO, claims, large_is_target=(what == "value"))


RECHECK_KS = (1, 128, 129, 2048, 2049)
RECHECK_NAMES = ["recheck_none"] + [f"recheck_ties_{k}" for k in RECHECK_KS] + ["recheck_cluster", "unsafe_value", "unsafe_norm"]


# ---------------------------------------------------------------------------------------------- tail
def _decoy(large, small, i, spare, j):
    """Row i of the larger cloud (hit by a second row of the smaller cloud as well) loses its mutual pair: row j of the smaller cloud moves to _code(i) + e9 / 2
    (0.25 from row i, which now answers j), and row `spare` of the larger cloud to _code(i) + e9 / 2 + e10 / 4 (0.0625
    from j, which answers it): (spare, j) is mutual, i is asked and not mutual"""
    c = _code([i])[0]
    small[j] = c
    small[j, 9] = 0.5
    large[spare] = c
    large[spare, 9], large[spare, 10] = 0.5, 0.25


def _tail_case(name):
    kind = name[len("tail_"):]
    mode, params, tgt_large = "half", V_ALL, True
    extra = {}
    if kind == "l513_rows_0_511_512":  # 513 rows: two workgroups of k_cross_multi, the pairs on the rows around their border
        s, l = 300, 513
        pi = np.r_[[0, 511, 512], np.array([0, 511, 512])[np.arange(s - 3) % 3]]
        extra = dict(mutual_per_block=[2, 1])
    elif kind == "l1025_rows_511_512_513":  # three workgroups; 511 | 512, 513 | nothing in the last (one row)
        s, l = 301, 1025
        pi = np.r_[[511, 512, 513], np.array([511, 512, 513])[np.arange(s - 3) % 3]]
        extra = dict(mutual_per_block=[1, 2, 0])
    elif kind == "l512_all":           # one workgroup, every row mutual: the smaller cloud is a permutation of the larger
        s, l = 512, 512
        pi = (np.arange(s) * 37 + 5) % l
        extra = dict(mutual_per_block=[512])
    elif kind == "l1024_middle_empty":  # ns == nt = 1024 (no swap): two workgroups, all pairs in the first
        s, l = 1024, 1024
        pi = np.arange(s) % 300
        extra = dict(mutual_per_block=[300, 0])
    elif kind == "l1025_swap_all":     # nt == ns + 1 (swap): every row of the smaller cloud mutual, the last row of the larger not
        s, l = 1024, 1025
        pi = (np.arange(s) * 39 + 11) % 1024
        extra = dict(mutual_per_block=[512, 512, 0])
    elif kind == "l1537_gap":          # four workgroups, the second contributes nothing, the last one row: look-back over three
        s, l = 700, 1537
        rows = np.r_[np.arange(0, 512, 3), np.arange(1024, 1536, 2), [1536]]
        pi = rows[np.arange(s) % rows.size]
        extra = dict(mutual_per_block=[171, 0, 256, 1])
    elif kind == "l1537_src_large":    # the same rows with the larger cloud as the source: k_pairs_multi has four workgroups
        s, l = 700, 1537
        rows = np.r_[np.arange(0, 512, 3), np.arange(1024, 1536, 2), [1536]]
        pi = rows[np.arange(s) % rows.size]
        tgt_large = False
        extra = dict(mutual_per_block=[171, 0, 256, 1])
    elif kind == "fewest_mutual":
        return _chain_case(name)
    elif kind == "none_passes":        # every length of the smaller cloud doubled: MC_NCROSS > 0 and L = 0 under the tuple test
        s, l = 600, 1025
        pi = _spread(l, s)
        mode = "scaled"
        extra = dict(L={0: 0, 4: 0, 1: 600})
    elif kind == "decoys":             # asked rows that are not mutual, next to the 512-row border
        s, l = 403, 1025
        pi = np.r_[np.arange(300, 700), [511, 512, 600]]  # (rows 400..402: second answers that keep the decoyed rows hit)
        large, small = _steered(l, s, pi)
        for i, spare, j in ((511, 900, 211), (512, 901, 212), (600, 902, 300)):
            _decoy(large, small, i, spare, j)
        hit = sorted(set(range(300, 700)) | {900, 901, 902})
        mutual = sorted((set(range(300, 700)) - {511, 512, 600}) | {900, 901, 902})
        nn_ls = {j: int(pi[j]) for j in range(s)}
        nn_ls.update({211: 900, 212: 901, 300: 902, 400: 511, 401: 512, 402: 600})
        nn_sl = {i: i - 300 for i in range(300, 700)}
        nn_sl.update({900: 211, 901: 212, 902: 300})
        claims = dict(nhit=len(hit), nn_large_of_small=nn_ls, nn_small_of_large=nn_sl, mutual_rows=mutual,
                      mutual_per_block=[211, 189, 0], plan256=_plan256(s, l, len(hit)))
        return _assemble(name, large, small, pi, V_ALL, claims, large_is_target=True, mode="rigid")
    else:
        raise KeyError(name)
    return _steered_case(name, s, l, pi, params, tgt_large, mode=mode, extra=extra)


def _chain_case(name):
    """The fewest mutual pairs a pair of clouds without NaNs can have is one (the closest pair of all, ties to the lowest
    rows, is mutual), and this pair has exactly one: the rows lie on a line in value 0, alternating between the clouds,
    S_0 L_0 S_1 L_1 ..., with gaps that shrink by one unit of 2^-12 per step, so every row's nearest row of the other cloud
    is the NEXT one on the line: S_k answers L_k, L_k answers S_(k+1), and only the last two rows answer each other.
    ns == nt = 600: no swap; every row of the larger cloud but one is asked and dropped by the mutual test."""
    n = 600
    M = 2 * n
    gaps = (M - np.arange(M - 1)).astype(np.float64) * 2.0 ** -12
    pos = np.r_[0.0, np.cumsum(gaps)]
    assert pos[-1] < 250 and np.array_equal(pos.astype(f32).astype(np.float64), pos)
    small = np.zeros((n, 33), dtype=f32)
    large = np.zeros((n, 33), dtype=f32)
    small[:, 0] = pos[0::2].astype(f32)
    large[:, 0] = pos[1::2].astype(f32)
    nn_ls = {k: k for k in range(n)}
    nn_sl = {k: k + 1 for k in range(n - 1)}
    nn_sl[n - 1] = n - 1
    claims = dict(nhit=n, nn_large_of_small=nn_ls, nn_small_of_large=nn_sl, mutual_rows=[n - 1], mutual_per_block=[0, 1],
                  attain0={k: 1 for k in range(n)}, attain1={k: 1 for k in range(n)})
    return _assemble(name, large, small, np.arange(n), V_ALL, claims, large_is_target=False)


TAIL_NAMES = ["tail_" + k for k in ("l513_rows_0_511_512", "l1025_rows_511_512_513", "l512_all", "l1024_middle_empty", "l1025_swap_all",
                                    "l1537_gap", "l1537_src_large", "fewest_mutual", "none_passes", "decoys")]


# ---------------------------------------------------------------------------------------------- rows without a candidate
def _nocand_case(name):
    """NaN descriptor rows in a steered pair of 700 and 600 rows.  A NaN distance never wins and a query without a candidate
    answers row 0 — in both directions; a NaN is outside the f16 guard, so every one of these pairs is MC_UNSAFE."""
    kind = name[len("nocand_"):]
    n_large, n_small = 700, 600
    pi = _spread(n_large, n_small)
    pi[0] = 0
    large, small = _steered(n_large, n_small, pi)
    nan = f32(np.nan)
    nn_ls = {j: int(pi[j]) for j in range(n_small)}
    hit, first = np.unique(pi, return_index=True)
    nn_sl = {int(i): int(j) for i, j in zip(hit, first)}
    if kind == "small_only":     # three rows of the smaller cloud, one of them with a single NaN value: they answer row 0
        small[3], small[64] = nan, nan
        small[599, 17] = nan
        for j in (3, 64, 599):
            nn_ls[j] = 0
            del nn_sl[int(pi[j])]
        claims = dict(attain0={3: 0, 64: 0, 599: 0}, cross_has_00=True)  # (row 0 answers 0 and 0 answers row 0: both are clean)
    elif kind == "large_row":    # a NaN row of the larger cloud that is not row 0: nobody can answer it, it is never asked
        large[int(pi[5])] = nan
        del nn_ls[5], nn_sl[int(pi[5])]
        claims = dict(nn_small_of_large_unasked=[int(pi[5])])
    elif kind == "row0_both":    # row 0 of both clouds: 0 answers 0 for want of a candidate, twice, and the pair (0, 0) is mutual
        large[0], small[0] = nan, nan
        nn_ls[0], nn_sl[0] = 0, 0
        claims = dict(attain0={0: 0}, attain1={0: 0}, cross_has_00=True)
    elif kind == "row0_large_asked":  # row 0 of the larger cloud is NaN and asked by a NaN row of the smaller one: it answers 0,
        large[0], small[7] = nan, nan  # whose own answer is another row: asked, answered, not mutual
        del nn_ls[0], nn_sl[int(pi[7])]
        nn_ls[7], nn_sl[0] = 0, 0
        claims = dict(attain0={7: 0}, attain1={0: 0}, cross_has_00=False)
    elif kind == "all_small":    # every row of the smaller cloud: all answer 0, row 0 is the one hit row and answers 0
        small[:] = nan
        nn_ls = {j: 0 for j in range(n_small)}
        nn_sl = {0: 0}
        claims = dict(nhit=1, attain0={j: 0 for j in range(n_small)}, attain1={0: 0}, cross_has_00=True, mutual_rows=[0])
    elif kind == "all_large":    # every row of the larger cloud
        large[:] = nan
        nn_ls = {j: 0 for j in range(n_small)}
        nn_sl = {0: 0}
        claims = dict(nhit=1, attain0={j: 0 for j in range(n_small)}, attain1={0: 0}, cross_has_00=True, mutual_rows=[0])
    else:
        raise KeyError(name)
    claims.update(nn_large_of_small=nn_ls, nn_small_of_large=nn_sl, unsafe=True)
    return _assemble(name, large, small, pi, V_ALL, claims, large_is_target=(kind not in ("large_row", "all_large")))


NOCAND_NAMES = ["nocand_" + k for k in ("small_only", "large_row", "row0_both", "row0_large_asked", "all_small", "all_large")]


# ---------------------------------------------------------------------------------------------- tail switch
SWITCH_SMALL = 600
SWITCH_NAMES = [f"switch_{n}_{side}" for n in (TAIL_MAXWG * 512, TAIL_MAXWG * 512 + 1) for side in ("src", "tgt")]


def _fpfh_like(rng, n):
    """random histograms in FPFH's range: three blocks of eleven bins that sum to 100 each"""
    d = rng.random((n, 3, 11), dtype=np.float32) ** 3
    d *= (100.0 / d.sum(axis=2, keepdims=True)).astype(f32)
    return np.ascontiguousarray(d.reshape(n, 33), dtype=f32)


def _switch_case(name):
    """The larger cloud has TAIL_MAXWG * 512 rows (the fused tail with all 256 look-back words in use) or one more (the
    six-launch tail), the smaller one 600; the smaller cloud's rows are noisy copies of rows spread over the larger one, so
    that a few hundred pairs are mutual and lie in workgroups all over the larger cloud."""
    _, n, side = name.split("_")
    n_large, n_small = int(n), SWITCH_SMALL
    rng = np.random.default_rng(_seed(name))
    large = _fpfh_like(rng, n_large)
    pi = _spread(n_large, n_small)
    small = large[pi] + rng.normal(0, 0.05, (n_small, 33)).astype(f32)
    claims = dict(nn_large_of_small={0: 0, n_small - 1: n_large - 1}, recheck=(None, None))
    return _assemble(name, large, small, pi, (variant(seed=3), variant(tuple_test=False)), claims, large_is_target=(side == "tgt"))


# ---------------------------------------------------------------------------------------------- the matcher mean
MEAN_SIZES = (1, 31, 32, 33, 2047, 2048, 2049, 4097)
MEAN_LEAF = 0.01


def mean_cloud(n):
    """n points whose coordinates alternate in sign with magnitudes between 1 and 190 (x), 30 (y) and full 24-bit fractions:
    a binary32 sum of them depends on the order of the additions.  The |x| are at least 0.04 apart, so at a leaf of
    MEAN_LEAF every point has a voxel of its own, and the box (372 x 60 x 0.02 m) is 37200 x 6000 x 3 voxels: int32."""
    assert n <= 4099
    rng = np.random.default_rng(_seed(f"mean{n}"))
    i = np.arange(n)
    sign = np.where(i % 2 == 0, 1.0, -1.0)
    x = sign * (1.0 + ((i * 37) % 4099) * 0.045) + rng.uniform(0, 0.004, n)
    y = -sign * (1.0 + ((i * 101) % 4099) * 0.007) * rng.uniform(0.5, 1.0, n)
    z = rng.uniform(0, 0.02, n)
    c = np.zeros((n, 4), dtype=f32)
    c[:, 0], c[:, 1], c[:, 2] = x.astype(f32), y.astype(f32), z.astype(f32)
    return c


# ---------------------------------------------------------------------------------------------- the grouped keyframes
GROUP_VOXELS = (1, 512, 513, 1025)
GROUP_LEAF = 0.3


def group_cloud(n, which):
    """n points on a jittered 0.5 m lattice over two walls and a floor, every point in a voxel of its own at GROUP_LEAF;
    which = 1 is the same scene moved by a small rigid motion"""
    rng = np.random.default_rng(_seed(f"group{n}"))
    m = int(np.ceil(np.sqrt(n / 3.0))) + 1
    a, b = np.meshgrid(np.arange(m) * 0.5, np.arange(m) * 0.5, indexing="ij")
    a, b = a.ravel() + 0.4, b.ravel() + 0.4  # (0.4 from the other two planes: no two points share a voxel)
    z0 = np.zeros_like(a)
    pts = np.concatenate([np.stack([a, b, z0], 1), np.stack([a, z0, b], 1), np.stack([z0, a, b], 1)])
    pts = pts[rng.permutation(pts.shape[0])[:n]] + rng.uniform(-0.02, 0.02, (n, 3))
    if which:
        pts = _rigid(pts)
    c = np.zeros((n, 4), dtype=f32)
    c[:, :3] = pts.astype(f32)
    return c


# ---------------------------------------------------------------------------------------------- the registry
ORDINARY_NAMES = PLAN_NAMES + CAND_NAMES + RECHECK_NAMES + TAIL_NAMES + NOCAND_NAMES
ALL_NAMES = ORDINARY_NAMES + SWITCH_NAMES
_cache = {}


def _build(name):
    if name in PLAN_NAMES:
        k = PLAN_NAMES.index(name)
        return _plan_case(name, *PLAN_SHAPES[k], k)
    if name == "cands_dir0":
        return _cands_dir0(name)
    if name == "cands_dir1":
        return _cands_dir1(name)
    if name == "hash_collision":
        return _hash_collision(name)
    if name.startswith("identical_"):
        return _all_identical(name, name[len("identical_"):])
    if name == "recheck_none":
        return _steered_case(name, 600, 700, _spread(700, 600), V_MAIN, True)
    if name.startswith("recheck_ties_"):
        return _recheck_ties(name, int(name.rsplit("_", 1)[1]))
    if name == "recheck_cluster":
        return _recheck_cluster(name)
    if name.startswith("unsafe_"):
        return _unsafe_case(name, name[len("unsafe_"):])
    if name.startswith("tail_"):
        return _tail_case(name)
    if name.startswith("nocand_"):
        return _nocand_case(name)
    if name.startswith("switch_"):
        return _switch_case(name)
    raise KeyError(name)


def case(name):
    if name not in _cache:
        c = _build(name)
        if name in SWITCH_NAMES:
            return c  # (17 MB each: not kept)
        _cache[name] = c
    return _cache[name]
