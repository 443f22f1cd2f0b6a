"""The yardstick of the grouped place query: a loop over the single query's restatement (tests/place_restate.py) and a
Python mirror of the host-side plan in include/qtr_place_batch_math.h.  Nothing is batched here: query q of a group is
place_restate.query with that query's descriptor, range and k, and its score row is place_restate.best_shift over its
clamped range."""
import numpy as np

import place_restate as pr

QT_CAP, LDS_BYTES, GRID_X, PAIR_CAP = 2, 65536, 2048, 1 << 26
MATCH_DTYPE = np.dtype([("id", "<i4"), ("shift", "<i4"), ("distance", "<f4"), ("yaw", "<f4")])


def stride(R, S):
    return ((R + 1) * S + 3) & ~3


def clamp(id_lo, id_hi, size):
    a, b = max(id_lo, 0), min(id_hi, size)
    return (a, b) if b > a else (0, 0)


def union(ranges):
    """The smallest [ulo, uhi) that holds every non-empty range; (0, 0) when there is none."""
    full = [(a, b) for a, b in ranges if b > a]
    if not full:
        return 0, 0
    return min(a for a, _ in full), max(b for _, b in full)


def qt(stride_floats):
    """The largest QT with (QT + 4) * stride * 4 <= 65536, at most QT_CAP."""
    n = 0
    while (n + 1 + 4) * stride_floats * 4 <= LDS_BYTES:
        n += 1
    return min(n, QT_CAP)


def pairs_ok(Q, U):
    return Q * U <= PAIR_CAP


def query_batch(descs, ranges, entries, k):
    """descs: Q images [R, S]; ranges: Q (id_lo, id_hi); entries [N, R, S].  Returns (records [Q, k] of MATCH_DTYPE, rows
    filled up to n[q] and zero behind, n int32 [Q])."""
    E = np.asarray(entries, dtype=np.float32)
    S = E.shape[2]
    out = np.zeros((len(descs), k), dtype=MATCH_DTYPE)
    n = np.zeros(len(descs), dtype=np.int32)
    for q, (d, (lo, hi)) in enumerate(zip(descs, ranges)):
        got = pr.query(d, E, k, lo, hi)
        n[q] = len(got)
        for r, (i, s, dist) in enumerate(got):
            out[q, r] = (i, s, dist, pr.yaw_of(s, S))
    return out, n


def scores(desc, rng, entries):
    """(distance float32, shift int32) of every entry of the query's clamped range, in id order."""
    E = np.asarray(entries, dtype=np.float32)
    lo, hi = clamp(rng[0], rng[1], len(E))
    if hi <= lo:
        return np.zeros(0, np.float32), np.zeros(0, np.int32)
    return pr.best_shift(desc, E[lo:hi])
