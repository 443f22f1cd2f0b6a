"""The yardstick of the place index: a plain restatement of the Scan Context descriptor, the shifted-column distance and
the ranking, written from the contract in include/quatro_hip.h and the operation order stated in
include/qtr_place_math.h.  It shares no code with the kernels: numpy float32 (every numpy operation rounds once, and no
product-sum is fused on the device either, so the bits agree), with the oracle's qm_atan2f for the one transcendental.
`distance64` is a second, independent evaluation of the same formulae in binary64."""
import numpy as np

PI_F = np.float32(3.14159274)
TWO_PI_F = np.float32(6.28318548)


def _atan2f(y, x):
    from oracle import oracle
    oracle.build()
    return oracle.math_fn(0, y, x)


def describe(xyz, R=20, S=60, max_range=80.0, height_offset=2.0, atan2f=_atan2f):
    """[R, S] float32 maximum-height image of the points xyz[:, :3] (float32)."""
    p = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)[:, :3])
    img = np.zeros(R * S, dtype=np.float32)
    p = p[np.isfinite(p).all(axis=1)]
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    zh = z + np.float32(height_offset)
    r = np.sqrt(x * x + y * y)
    keep = (zh > 0) & (r < np.float32(max_range))
    x, y, zh, r = x[keep], y[keep], zh[keep], r[keep]
    if x.size == 0:
        return img.reshape(R, S)
    ring = np.minimum(((r * np.float32(R)) / np.float32(max_range)).astype(np.int32), R - 1)
    a = atan2f(y, x).astype(np.float32) + PI_F
    sec = np.clip(((a * np.float32(S)) / TWO_PI_F).astype(np.int32), 0, S - 1)
    np.maximum.at(img, ring * S + sec, zh)
    return img.reshape(R, S)


def colnorm2(d):
    """[S] float32: the squares of column j added ring by ring."""
    d = np.asarray(d, dtype=np.float32)
    acc = np.zeros(d.shape[1], dtype=np.float32)
    for r in range(d.shape[0]):
        acc = acc + d[r] * d[r]
    return acc


def shift_distances(q, entries):
    """d(s) of the query image q [R, S] against every entry of entries [N, R, S]: [N, S] float32, column s = shift s."""
    q = np.asarray(q, dtype=np.float32)
    C = np.asarray(entries, dtype=np.float32)
    N, R, S = C.shape
    qn2 = colnorm2(q)
    cn2 = np.zeros((N, S), dtype=np.float32)
    for r in range(R):
        cn2 = cn2 + C[:, r, :] * C[:, r, :]
    total = np.zeros((N, S), dtype=np.float32)
    cnt = np.zeros((N, S), dtype=np.int32)
    shifts = np.arange(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(S):
            if not qn2[j] > 0:
                continue
            jc = (j + shifts) % S  # the entry's column for every shift
            den = np.sqrt(qn2[j] * cn2[:, jc])
            dot = np.zeros((N, S), dtype=np.float32)
            for r in range(R):
                dot = dot + q[r, j] * C[:, r, jc]
            t = np.float32(1.0) - dot / den
            t = np.where(t > 0, t, np.float32(0.0)).astype(np.float32)
            counts = den > 0
            total = np.where(counts, total + t, total).astype(np.float32)
            cnt = cnt + counts
        d = np.where(cnt > 0, total / cnt.astype(np.float32), np.float32(1.0)).astype(np.float32)
    return d


def best_shift(q, entries):
    """(distance [N] float32, shift [N]): the minimum over the shifts, ties to the lowest shift."""
    d = shift_distances(q, entries)
    s = np.argmin(d, axis=1)  # (argmin returns the first minimum)
    return d[np.arange(d.shape[0]), s], s.astype(np.int32)


def yaw_of(shift, S):
    y = (np.float32(shift) * TWO_PI_F) / np.float32(S)
    return np.float32(y - TWO_PI_F) if y > PI_F else np.float32(y)


def query(q, entries, k, id_lo=0, id_hi=None):
    """The min(k, candidates) best of the entries id_lo <= id < id_hi in ascending (distance bits, id) order, as tuples
    (id, shift, distance float32)."""
    N = len(entries)
    lo, hi = max(id_lo, 0), N if id_hi is None else min(id_hi, N)
    if hi <= lo:
        return []
    d, s = best_shift(q, np.asarray(entries, dtype=np.float32)[lo:hi])
    bits = d.view(np.uint32).astype(np.uint64)
    order = np.argsort((bits << np.uint64(32)) | (np.arange(lo, hi).astype(np.uint64)), kind="stable")[:k]
    return [(int(lo + i), int(s[i]), d[i]) for i in order]


def distance64(q, c):
    """(distance, shift) in binary64, by the formulae alone: roll the entry, cosine per column, mean over the columns where
    both are non-zero."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    S = q.shape[1]
    qn = np.linalg.norm(q, axis=0)
    best = (2.0, 0)
    for s in range(S):
        cs = np.roll(c, -s, axis=1)  # column j of cs = column (j + s) mod S of c
        cn = np.linalg.norm(cs, axis=0)
        both = (qn > 0) & (cn > 0)
        d = 1.0 if not both.any() else float(np.mean(1.0 - (q[:, both] * cs[:, both]).sum(axis=0) / (qn[both] * cn[both])))
        if d < best[0]:
            best = (d, s)
    return best
