"""The matcher restated in binary32 numpy, from the text of teaser::Matcher (normalizePoints, advancedMatching), of
flann::L2 and from the rules the CPU oracle declares where the reference leaves a choice open — not from
quatro_amd/csrc/match.hip.  tests/test_match_cases_cpu.py holds the oracle to it on the named clouds of
tests/match_cases.py; tests/test_gpu_match_cases.py holds the device to the oracle.

  * distance: flann::L2 over 33 values — eight groups of four, result += ((d0 d0 + d1 d1) + d2 d2) + d3 d3, then the
    tail term result += d d; every operation rounded to binary32, nothing contracted;
  * arg-min: a scan in ascending row order from +inf with strict improvement (KNNSimpleResultSet::addPoint), so the
    lowest row wins a tie, a NaN distance (and an infinite one) never wins, and a query without a candidate answers row 0;
  * the second direction is lazy: only the rows of the larger cloud that some row of the smaller cloud answers are asked
    (-1 everywhere else);
  * use_crosscheck: (i, j) with j = NN_j(i) and NN_i(j) = i, in ascending i; without it corres_ij (asked rows, ascending
    i) followed by corres_ji (ascending j);
  * the tuple test: ncorr * 100 trials, trial t draws rand_u32(seed, 3 t + k) % ncorr for k = 0, 1, 2 (the SplitMix64
    counter generator that stands in for srand(time) / rand()), the points centred on the sequential binary32 mean of
    their cloud, lengths sqrt(dx dx + (dy dy + dz dz));
  * un-swap, sort, unique.
"""
import numpy as np

f32 = np.float32
u64 = np.uint64


# ---------------------------------------------------------------------------------------------- the counter generator
def mix64(z):
    z = np.asarray(z, dtype=u64)
    with np.errstate(over="ignore"):
        z = z + u64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    return z ^ (z >> u64(31))


def rand_u32(seed, counter):
    """SplitMix64 finaliser over seed and counter: the high half of mix64(mix64(seed) ^ counter * 0xD1342543DE82EF95)"""
    counter = np.asarray(counter, dtype=u64)
    with np.errstate(over="ignore"):
        w = mix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=u64)) ^ (counter * u64(0xD1342543DE82EF95))
    return (mix64(w) >> u64(32)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- means
def seq_mean(xyz):
    """Matcher::normalizePoints: mean = mean + p over the cloud in order, then mean / n, all in binary32 -> [3]"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=f32)
    n = p.shape[0]
    return np.add.accumulate(p, axis=0, dtype=f32)[-1] / f32(n)


# ---------------------------------------------------------------------------------------------- nearest neighbours
def l2_flann33(Q, B):
    """[nq, 33] x [nb, 33] -> [nq, nb] binary32 distances in flann::L2's order"""
    Q, B = np.ascontiguousarray(Q, dtype=f32), np.ascontiguousarray(B, dtype=f32)
    res = np.zeros((Q.shape[0], B.shape[0]), dtype=f32)
    with np.errstate(all="ignore"):
        for g in range(8):
            d = [Q[:, None, 4 * g + k] - B[None, :, 4 * g + k] for k in range(4)]
            s = d[0] * d[0] + d[1] * d[1]
            s = s + d[2] * d[2]
            s = s + d[3] * d[3]
            res = res + s
        d = Q[:, None, 32] - B[None, :, 32]
        res = res + d * d
    return res


def repeats(desc):
    """rows that repeat an earlier row of the table bit for bit -> bool [n]"""
    b = np.ascontiguousarray(desc, dtype=f32).reshape(-1, 33).view(np.uint32)
    seen, out = set(), np.zeros(b.shape[0], dtype=bool)
    for i in range(b.shape[0]):
        k = b[i].tobytes()
        out[i] = k in seen
        seen.add(k)
    return out


def nn33(Q, B, block=256):
    """-> (row of B per query, int32; how many rows of B attain the query's minimum, 0 for a query without a candidate;
    the distance from the minimum to the next row of B that does not repeat an earlier row, +inf when there is none)"""
    Q = np.ascontiguousarray(Q, dtype=f32).reshape(-1, 33)
    idx = np.zeros(Q.shape[0], dtype=np.int32)
    ties = np.zeros(Q.shape[0], dtype=np.int64)
    gap = np.full(Q.shape[0], np.inf, dtype=np.float64)
    rep = repeats(B)
    for q0 in range(0, Q.shape[0], block):
        D = l2_flann33(Q[q0:q0 + block], B)
        D = np.where(D < np.inf, D, f32(np.inf))  # (a NaN compares false: neither it nor +inf ever improves on +inf)
        m = D.min(axis=1)
        has = m < np.inf
        idx[q0:q0 + block] = np.where(has, D.argmin(axis=1), 0)  # (argmin: the first, i.e. lowest, row of the minimum)
        ties[q0:q0 + block] = np.where(has, (D == m[:, None]).sum(axis=1), 0)
        if B.shape[0] - int(rep.sum()) >= 2:
            two = np.partition(D[:, ~rep].astype(np.float64), 1, axis=1)[:, :2]
            with np.errstate(invalid="ignore"):
                gap[q0:q0 + block] = np.where(two[:, 1] < np.inf, two[:, 1] - two[:, 0], np.inf)
    return idx, ties, gap


def tables(desc_s, desc_t):
    """Both nearest-neighbour tables of a pair (they do not depend on the settings) -> dict for match(tables_=...)"""
    feat = [np.ascontiguousarray(desc_s, dtype=f32).reshape(-1, 33), np.ascontiguousarray(desc_t, dtype=f32).reshape(-1, 33)]
    fi, fj = (1, 0) if feat[1].shape[0] > feat[0].shape[0] else (0, 1)
    n_i = feat[fi].shape[0]
    nn_i_of_j, ties0, gap0 = nn33(feat[fj], feat[fi])
    hit = np.zeros(n_i, dtype=bool)
    hit[nn_i_of_j] = True
    rows = np.nonzero(hit)[0]
    i_to_j = np.full(n_i, -1, dtype=np.int32)
    i_to_j[rows], ties1, gap1 = nn33(feat[fi][rows], feat[fj])
    return dict(nn_i_of_j=nn_i_of_j, ties0=ties0, gap0=gap0, rows=rows, i_to_j=i_to_j, ties1=ties1, gap1=gap1)


# ---------------------------------------------------------------------------------------------- the matcher
def match(xyz_s, desc_s, xyz_t, desc_t, crosscheck=True, tuple_test=True, tuple_scale=0.95, seed=0, tables_=None):
    """tables_: what tables(desc_s, desc_t) returned, to run one pair under several settings.
    -> dict: corr [L, 2] (source, target), nn_large_of_small [n_small], nn_small_of_large [n_large] (-1: not asked), swapped, nhit, cross [ncorr, 2] (the list handed to the tuple test: rows of the larger, of the smaller cloud),
    ties0 / ties1 (per query of either direction: rows attaining its minimum), gap0 / gap1 (see nn33), hit_rows,
    mean_s, mean_t"""
    xyz = [np.ascontiguousarray(np.asarray(xyz_s)[:, :3], dtype=f32), np.ascontiguousarray(np.asarray(xyz_t)[:, :3], dtype=f32)]
    feat = [np.ascontiguousarray(desc_s, dtype=f32).reshape(-1, 33), np.ascontiguousarray(desc_t, dtype=f32).reshape(-1, 33)]
    mean = [seq_mean(x) for x in xyz]
    pc = [x - m[None, :] for x, m in zip(xyz, mean)]
    fi, fj = 0, 1
    swapped = False
    if xyz[fj].shape[0] > xyz[fi].shape[0]:
        fi, fj, swapped = 1, 0, True
    n_i, n_j = xyz[fi].shape[0], xyz[fj].shape[0]
    T = tables_ if tables_ is not None else tables(feat[0], feat[1])
    nn_i_of_j, rows, i_to_j = T["nn_i_of_j"], T["rows"], T["i_to_j"]
    if crosscheck:
        keep = rows[nn_i_of_j[i_to_j[rows]] == rows]
        cross = np.stack([keep, i_to_j[keep]], axis=1).astype(np.int64)
    else:
        cross = np.concatenate([np.stack([rows, i_to_j[rows]], axis=1), np.stack([nn_i_of_j, np.arange(n_j)], axis=1)]).astype(np.int64)
    corres = cross
    if tuple_test and tuple_scale != 0:
        ncorr = cross.shape[0]
        kept = np.zeros((0, 2), dtype=np.int64)
        if ncorr > 0:
            t = np.arange(ncorr * 100, dtype=u64)
            r = [(rand_u32(seed, u64(3) * t + u64(k)) % np.uint32(ncorr)).astype(np.int64) for k in range(3)]
            scale = f32(tuple_scale)

            def length(p, a, b):
                d = p[a] - p[b]
                with np.errstate(all="ignore"):
                    return np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))

            ok = np.ones(t.shape[0], dtype=bool)
            for a, b in ((0, 1), (1, 2), (2, 0)):
                li = length(pc[fi], cross[r[a], 0], cross[r[b], 0])
                lj = length(pc[fj], cross[r[a], 1], cross[r[b], 1])
                with np.errstate(all="ignore"):
                    ok &= (li * scale < lj) & (lj < li / scale)
            kept = np.concatenate([cross[r[k][ok]] for k in range(3)])
        corres = kept
    if swapped:
        corres = corres[:, ::-1]
    corr = np.unique(corres, axis=0).astype(np.int32).reshape(-1, 2) if corres.shape[0] else np.zeros((0, 2), dtype=np.int32)
    return dict(corr=corr, nn_large_of_small=nn_i_of_j, nn_small_of_large=i_to_j, swapped=swapped, nhit=int(rows.size),
                cross=cross, ties0=T["ties0"], ties1=T["ties1"], gap0=T["gap0"], gap1=T["gap1"], hit_rows=rows,
                mean_s=mean[0], mean_t=mean[1])
