"""No-GPU checks of tests/graph_cases.py, the adversarial inputs of tests/test_gpu_graph_edges.py:

  * the reference is pinned: the oracle's build_graph equals a numpy binary64 restatement of the reference's solveForScale
    (include/quatro.hpp: the two divisions, cwiseInverse, norms as e0 + (e1 + e2)) on every case;
  * the cases stay adversarial: the share of block pairs at the threshold, the exact ties and how the reference splits
    them, the squared norms against the MFMA kernel's range limit, the subnormal binary16 halves — conditions a later edit
    of the generators has to keep;
  * the software part of k_graph_build_mfma's error bound (quatro_amd/csrc/solver.hip: 27.1 u M, of which 16.1 u M are the
    matrix unit's accumulation, measured on the device by tests/gpu_checks/mfma_f16_accumulation.hip) holds on a numpy
    model of gbm_records: |R_model - (-|P - P'|^2 / 2)| <= 11 u M + 2e-6;
  * pair_consistent's squared-form shortcut, restated in numpy, never decides a pair against the verbatim expression.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_cases as gc  # noqa: E402

L = 2111  # the larger of the two sizes the product library is run at (nb = 33: a last row block of 63 rows)
U = 2.0 ** -24
NAMES = list(gc.CASES)
FINITE = [n for n in NAMES if not n.startswith("nonfinite")]


def _block_pairs(c):
    lo, hi = c.block
    i, j = np.triu_indices(hi - lo, 1)
    return i + lo, j + lo


def _rel_norms(c):
    """squared norms relative to correspondence 0 in binary32, as gbm_records forms them: (n_src, n_tgt)"""
    out = []
    with np.errstate(all="ignore"):
        for cloud in (c.src, c.tgt):
            x = cloud[:, :3] - cloud[0, :3]
            out.append(x[:, 0] * x[:, 0] + (x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]))
    assert out[0].dtype == np.float32
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_graph_equals_the_numpy_restatement_of_solveForScale(qo, name):
    c = gc.case(name, L)
    assert c.src.dtype == np.float32 and c.src.shape == (L, 4) and c.tgt.shape == (L, 4)
    assert 2 * c.noise_bound * np.sqrt(c.cbar2) == gc.beta_of(c.noise_bound, c.cbar2)
    lo, hi = c.block
    assert 1 <= lo and hi <= L and hi - lo == gc.BLOCK
    bm = qo.build_graph(c.src, c.tgt, c.noise_bound, c.cbar2)
    want = gc.restate_graph(c)
    got = gc.bits_of(bm, L)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(want, want.T)
    if name.startswith("nonfinite"):
        bad = ~(np.isfinite(c.src).all(1) & np.isfinite(c.tgt).all(1))
        assert bad.sum() >= 8 and bad[L - 1] and bad[0] == (name == "nonfinite_row0")
        assert not want[bad].any() and not want[:, bad].any()
    # the whole graph stays sparse outside the block (a short solve)
    out = np.ones(L, bool)
    out[lo:hi] = False
    assert want[out].mean() < 0.3


def test_generators_are_deterministic_and_scale_down():
    a, b = gc.CASES["band_0.6"](300), gc.CASES["band_0.6"](300)
    assert np.array_equal(a.src, b.src) and np.array_equal(a.tgt, b.tgt) and a.block == b.block
    for name in NAMES:
        for n in (130, 257):
            c = gc.case(name, n)
            assert c.src.shape == (n, 4) and c.block[1] - c.block[0] == n // 2 and c.block[0] >= 1


@pytest.mark.parametrize("name", NAMES)
def test_share_of_block_pairs_at_the_threshold(name, capsys):
    """band cases: >= 1 % of the block's pairs within 1e-5 beta of the threshold, >= 20 % within 1e-2 beta, both decisions
    among the former.  (The counts of every case are printed: run with -s.)"""
    c = gc.case(name, L)
    beta = gc.beta_of(c.noise_bound)
    a, b = gc.pair_lengths(c)
    i, j = _block_pairs(c)
    with np.errstate(invalid="ignore"):
        dist = np.abs(np.abs(b[i, j] - a[i, j]) - beta)
        near5, near2 = dist < 1e-5 * beta, dist < 1e-2 * beta
    dec = gc.restate_graph(c)[i, j]
    with capsys.disabled():
        print(f"\n[graph_cases] {name}: {i.size} block pairs, {int(near5.sum())} within 1e-5 beta "
              f"({int(dec[near5].sum())} accepted), {int(near2.sum())} within 1e-2 beta", end="")
    if name in gc.BAND_CASES:
        assert near5.sum() >= 0.01 * i.size
        assert near2.sum() >= 0.20 * i.size
        assert dec[near5].any() and not dec[near5].all()


def test_exact_ties_are_exact_and_the_reference_splits_them(capsys):
    c = gc.case("exact_ties", L)
    assert gc.beta_of(c.noise_bound) == 0.5
    a, b = gc.pair_lengths(c)
    i, j = _block_pairs(c)
    tie = np.abs(b[i, j] - a[i, j]) == 0.5
    dec = gc.restate_graph(c)[i, j]
    n, acc = int(tie.sum()), int(dec[tie].sum())
    with capsys.disabled():
        print(f"\n[graph_cases] exact_ties: {n} pairs with |b - a| == beta, {acc} accepted, {n - acc} rejected", end="")
    assert n >= 20000
    assert acc >= 0.1 * n and n - acc >= 0.1 * n


@pytest.mark.parametrize("d", [250, 330, 2000])
def test_far_origin_norms_sit_on_both_sides_of_the_range_limit(d):
    c = gc.case(f"far_origin_{d}", L)
    ns, nt = _rel_norms(c)
    for n in (ns, nt):
        assert (n.max() < 1e5) == (d == 250), (d, n.max())
    if d == 330:
        # tiles of the block on both sides of the kernel's `safe` test: largest row norm + largest column norm < 1e5
        nb = (L + 63) // 64
        pad = np.full(nb * 64 - L, -np.inf, np.float32)
        gs = np.concatenate([ns, pad]).reshape(nb, 64).max(1)
        gt = np.concatenate([nt, pad]).reshape(nb, 64).max(1)
        blk = [k for k in range(nb) if c.block[0] <= 64 * k and 64 * k + 64 <= c.block[1]]  # row blocks inside the block
        safe = [(gs[p] + gs[q] < 1e5) and (gt[p] + gt[q] < 1e5) for p in blk for q in blk if p <= q]
        assert sum(safe) >= 3 and len(safe) - sum(safe) >= 3, (sum(safe), len(safe))


def _halves(x):
    """binary32 -> its two binary16 halves (gbm_records)"""
    x1 = x.astype(np.float16)
    x2 = (x - x1.astype(np.float32)).astype(np.float16)
    return x1, x2


def test_flat_block_has_subnormal_second_halves():
    c = gc.case("flat", L)
    lo, hi = c.block
    tiny = np.float16(2.0 ** -14)  # the smallest normal binary16
    for cloud in (c.src, c.tgt):
        rel = cloud[lo:hi, 1:3] - cloud[0, 1:3]
        assert np.abs(rel).max() <= 1.01e-3
        x1, x2 = _halves(rel)
        assert np.mean(np.abs(x2) < tiny) >= 0.5
        assert np.any(x2 != 0)


def _mfma_model(cloud):
    """R (L x L, binary64) of gbm_records' operands: origin subtraction in binary32, coordinates and a = -0.5f n split in
    two binary16 halves, the sixteen products of row i's and column j's operands exact, summed in binary64"""
    with np.errstate(all="ignore"):
        x = cloud[:, :3] - cloud[0, :3]
        n = x[:, 0] * x[:, 0] + (x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
        a = np.float32(-0.5) * n
        assert x.dtype == np.float32 and a.dtype == np.float32
        x1, x2 = _halves(x)
        a1, a2 = _halves(a)
        one = np.ones(x.shape[0])
        f = lambda v: v.astype(np.float64)
        row, col = [], []
        for k in range(3):
            row += [f(x1[:, k]), f(x1[:, k]), f(x2[:, k]), f(x2[:, k])]
            col += [f(x1[:, k]), f(x2[:, k]), f(x1[:, k]), f(x2[:, k])]
        row += [f(a1), f(a2), one, one]
        col += [one, one, f(a1), f(a2)]
        R = np.zeros((x.shape[0], x.shape[0]))
        for r_, c_ in zip(row, col):  # (sixteen outer products, each exact in binary64: 11-bit x 11-bit significands)
            R += r_[:, None] * c_[None, :]
        return R


@pytest.mark.parametrize("name", FINITE)
def test_software_part_of_the_mfma_bound_holds(name, capsys):
    """|R_model - (-|P - P'|^2 / 2)| <= 11 u M + 2e-6 on all pairs with M < 1e5 (both clouds): the kernel comment's
    27.1 u M minus the 16.1 u M it budgets for the matrix unit's accumulation."""
    c = gc.case(name, L)
    worst, cnt = 0.0, 0
    for cloud in (c.src, c.tgt):
        R = _mfma_model(cloud)
        p = cloud[:, :3].astype(np.float64)
        q = p - p[0]
        n = (q * q).sum(1)
        M = n[:, None] + n[None, :]
        exact = np.zeros((L, L))
        for k in range(3):
            d = p[:, None, k] - p[None, :, k]
            exact -= 0.5 * d * d
        sel = M < 1e5
        with np.errstate(invalid="ignore"):
            err = np.abs(R - exact)
        assert np.all(err[sel] <= 11 * U * M[sel] + 2e-6), (name, float((err[sel] / (11 * U * M[sel] + 2e-6)).max()))
        big = sel & (M >= 1.0)
        if big.any():
            worst = max(worst, float((err[big] / (U * M[big])).max()))
        cnt += int(sel.sum())
    with capsys.disabled():
        print(f"\n[graph_cases] {name}: {cnt} pairs with M < 1e5, largest |R_model - exact| / (u M) = {worst:.2f} "
              f"(over M >= 1; 11 allowed)", end="")
    if not name.startswith("far_origin") and name != "map_frame_wide":
        assert cnt > L * L  # the bound was tried on more than half of the pairs


@pytest.mark.parametrize("name", NAMES)
def test_squared_form_shortcut_never_decides_against_the_verbatim_expression(name):
    """pair_consistent (solver.hip) restated: with s, t the squared lengths (within a factor 256 of each other) and
    u = s + t - beta^2 > 0 it rejects when u^2 > 4 s t (1 + 1e-9), accepts when u^2 < 4 s t (1 - 1e-9), and evaluates the
    reference expression otherwise."""
    c = gc.case(name, L)
    beta = gc.beta_of(c.noise_bound)
    with np.errstate(all="ignore"):
        st = []
        for cloud in (c.src, c.tgt):
            p = cloud[:, :3].astype(np.float64)
            d = [p[None, :, k] - p[:, None, k] for k in range(3)]
            st.append(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]))
    rej, acc = _shortcut(st[0], st[1], beta)
    want = gc.restate_graph(c)
    off = ~np.eye(L, dtype=bool)
    assert not (want & rej & off).any() and (want | ~acc | ~off).all()


def _shortcut(s, t, beta):
    """(rejected, accepted) by the squared form of pair_consistent: lengths within a factor 16, outside the 1e-9 band"""
    with np.errstate(all="ignore"):
        u = s + t - beta * beta
        ok = (s > 0.0) & (t > 0.0) & (s < 256.0 * t) & (t < 256.0 * s) & (u > 0.0)
        lhs, rhs = u * u, 4.0 * s * t
        rej = ok & (lhs > rhs * (1.0 + 1e-9))
        acc = ok & ~rej & (lhs < rhs * (1.0 - 1e-9))
    return rej, acc


@pytest.mark.parametrize("beta", [0.6, 0.5, 6.0, 0.004])
def test_squared_form_shortcut_at_extreme_length_ratios(beta):
    """graph_cases.extreme_ratio_tims (what tests/test_gpu_graph_edges.py feeds qtr_scale_mask): without the limit on the
    ratio of the lengths the 1e-9 band decided ~10 % of these pairs against the reference expression."""
    ts, tt = gc.extreme_ratio_tims(beta)
    s = ts[0] * ts[0] + (ts[1] * ts[1] + ts[2] * ts[2])
    t = tt[0] * tt[0] + (tt[1] * tt[1] + tt[2] * tt[2])
    rej, acc = _shortcut(s, t, beta)
    want = gc.restate_mask(ts, tt, beta)
    assert want.any() and not want.all()
    assert not (want & rej).any() and not (~want & acc).any()
    # the inputs do reach the trap: the squared form's two sides are within 1e-6 of each other for most pairs
    with np.errstate(all="ignore"):
        u = s + t - beta * beta
        assert np.mean(np.abs(u * u / (4.0 * s * t) - 1.0) < 1e-6) > 0.5
