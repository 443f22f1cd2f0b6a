"""Second restatements of the back end's stages, written from the reference's text in plain Python / numpy (IEEE binary64):
what tests/test_oracle_cpu.py and tests/test_finalize_cases_cpu.py hold the CPU oracle against.  No GPU work, no oracle."""
import numpy as np


def ref_cote_python(X, r, median):
    """Quatro::estimate (reference include/quatro.hpp:618-747) written again, directly from the reference text, as plain
    Python floats (IEEE binary64, the same operation order); r: one range or one per element; std::sort's unspecified
    order among equal keys taken as insertion order (the oracle's definition); ranges.sum() taken sequentially."""
    N = len(X)
    R = [float(r)] * N if np.isscalar(r) else [float(v) for v in r]
    h = []
    for i in range(N):
        h.append((X[i] - R[i], i + 1))
        h.append((X[i] + R[i], -i - 1))
    h.sort(key=lambda e: e[0])  # stable
    ranges_inverse_sum = 0.0
    for i in range(N):
        ranges_inverse_sum += R[i]
    dot_X_weights = dot_weights_consensus = sum_xi = sum_xi_square = 0.0
    card = 0
    x_hat, x_cost, set_card = [], [], []
    for key, tag in h:
        idx = abs(tag) - 1
        eps = 1 if tag > 0 else -1
        w = 1.0 / (R[idx] * R[idx])
        card += eps
        dot_weights_consensus += eps * w
        dot_X_weights += eps * w * X[idx]
        ranges_inverse_sum -= eps * R[idx]
        sum_xi += eps * X[idx]
        sum_xi_square += eps * X[idx] * X[idx]
        set_card.append(card)
        xh = dot_X_weights / dot_weights_consensus if dot_weights_consensus != 0 else float("nan")
        x_hat.append(xh)
        x_cost.append(card * xh * xh + sum_xi_square - 2 * sum_xi * xh + ranges_inverse_sum)
    mi = min(range(2 * N), key=lambda i: (x_cost[i], i))  # Eigen minCoeff: first minimum
    n_card = set_card[mi]
    if median:
        cand = sorted(X[abs(h[mi - j][1]) - 1] for j in range(n_card))
        est = (cand[len(cand) // 2 - 1] + cand[len(cand) // 2]) / 2.0 if n_card >= 2 else (cand[0] if n_card == 1 else x_hat[mi])
    else:
        est = x_hat[mi]
    return est, n_card, [abs(x - est) <= ri for x, ri in zip(X, R)]


def ref_gnc_rotation2d_numpy(src, dst, noise_bound, gnc_factor, max_iter, cost_thr):
    """solveForRotation2D (reference include/quatro.hpp:430-572) with teaser::utils::svdRot2d (include/teaser/utils.h:
    151-166) written again from the reference text: numpy SVD, sequential cost sum."""
    X, Y = np.asarray(src, dtype=np.float64).T, np.asarray(dst, dtype=np.float64).T  # 2 x M
    M = X.shape[1]
    w = np.ones(M)
    mu, prev_cost, cost = 1.0, np.inf, np.inf
    nb_sq = noise_bound ** 2
    if nb_sq < 1e-16:
        nb_sq = 1e-2
    R = np.eye(2)
    iters = 0
    for i in range(max_iter):
        iters = i + 1
        H = (X * w) @ Y.T
        U, _, Vt = np.linalg.svd(H)
        V = Vt.T
        if np.linalg.det(U) * np.linalg.det(V) < 0:
            V[:, 1] *= -1
        R = V @ U.T
        res = ((Y - R @ X) ** 2).sum(0)
        if i == 0:
            mu = 1 / (2 * res.max() / nb_sq - 1)
            if mu <= 0:
                break
        th1, th2 = (mu + 1) / mu * nb_sq, mu / (mu + 1) * nb_sq
        cost = 0.0
        for j in range(M):
            cost += w[j] * res[j]
            if res[j] >= th1:
                w[j] = 0
            elif res[j] <= th2:
                w[j] = 1
            else:
                w[j] = np.sqrt(nb_sq * mu * (mu + 1) / res[j]) - mu
        cost_diff = abs(cost - prev_cost)
        mu *= gnc_factor
        prev_cost = cost
        if cost_diff < cost_thr:
            break
    return R, cost, iters, w >= 0.4


def ref_gnc_rotation3d_numpy(X, Y, nb, factor, max_iter, thr):
    """The 3-DoF loop (TEASER++'s GNC-TLS rotation, the loop solveForRotation2D was derived from) with numpy's SVD-based
    svdRot (reference include/teaser/utils.h:123-149) and a sequential cost sum.  X / Y: M x 3."""
    X, Y = X.T, Y.T
    M = X.shape[1]
    w = np.ones(M)
    mu, prev, cost, iters = 1.0, np.inf, np.inf, 0
    nb_sq = nb * nb if nb * nb >= 1e-16 else 1e-2
    R = np.eye(3)
    for i in range(max_iter):
        iters = i + 1
        U, _, Vt = np.linalg.svd((X * w) @ Y.T)
        V = Vt.T
        if np.linalg.det(U) * np.linalg.det(V) < 0:
            V[:, 2] *= -1
        R = V @ U.T
        res = ((Y - R @ X) ** 2).sum(0)
        if i == 0:
            mu = 1 / (2 * res.max() / nb_sq - 1)
            if mu <= 0:
                break
        th1, th2 = (mu + 1) / mu * nb_sq, mu / (mu + 1) * nb_sq
        cost = 0.0
        for j in range(M):
            cost += w[j] * res[j]
            w[j] = 0 if res[j] >= th1 else 1 if res[j] <= th2 else np.sqrt(nb_sq * mu * (mu + 1) / res[j]) - mu
        d = abs(cost - prev)
        mu *= factor
        prev = cost
        if d < thr:
            break
    return R, cost, iters, w >= 0.4
