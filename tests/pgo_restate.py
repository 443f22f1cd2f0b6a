"""numpy float64 restatement of the pose-graph optimisation (include/qtr_pgo_math.h; quatro_amd/csrc/pgo.hip).

Nothing of the header or the kernels is used.  Every quantity is formed in the header's written order with numpy's binary64
+ - * / sqrt (numpy never fuses a product into a sum): arrays run ACROSS edges or nodes, never along a sum, so every sum
keeps its order — the 6-term sums from index 0 to 5, a node's sums over its incidence list in ascending edge index (one
list rank at a time, all nodes at once), a dot product as 1024 strided partials, the 64-lane fold of each of the 16 waves
and the wave sums from left to right, F in the ICP's chunk shape (eval_restate.fold_sum).  So the comparison with the header
compiled by g++ and with the device is equality of bits, not a tolerance.
"""
import numpy as np

import eval_restate as er

THREADS = 1024
LAMBDA_MAX = 1e32
PIVOT_REL = 1e-12
STOP_MAX_ITERATIONS, STOP_RELATIVE, STOP_STEP, STOP_LAMBDA, STOP_NOTHING = 1, 2, 3, 4, 5
DEFAULTS = dict(max_iterations=100, pcg_max_iterations=500, rel_tol=1e-6, step_tol=1e-9, tau=1e-5, pcg_tol=1e-8,
                line_process_weight=0.0, edge_prune_threshold=0.25)
bits = er.bits


def u(a, b):
    return (a * (11 - a)) // 2 + b if a <= b else (b * (11 - b)) // 2 + a


def inv(X):
    Y = np.zeros((X.shape[0], 12))
    for r in range(3):
        for c in range(3):
            Y[:, 4 * r + c] = X[:, 4 * c + r]
        Y[:, 4 * r + 3] = -((X[:, r] * X[:, 3] + X[:, 4 + r] * X[:, 7]) + X[:, 8 + r] * X[:, 11])
    return Y


def mul(A, B):
    C = np.zeros((A.shape[0], 12))
    for r in range(3):
        for c in range(3):
            C[:, 4 * r + c] = (A[:, 4 * r] * B[:, c] + A[:, 4 * r + 1] * B[:, 4 + c]) + A[:, 4 * r + 2] * B[:, 8 + c]
        C[:, 4 * r + 3] = ((A[:, 4 * r] * B[:, 3] + A[:, 4 * r + 1] * B[:, 7]) + A[:, 4 * r + 2] * B[:, 11]) + A[:, 4 * r + 3]
    return C


def rotmul(A, B):
    C = np.zeros((A.shape[0], 12))
    for r in range(3):
        for c in range(4):
            C[:, 4 * r + c] = (A[:, 4 * r] * B[:, c] + A[:, 4 * r + 1] * B[:, 4 + c]) + A[:, 4 * r + 2] * B[:, 8 + c]
    return C


def vee(E):
    return np.stack([0.5 * (E[:, 9] - E[:, 6]), 0.5 * (E[:, 2] - E[:, 8]), 0.5 * (E[:, 4] - E[:, 1]), E[:, 3], E[:, 7],
                     E[:, 11]], axis=1)


def generator(k, P):
    Q = np.zeros_like(P)
    if k >= 3:
        Q[:, 4 * (k - 3) + 3] = 1.0
        return Q
    a, b = (k + 1) % 3, (k + 2) % 3
    for c in range(4):
        Q[:, 4 * a + c] = -P[:, 4 * b + c]
        Q[:, 4 * b + c] = P[:, 4 * a + c]
    return Q


def residual(Xs, Xt, Z):
    """r [n, 6] and J [n, 6, 6] (J[:, a, k] = d r_a / d delta_s[k]) of n edges; poses as [n, 16]."""
    Xti = inv(Xt)
    P = mul(Xs, inv(Z))
    r = vee(mul(Xti, P))
    J = np.zeros((Xs.shape[0], 6, 6))
    for k in range(6):
        J[:, :, k] = vee(rotmul(Xti, generator(k, P)))
    return r, J


def edge_terms(Xs, Xt, Z, info, unc, mu):
    """A [n, 21], g [n, 6], chi2, w, F share [n] each."""
    r, J = residual(Xs, Xt, Z)
    om = lambda a, b: info[:, 6 * a + b] if a <= b else info[:, 6 * b + a]
    n = Xs.shape[0]
    v, B = np.zeros((n, 6)), np.zeros((n, 6, 6))
    for a in range(6):
        s = om(a, 0) * r[:, 0]
        for b in range(1, 6):
            s = s + om(a, b) * r[:, b]
        v[:, a] = s
        for k in range(6):
            t = om(a, 0) * J[:, 0, k]
            for b in range(1, 6):
                t = t + om(a, b) * J[:, b, k]
            B[:, a, k] = t
    chi2 = r[:, 0] * v[:, 0]
    for a in range(1, 6):
        chi2 = chi2 + r[:, a] * v[:, a]
    mu = np.float64(mu)
    lp = np.asarray(unc).astype(bool) & bool(mu > 0.0)
    s = mu / (mu + chi2)
    w = np.where(lp, s * s, 1.0)
    F = np.where(lp, w * chi2 + mu * ((s - 1.0) * (s - 1.0)), chi2)
    A, g = np.zeros((n, 21)), np.zeros((n, 6))
    m = 0
    for k in range(6):
        for l in range(k, 6):
            s = J[:, 0, k] * B[:, 0, l]
            for a in range(1, 6):
                s = s + J[:, a, k] * B[:, a, l]
            A[:, m] = w * s
            m += 1
        s = J[:, 0, k] * v[:, 0]
        for a in range(1, 6):
            s = s + J[:, a, k] * v[:, a]
        g[:, k] = w * s
    return A, g, chi2, w, F


def incidence(N, src, dst):
    lists = [[] for _ in range(N)]
    for e, (s, t) in enumerate(zip(src, dst)):
        lists[s].append(e)
        lists[t].append(e)
    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([e for l in lists for e in l], np.int64)


def _ranks(off):
    deg = off[1:] - off[:-1]
    for k in range(int(deg.max()) if deg.size else 0):
        yield k, np.flatnonzero(deg > k)


def node_gather(N, off, inc, src, EA, Eg):
    D, g = np.zeros((N, 21)), np.zeros((N, 6))
    for k, nodes in _ranks(off):
        e = inc[off[nodes] + k]
        D[nodes] = D[nodes] + EA[e]
        g[nodes] = np.where((src[e] == nodes)[:, None], g[nodes] + Eg[e], g[nodes] - Eg[e])
    return D, g


def matvec(N, off, inc, src, dst, EA, lam, x, free):
    """(H + lambda I) x as [N, 6]; rows of fixed nodes are 0."""
    y = np.zeros((N, 6))
    for k, nodes in _ranks(off):
        e = inc[off[nodes] + k]
        d = x[src[e]] - x[dst[e]]
        v = np.zeros((nodes.size, 6))
        for a in range(6):
            s = EA[e, u(a, 0)] * d[:, 0]
            for b in range(1, 6):
                s = s + EA[e, u(a, b)] * d[:, b]
            v[:, a] = s
        y[nodes] = np.where((src[e] == nodes)[:, None], y[nodes] + v, y[nodes] - v)
    y = y + lam * x
    y[~free] = 0.0
    return y


def solve6(U21, b):
    """qtr_icp_solve6 on n systems at once: (x [n, 6], ok [n])."""
    n = U21.shape[0]
    A = np.zeros((n, 6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[:, i, j] = A[:, j, i] = U21[:, k]
            k += 1
    L, Dg, ok = np.zeros((n, 6, 6)), np.zeros((n, 6)), np.ones(n, bool)
    for i in range(6):
        L[:, i, i] = 1.0
    for j in range(6):
        d = A[:, j, j].copy()
        for m in range(j):
            d = d - (L[:, j, m] * L[:, j, m]) * Dg[:, m]
        ok &= d > PIVOT_REL * A[:, j, j]
        Dg[:, j] = d
        for i in range(j + 1, 6):
            s = A[:, i, j].copy()
            for m in range(j):
                s = s - (L[:, i, m] * L[:, j, m]) * Dg[:, m]
            L[:, i, j] = s / d
    y, x = np.zeros((n, 6)), np.zeros((n, 6))
    for i in range(6):
        s = b[:, i].copy()
        for m in range(i):
            s = s - L[:, i, m] * y[:, m]
        y[:, i] = s
    for i in range(5, -1, -1):
        s = y[:, i] / Dg[:, i]
        for m in range(i + 1, 6):
            s = s - L[:, m, i] * x[:, m]
        x[:, i] = s
    return x, ok


def precond(D, lam, r, free, refusals=None):
    """refusals (a list, optional) receives the number of free nodes whose block solve6 refused, once per call."""
    U = D.copy()
    for a in range(6):
        U[:, u(a, a)] = U[:, u(a, a)] + lam
    x, ok = solve6(U, r)
    if refusals is not None:
        refusals.append(int((~ok & free).sum()))
    z = np.where(ok[:, None], x, r)
    z[~free] = 0.0
    return z


def dot(a, b):
    """<a, b> over the flattened vectors in the header's shape."""
    p = a.reshape(-1) * b.reshape(-1)
    rows = (p.size + THREADS - 1) // THREADS
    q = np.zeros(rows * THREADS)
    q[:p.size] = p
    acc = np.zeros(THREADS)
    for row in q.reshape(rows, THREADS):  # thread t: k = t, t + 1024, ... in ascending order (a padded 0.0 changes no bit)
        acc = acc + row
    w = acc.reshape(THREADS // 64, 64).copy()
    off = 32
    while off >= 1:
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
        off >>= 1
    s = w[0, 0]
    for k in range(1, THREADS // 64):
        s = s + w[k, 0]
    return s


def rot_from_omega(w):
    q0, q1, q2, q3 = np.ones(w.shape[0]), 0.5 * w[:, 0], 0.5 * w[:, 1], 0.5 * w[:, 2]
    nq = np.sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3))
    q0, q1, q2, q3 = q0 / nq, q1 / nq, q2 / nq, q3 / nq
    return np.stack([((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3, 2.0 * (q1 * q2 - q0 * q3), 2.0 * (q1 * q3 + q0 * q2),
                     2.0 * (q1 * q2 + q0 * q3), ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3, 2.0 * (q2 * q3 - q0 * q1),
                     2.0 * (q1 * q3 - q0 * q2), 2.0 * (q2 * q3 + q0 * q1), ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3], axis=1)


def update(X, x):
    """[dR(x[:, :3]) x[:, 3:]] X for every row (qtr_pgo_update_node: qtr_icp_rot_from_omega, qtr_icp_compose)."""
    dR = rot_from_omega(x)
    Xn = np.zeros_like(X)
    for r in range(3):
        for c in range(4):
            Xn[:, 4 * r + c] = (dR[:, 3 * r] * X[:, c] + dR[:, 3 * r + 1] * X[:, 4 + c]) + dR[:, 3 * r + 2] * X[:, 8 + c]
        Xn[:, 4 * r + 3] = Xn[:, 4 * r + 3] + x[:, 3 + r]
    Xn[:, 15] = 1.0
    return Xn


def linearize(X, src, dst, Z, info, unc, mu, off, inc, free):
    A, g, _, w, F = edge_terms(X[src], X[dst], Z, info, unc, mu)
    D, ng = node_gather(X.shape[0], off, inc, src, A, g)
    md = np.fmax.reduce(D[free][:, [u(a, a) for a in range(6)]].reshape(-1), initial=0.0) if free.any() else 0.0
    return dict(A=A, w=w, D=D, g=ng, F=er.fold_sum(F.reshape(-1, 1))[0], max_diag=np.float64(md))


def pcg(lin, lam, off, inc, src, dst, free, tol, max_its, rr_log=None, refusals=None):
    """(x [N, 6], iterations) of (H + lambda I) x = -g by the header's loop."""
    N = free.size
    D, g, A = lin["D"], lin["g"], lin["A"]
    x = np.zeros((N, 6))
    r = np.where(free[:, None], -g, 0.0)
    z = precond(D, lam, r, free, refusals)
    p = z.copy()
    rz, rr = dot(r, z), dot(r, r)
    limit = (tol * tol) * rr
    its = 0
    if rr_log is not None:
        rr_log.append(rr)
    while its < max_its and rr > limit:
        q = matvec(N, off, inc, src, dst, A, lam, p, free)
        alpha = rz / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        rr = dot(r, r)
        its += 1
        if rr_log is not None:
            rr_log.append(rr)
        if not rr > limit:
            break
        z = precond(D, lam, r, free, refusals)
        rzn = dot(r, z)
        beta = rzn / rz
        rz = rzn
        p = z + beta * p
    return x, its


def optimize(poses, fixed, src, dst, Z, info, unc, rr_log=None, refusals=None, **params):
    """The whole call.  poses [N, 16] or [N, 4, 4]; fixed None = node 0.  Returns a dict: poses [N, 16], weights [E], trace
    [1 + iterations, 8] and the fields of qtr_pgo_result.  rr_log (a list) receives <r, r> before and after every iteration
    of the first solve; refusals (a list) one count per preconditioner application of every solve: the free nodes whose
    block solve6 refused (z_i = r_i)."""
    P = dict(DEFAULTS, **params)
    f64 = np.float64
    X0 = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
    N, E = X0.shape[0], len(src)
    src, dst = np.asarray(src, np.int64).reshape(E), np.asarray(dst, np.int64).reshape(E)
    Z, info = np.asarray(Z, np.float64).reshape(E, 16), np.asarray(info, np.float64).reshape(E, 36)
    unc = np.zeros(E, bool) if unc is None else np.asarray(unc).astype(bool).reshape(E)
    free = np.arange(N) != 0 if fixed is None else ~np.asarray(fixed).astype(bool).reshape(N)
    out = dict(status=0, valid=True, iterations=0, accepted=0, pcg_iterations_total=0, n_pruned=0, objective_initial=0.0,
               objective_final=0.0, lambda_final=0.0)
    if E == 0 or not free.any():
        return dict(out, stop_reason=STOP_NOTHING, poses=X0.copy(), weights=np.ones(E), trace=np.zeros((0, 8)))
    mu, rel_tol, step_tol, tau = f64(P["line_process_weight"]), f64(P["rel_tol"]), f64(P["step_tol"]), f64(P["tau"])
    off, inc = incidence(N, src, dst)
    trace = []
    with np.errstate(all="ignore"):
        # the start is the first "trial" (qtr_pgo_decide, not started)
        Xc = X0
        cur = linearize(Xc, src, dst, Z, info, unc, mu, off, inc, free)
        F = F0 = cur["F"]
        lam = tau * cur["max_diag"]
        if not lam > 0.0:
            lam = tau
        nu, trials, accepted, pcg_last, pcg_total, reason = f64(2.0), 0, 0, 0, 0, 0
        denom = ms = f64(0.0)
        if trials >= P["max_iterations"]:
            reason = STOP_MAX_ITERATIONS
        elif not lam <= LAMBDA_MAX:
            reason = STOP_LAMBDA
        trace.append([F, lam, 0.0, 1.0, 0.0, F, 0.0, 0.0])
        first = True
        while not reason:
            x, its = pcg(cur, lam, off, inc, src, dst, free, f64(P["pcg_tol"]), P["pcg_max_iterations"],
                         rr_log if first else None, refusals)
            first = False
            uvec = np.where(free[:, None], lam * x - cur["g"], 0.0)
            ms = f64(np.fmax.reduce(np.abs(x).reshape(-1), initial=0.0))
            denom = dot(x, uvec)
            Xt = np.where(free[:, None], update(Xc, x), Xc)
            pcg_last, pcg_total = its, pcg_total + its
            if ms < step_tol:
                reason = STOP_STEP
                break
            tri = linearize(Xt, src, dst, Z, info, unc, mu, off, inc, free)
            trials += 1
            dF = F - tri["F"]
            rho = dF / denom
            acc = bool(rho > 0.0)
            if acc:
                t = 2.0 * rho - 1.0
                f = 1.0 - (t * t) * t
                third = f64(1.0) / f64(3.0)
                lam = lam * (f if f > third else third)
                nu = f64(2.0)
                if dF <= rel_tol * F:
                    reason = STOP_RELATIVE
                F, Xc, cur = tri["F"], Xt, tri
                accepted += 1
            else:
                lam = lam * nu
                nu = 2.0 * nu
            if not reason:
                if trials >= P["max_iterations"]:
                    reason = STOP_MAX_ITERATIONS
                elif not lam <= LAMBDA_MAX:
                    reason = STOP_LAMBDA
            trace.append([tri["F"], lam, rho, float(acc), float(pcg_last), F, denom, ms])
    w = cur["w"]
    return dict(out, valid=bool(np.isfinite(F)), iterations=trials, accepted=accepted, pcg_iterations_total=pcg_total,
                stop_reason=reason, n_pruned=int((unc & (w < P["edge_prune_threshold"])).sum()), objective_initial=float(F0),
                objective_final=float(F), lambda_final=float(lam), poses=Xc.copy(), weights=w.copy(),
                trace=np.array(trace, dtype=np.float64).reshape(-1, 8))


FIELDS_INT = ("valid", "iterations", "accepted", "pcg_iterations_total", "stop_reason", "n_pruned")
FIELDS_F64 = ("objective_initial", "objective_final", "lambda_final", "poses", "weights", "trace")


def differences(got, want):
    """Names of the fields of `got` whose value (bits, for the float ones) differs from want's."""
    bad = [f for f in FIELDS_INT if int(got[f]) != int(want[f])]
    for f in FIELDS_F64:
        a, b = bits(got[f]), bits(want[f])
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append(f)
    return bad


# ---- graphs the tests share ---------------------------------------------------------------------------------------------
def rot(w):
    """Rodrigues (the tests' own truth: never compared bit for bit)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def rigid(w, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(w), t
    return T


def perturb(T, rng, s_rot, s_tr):
    return rigid(rng.normal(0, s_rot, 3), rng.normal(0, s_tr, 3)) @ T


def information(rng, n_pts=200, spread=10.0):
    """An `information` as qtr_evaluate forms it: sum G^T G, G = [-[t]x | I], over random target points."""
    t = rng.uniform(-spread, spread, (n_pts, 3)) * np.array([1.0, 1.0, 0.2])
    I = np.zeros((6, 6))
    for p in t:
        G = np.zeros((3, 6))
        G[:, :3] = -np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        G[:, 3:] = np.eye(3)
        I += G.T @ G
    return I


def measurement(Xs, Xt):
    """Z of an exact edge s -> t: X_t^-1 X_s."""
    return np.linalg.inv(Xt) @ Xs


def ring(N, n_loops, seed, drift=(0.02, 0.1), noise=(0.0, 0.0), n_uncertain=0, extra=0, radius=None):
    """A ring trajectory of N poses with odometry edges (i + 1 -> i), n_loops chords and `extra` further chords, the start
    drifted.  Returns dict(truth, poses, src, dst, Z, info, unc)."""
    rng = np.random.default_rng(seed)
    R = radius or max(5.0, N * 0.3)
    truth = np.stack([rigid([0.05 * np.sin(i), 0.03 * np.cos(2 * i), 2 * np.pi * i / N + np.pi / 2],
                            [R * np.cos(2 * np.pi * i / N), R * np.sin(2 * np.pi * i / N), 0.2 * np.sin(i)]) for i in range(N)])
    pairs = [(i + 1, i) for i in range(N - 1)]
    if N > 2:
        pairs.append((0, N - 1))
    chords = set()
    while len(chords) < min(n_loops + extra, max(0, N * (N - 3) // 2)):
        a, b = sorted(rng.choice(N, 2, replace=False))
        if b - a > 1 and not (a == 0 and b == N - 1):
            chords.add((int(b), int(a)))
    pairs += sorted(chords)
    E = len(pairs)
    src, dst = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    Z = np.stack([perturb(measurement(truth[s], truth[t]), rng, *noise) if noise[0] or noise[1]
                  else measurement(truth[s], truth[t]) for s, t in pairs])
    info = np.stack([information(rng) for _ in pairs])
    unc = np.zeros(E, np.uint8)
    unc[E - n_uncertain:] = 1 if n_uncertain else 0
    poses = truth.copy()
    acc = np.eye(4)
    for i in range(1, N):  # a drift that grows along the trajectory
        acc = rigid(rng.normal(0, drift[0], 3), rng.normal(0, drift[1], 3)) @ acc
        poses[i] = acc @ truth[i]
    return dict(truth=truth, poses=poses, src=src, dst=dst, Z=Z, info=info, unc=unc)


def graphs():
    """The four graphs of the issue: N = 2 / E = 1, a 5-ring, N = 65 / E = 70, N = 300 / E = 340 with 12 uncertain edges."""
    g2 = ring(2, 0, 1)
    g5 = ring(5, 0, 2, noise=(0.01, 0.05))
    g65 = ring(65, 5, 3, noise=(0.01, 0.05))
    g300 = ring(300, 40, 4, noise=(0.005, 0.03), n_uncertain=12)
    assert (len(g2["src"]), len(g5["src"]), len(g65["src"]), len(g300["src"])) == (1, 5, 70, 340)
    return {"n2_e1": g2, "ring5": g5, "n65_e70": g65, "n300_e340": g300}
