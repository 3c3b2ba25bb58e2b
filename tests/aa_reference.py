"""A float64 restatement of archetypal analysis as xeofs_amd.single.ArchetypalAnalysis defines it (its module docstring), written
from the definition and sharing no code with the model: the projection onto the probability simplex by sorting (and
Michelot's fixed point beside it), the FurthestSum start, the projected-gradient step of the scores, and the full alternating
algorithm on a Gram matrix K -- either with its own adaptive step, or replaying a recorded sequence of (mu, inner count) steps.
Used by the CPU test of the restatement itself and by the GPU tests of the operators and of the model."""

import numpy as np


# ------------------------------------------------------------------------------------------------ the projection
def project_sort(U):
    """rows of U [r x m] (float64) -> (their Euclidean projections onto {x >= 0, sum x = 1}, tau [r]): sort descending, the
    largest rho with s_rho - (sum_{j <= rho} s_j - 1) / rho > 0, tau = (sum_{j <= rho} s_j - 1) / rho (Held et al. 1974)"""
    U = np.atleast_2d(np.asarray(U, dtype=np.float64))
    r, m = U.shape
    s = -np.sort(-U, axis=1)
    css = np.cumsum(s, axis=1) - 1.0
    ks = np.arange(1, m + 1, dtype=np.float64)
    ok = s - css / ks > 0.0
    rho = m - 1 - np.argmax(ok[:, ::-1], axis=1)              # the last True of every row (the first is always True)
    tau = css[np.arange(r), rho] / (rho + 1.0)
    return np.maximum(U - tau[:, None], 0.0), tau


def project_michelot(u):
    """one row (float64) -> (projection, tau, rounds): S = all; tau = (sum_S u - 1) / |S|; thr = the largest tau so far;
    S = {u > thr}; until |S| stands still"""
    u = np.asarray(u, dtype=np.float64)
    S = np.ones(u.size, dtype=bool)
    tau = thr = (u.sum() - 1.0) / u.size
    rounds = 1
    while True:
        S2 = u > thr
        if S2.sum() == S.sum() or S2.sum() == 0:
            break
        S = S2
        tau = (u[S].sum() - 1.0) / S.sum()
        thr = max(thr, tau)
        rounds += 1
    return np.where(u > thr, u - tau, 0.0), tau, rounds


def active_count(U, tau):
    """|{j : u_ij > tau_i}| per row"""
    return (np.atleast_2d(U) > np.asarray(tau, dtype=np.float64).reshape(-1, 1)).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the start
def furthest_sum(K, k, start):
    """k - 1 greedy picks by the largest sum of distances d(i, j) = sqrt(max(K_ii + K_jj - 2 K_ij, 0)) to the picks so far,
    then (k >= 2) one sweep that takes each pick out in turn and picks again; the lowest index wins ties"""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    dg = np.diag(K)
    D = np.sqrt(np.maximum(dg[:, None] + dg[None, :] - 2.0 * K, 0.0))
    picks = [int(start)]

    def best(others):
        total = D[others].sum(axis=0) if others else np.zeros(n)
        total = total.copy()
        total[others] = -np.inf
        return int(np.argmax(total))

    while len(picks) < k:
        picks.append(best(picks))
    if k >= 2:
        for t in range(k):
            others = picks[:t] + picks[t + 1:]
            picks[t] = best(others)
    return np.asarray(picks, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the A step
def pg_steps(A, Q, M, inv_L, iters, round_m=True):
    """`iters` times a <- P(a - inv_L (a M - q)) on every row, in float64; M rounded once to float32 first, as the kernel does"""
    A = np.array(A, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    if round_m:
        M = M.astype(np.float32).astype(np.float64)
    for _ in range(int(iters)):
        A = project_sort(A - float(inv_L) * (A @ M - Q))[0]
    return A


def lambda_max(M):
    M = np.asarray(M, dtype=np.float64)
    return float(np.linalg.eigvalsh(0.5 * (M + M.T))[-1])


def objective_gram(trK, A, Q, B):
    """f = trK - 2 <A, Q> + <A^T A, B Q>"""
    return float(trK - 2.0 * np.sum(A * Q) + np.sum((A.T @ A) * (B @ Q)))


def objective_direct(X, A, B):
    X = np.asarray(X, dtype=np.float64)
    R = X - A @ (B @ X)
    return float(np.sum(R * R))


# ------------------------------------------------------------------------------------------------ the algorithm
def fit(K, k, idx, max_iter=500, tol=1e-6, inner_iter=10, init_iter=50, replay=None, max_rejections=40):
    """The alternating algorithm on K [n x n] from the start indices idx, in float64.  replay: a list of dicts with "mu",
    "inner" and "accepted" (the model's stats["steps"]): the A step runs "inner" iterations and the B step is the projection
    with "mu", taken without a trial (skipped where "accepted" is False); max_iter, tol and the step rule are then unused.
    -> dict(A, B, f, history, steps, trK, stalled, products)"""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    trK = float(np.trace(K))
    B = np.zeros((k, n))
    B[np.arange(k), np.asarray(idx)] = 1.0
    A = np.full((n, k), 1.0 / k)
    Q = K @ B.T
    f = objective_gram(trK, A, Q, B)
    f_start = f
    mu = 1.0 / (lambda_max(A.T @ A) * trK)
    rejected_ever = stalled = False
    history, steps = [], []
    products = 1
    for it in range(len(replay) if replay is not None else max_iter):
        M = B @ Q
        if replay is not None:
            rec = replay[it]
            A = pg_steps(A, Q, M, 1.0 / lambda_max(M), rec["inner"], round_m=False)
            if rec.get("accepted", True):
                S = A.T @ A
                G = (S @ B - A.T) @ K
                B = project_sort(B - rec["mu"] * G)[0]
                Q = K @ B.T
                products += 2
            history.append(objective_gram(trK, A, Q, B))
            continue
        iters = init_iter if it == 0 else inner_iter
        A = pg_steps(A, Q, M, 1.0 / lambda_max(M), iters, round_m=False)
        S = A.T @ A
        fA = objective_gram(trK, A, Q, B)
        G = (S @ B - A.T) @ K
        products += 1
        rej = 0
        while True:
            Bn = project_sort(B - mu * G)[0]
            Qn = K @ Bn.T
            products += 1
            fn = objective_gram(trK, A, Qn, Bn)
            used = mu
            if fn <= fA:
                B, Q = Bn, Qn
                mu *= 1.2 if rejected_ever else 2.0
                break
            rejected_ever = True
            rej += 1
            mu /= 2.0
            if rej == max_rejections:
                stalled, fn = True, fA
                break
        steps.append(dict(mu=used, inner=iters, rejections=rej, f=fn, accepted=not stalled))
        history.append(fn)
        f_prev, f = f, fn
        if stalled or (rejected_ever and f_prev - f <= tol * trK):
            break
    order = np.argsort(-A.sum(axis=0), kind="stable")
    return dict(A=A[:, order], B=B[order], f=history[-1] if history else f_start, f_start=f_start,
                history=np.asarray(history), steps=steps, trK=trK, stalled=stalled, products=products, order=order)


# ------------------------------------------------------------------------------------------------ designed fields
def planted_field(n=96, p=130, k=3, vertices=(5, 40, 77), seed=0):
    """-> (X [n x p] float64, W [n x k] the planted convex weights): rows `vertices` are the pure archetypes (random Gaussian
    patterns), every other row a Dirichlet(1) mixture of them"""
    rs = np.random.RandomState(seed)
    Z = rs.standard_normal((k, p))
    W = rs.dirichlet(np.ones(k), size=n)
    for j, v in enumerate(vertices):
        W[v] = 0.0
        W[v, j] = 1.0
    return W @ Z, W


def noisy_mixtures(n, p, k, seed=0, noise=0.3):
    """Dirichlet(0.5) mixtures of k Gaussian patterns plus white noise"""
    rs = np.random.RandomState(seed)
    Z = rs.standard_normal((k, p))
    W = rs.dirichlet(0.5 * np.ones(k), size=n)
    return W @ Z + noise * rs.standard_normal((n, p))
