"""A float64 restatement of independent component analysis (xeofs_amd.single.ICA, csrc/eofx_ica.hpp) for the tests: the contrast
functions, one step of parallel FastICA, the symmetric decorrelation, the loop with scikit-learn's stopping rule, the contrast of
a solution, the model's host steps, and the error bounds the GPU tests hold the operator to.  `f32=True` rounds the projection
s (the fmaf chain emulated: every product of two float32 is exact in float64, the sum is rounded to float32 once per term), g, g'
and G to float32 as the kernel does; the sums stay float64.  tests/test_ica_reference_cpu.py pins the float64 form to
sklearn.decomposition.FastICA(whiten=False)."""

import numpy as np

U32 = 2.0 ** -24
FUNS = ("logcosh", "exp", "cube")
# The largest absolute errors of the device's g and g' and the largest error of G relative to 1 + |G| (logcosh over alpha = 1,
# 1.5, 2; exp) seen over the sweep of tests/test_gpu_ica_step.py::test_contrast_error_sweep against float64 numpy, DOUBLED
# because the sweep is not exhaustive: (eps_g, eps_g', eps_G).  cube holds no transcendental: its bounds
# follow from the formulas (two roundings each for g and g', three for G: relative errors below 3 2^-24).
EPS_MEASURED = {"logcosh": (7.4e-8, 1.9e-7, 1.2e-7), "exp": (7.2e-8, 8.1e-8, 3.5e-8)}
EPS_G = {fun: tuple(2.0 * e for e in v) for fun, v in EPS_MEASURED.items()}
CUBE_REL = 3.0 * 2.0 ** -24 * 1.0001


def r32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def contrast(s, fun, alpha=1.0, f32=False):
    """g, g', G at s (float64 arrays); with f32 the kernel's float32 formulas, every operation rounded"""
    s = np.asarray(s, dtype=np.float64)
    if not f32:
        if fun == "logcosh":
            u = alpha * s
            g = np.tanh(u)
            return g, alpha * (1.0 - g * g), (np.abs(u) + np.log1p(np.exp(-2.0 * np.abs(u))) - np.log(2.0)) / alpha
        if fun == "exp":
            e = np.exp(-0.5 * s * s)
            return s * e, (1.0 - s * s) * e, -e
        return s ** 3, 3.0 * s * s, 0.25 * s ** 4
    f = np.float32
    s = s.astype(f)
    with np.errstate(over="ignore", under="ignore"):
        if fun == "logcosh":
            a_ = f(alpha)
            u = a_ * s
            a = np.abs(u)
            g = np.tanh(u)
            gp = a_ * r32(1.0 - g.astype(np.float64) ** 2).astype(f)
            G = ((a + np.log1p(np.exp(f(-2.0) * a))) - f(0.69314718055994531)) / a_
        elif fun == "exp":
            e = np.exp(f(-0.5) * (s * s))
            with np.errstate(invalid="ignore"):
                gp = np.where(e == 0, f(0.0), r32(1.0 - s.astype(np.float64) ** 2).astype(f) * e)
            g, G = s * e, -e
        else:
            p = s * s
            g, gp, G = p * s, f(3.0) * p, f(0.25) * (p * p)
    return g.astype(np.float64), gp.astype(np.float64), G.astype(np.float64)


def finite_rows(Z):
    return np.isfinite(np.asarray(Z, dtype=np.float64)).all(axis=1)


def project(Z, W, f32=False):
    """S [n x q], s_ij = sum_i' W[j, i'] Z[i, i']"""
    Z = np.asarray(Z, dtype=np.float64)
    if not f32:
        return Z @ np.asarray(W, dtype=np.float64).T
    Wf = r32(W)
    S = np.zeros((Z.shape[0], Wf.shape[0]))
    for i in range(Z.shape[1]):
        S = r32(Z[:, i:i + 1] * Wf[:, i][None, :] + S)
    return S


def moments(Z, W, fun, alpha=1.0, f32=False):
    """-> W1 = g^T z / nused - diag(mean g') W, gmean, nused over the rows without a NaN or an infinity"""
    Z = np.asarray(Z, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    ok = finite_rows(Z)
    Zu = Z[ok]
    nused = int(ok.sum())
    g, gp, G = contrast(project(Zu, W, f32), fun, alpha, f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        W1 = (g.T @ Zu) / nused - (gp.sum(axis=0) / nused)[:, None] * W
        gmean = G.sum(axis=0) / nused
    return W1, gmean, nused


def sym_decorrelation(W):
    """(W W^T)^-1/2 W by the eigendecomposition of W W^T: scikit-learn's route"""
    s, u = np.linalg.eigh(W @ W.T)
    s = np.clip(s, np.finfo(np.float64).tiny, None)
    return np.linalg.multi_dot([u * (1.0 / np.sqrt(s)), u.T, W])


def polar(W):
    """the orthogonal polar factor by the SVD"""
    U, _, Vt = np.linalg.svd(W)
    return U @ Vt


def degenerate(W1, nused):
    if nused == 0 or not np.isfinite(W1).all():
        return True
    sv = np.linalg.svd(W1, compute_uv=False)
    return not sv[-1] ** 2 > W1.shape[0] * 2.0 ** -52 * sv[0] ** 2


def step(Z, W, fun, alpha=1.0, f32=False):
    """-> dict(W1, gmean, nused, W (None where degenerate), lim)"""
    W1, gmean, nused = moments(Z, W, fun, alpha, f32)
    if degenerate(W1, nused):
        return dict(W1=W1, gmean=gmean, nused=nused, W=None, lim=np.nan)
    Wn = sym_decorrelation(W1)
    lim = float(np.max(np.abs(np.abs(np.einsum("ij,ij->i", Wn, W)) - 1.0)))
    return dict(W1=W1, gmean=gmean, nused=nused, W=Wn, lim=lim)


def run(Z, W0, fun, alpha=1.0, tol=1e-4, max_iter=200, f32=False):
    """the loop from an ORTHOGONAL start -> dict(W, iters, status, lims, path): path[t] is the W that iteration t starts from"""
    W = np.array(W0, dtype=np.float64)
    lims, path, status, it = [], [], 0, 0
    while it < max_iter and status == 0:
        path.append(W.copy())
        st = step(Z, W, fun, alpha, f32)
        if st["W"] is None:
            status = 2
            break
        W, it = st["W"], it + 1
        lims.append(st["lim"])
        if st["lim"] < tol:
            status = 1
    return dict(W=W, iters=it, status=status, lims=np.array(lims), path=path)


def gamma(fun, alpha=1.0):
    """E[G(nu)] for a standard normal nu: closed forms for cube and exp, 64-point Gauss-Hermite for logcosh"""
    if fun == "cube":
        return 0.75
    if fun == "exp":
        return -1.0 / np.sqrt(2.0)
    x, w = np.polynomial.hermite.hermgauss(64)
    return float((w * contrast(np.sqrt(2.0) * x, "logcosh", alpha)[2]).sum() / np.sqrt(np.pi))


def contrast_value(gmean, fun, alpha=1.0):
    return float(((np.asarray(gmean, dtype=np.float64) - gamma(fun, alpha)) ** 2).sum())


def starts(q, R, random_state=None):
    """[R x q x q]: every restart normal(size=(q, q)) from one RandomState in restart order, decorrelated"""
    rs = np.random.RandomState(random_state)
    return np.stack([sym_decorrelation(rs.normal(size=(q, q))) for _ in range(R)])


def whiten(S):
    """Z = S diag(sqrt(n) / sigma_j) in float32 as the model forms it, and sigma"""
    S64 = np.asarray(S, dtype=np.float64)
    sigma = np.sqrt((S64 * S64).sum(axis=0))
    return np.asarray(S, dtype=np.float32) * (np.sqrt(S64.shape[0]) / sigma).astype(np.float32), sigma


def fit(Z, W0s, fun, alpha=1.0, tol=1e-4, max_iter=200, f32=False):
    """all restarts, their contrasts, the pick -> dict(runs, contrasts, best)"""
    runs = [run(Z, W0, fun, alpha, tol, max_iter, f32) for W0 in W0s]
    cons = np.array([contrast_value(moments(Z, r["W"], fun, alpha, f32)[1], fun, alpha) if r["status"] != 2 else -np.inf for r in runs])
    return dict(runs=runs, contrasts=cons, best=int(np.argmax(cons)))


def carry_back(W, sigma, n, lam):
    """Vq = D^-1 W^T, Wq = D W^T with D = diag(sigma / sqrt(n)); the explained variance sum_i lam_i w_ji^2 and its order"""
    d = np.asarray(sigma, dtype=np.float64) / np.sqrt(n)
    ev = (np.asarray(W) ** 2) @ np.asarray(lam, dtype=np.float64)
    order = np.argsort(-ev, kind="stable")
    return (W.T / d[:, None])[:, order], (W.T * d[:, None])[:, order], ev[order], order


# ---------------------------------------------------------------------------------------------------------------- the bounds
def eps_contrast(S, fun, alpha=1.0):
    """the absolute error of the device's g and g' at the projections S"""
    a = np.abs(S)
    if fun == "cube":
        return CUBE_REL * a ** 3, CUBE_REL * 3.0 * a * a
    return np.full_like(a, EPS_G[fun][0]), np.full_like(a, EPS_G[fun][1])


def moment_bound(Z, W, fun, alpha=1.0):
    """per element of W1: sum_rows (L ds + eps_g) |z_i| / n + sum_rows (L' ds + eps_g') / n |w_ji| with
    ds = (q + 1) 2^-24 sum_i |w_ji| |z_i| and L, L' the Lipschitz constants of g, g' over the interval reached"""
    Z = np.asarray(Z, dtype=np.float64)
    ok = finite_rows(Z)
    Z, W = Z[ok], np.asarray(W, dtype=np.float64)
    n, q = Z.shape
    ds = (q + 1) * U32 * (np.abs(Z) @ np.abs(W).T)                       # n x q
    S = np.abs(Z @ W.T) + ds
    if fun == "logcosh":
        L, Lp = alpha, 2.0 * alpha * alpha * 0.77                        # |g''| = 2 a^2 |tanh| sech^2 <= 0.77 a^2
        L, Lp = np.full_like(S, L), np.full_like(S, Lp)
    elif fun == "exp":
        L, Lp = np.ones_like(S), np.full_like(S, 1.4)                    # |g'| <= 1;  |g''| = |s^3 - 3 s| e <= 1.38
    else:
        L, Lp = 3.0 * S * S, 6.0 * S
    eg, egp = eps_contrast(S, fun, alpha)
    return ((L * ds + eg).T @ np.abs(Z)) / n + ((Lp * ds + egp).sum(axis=0) / n)[:, None] * np.abs(W)


def polar_bound(W1, dW1):
    """|| polar(W1 + E) - polar(W1) ||_F <= 2 ||E||_F / (sigma_min(W1) + sigma_min(W1 + E)) for |E| <= dW1 elementwise: the
    second sigma_min is taken at its lower bound sigma_min(W1) - ||E||_2"""
    e = float(np.linalg.norm(dW1))
    smin = float(np.linalg.svd(W1, compute_uv=False)[-1])
    return 2.0 * e / max(2.0 * smin - e, 1e-300)


def gmean_bound(Z, W, fun, alpha=1.0):
    """per source: the error of the mean of G -- |G'| = |g| times ds plus the error of G itself"""
    Z = np.asarray(Z, dtype=np.float64)
    Z, W = Z[finite_rows(Z)], np.asarray(W, dtype=np.float64)
    n, q = Z.shape
    ds = (q + 1) * U32 * (np.abs(Z) @ np.abs(W).T)
    S = np.abs(Z @ W.T) + ds
    g, _, G = contrast(S, fun, alpha)
    eG = CUBE_REL * np.abs(G) if fun == "cube" else EPS_G[fun][2] * (1.0 + np.abs(G))
    return (np.abs(g) * ds + eG).sum(axis=0) / n


# ------------------------------------------------------------------------------------------------------------ the test data
def random_orthogonal(q, rs):
    Q, R = np.linalg.qr(rs.standard_normal((q, q)))
    return Q * np.sign(np.diag(R))


def white(X):
    """the float32 white panel of the columns of X: centred, decorrelated by the eigenvectors of the covariance"""
    X = np.asarray(X, dtype=np.float64)
    X = X - X.mean(axis=0)
    d, E = np.linalg.eigh(X.T @ X / X.shape[0])
    return ((X @ E) / np.sqrt(d)).astype(np.float32)


def sources(n, rs, period=37.3):
    """four sources of unit variance with known non-Gaussian laws: uniform, Laplace, bimodal, a sine"""
    t = np.arange(n)
    S = np.stack([rs.uniform(-np.sqrt(3.0), np.sqrt(3.0), n), rs.laplace(0.0, 1.0 / np.sqrt(2.0), n),
                  (np.where(rs.random_sample(n) < 0.5, -1.0, 1.0) + 0.3 * rs.standard_normal(n)) / np.sqrt(1.09),
                  np.sqrt(2.0) * np.sin(2.0 * np.pi * t / period)], axis=1)
    S = S - S.mean(axis=0)
    return S / S.std(axis=0)


def mixed_panel(seed, n=1024, q=4):
    """a white float32 panel [n x q] of q mixed non-Gaussian sources (the four laws above, cycled) and an orthogonal start"""
    rs = np.random.RandomState(seed)
    S = np.concatenate([sources(n, rs, 37.3 + 11.0 * b) for b in range((q + 3) // 4)], axis=1)[:, :q]
    Z = white(S @ rs.standard_normal((q, q)))
    return Z, sym_decorrelation(rs.standard_normal((q, q)))


# the whole runs of tests/test_gpu_ica_step.py that assert an iteration count: (fun, alpha, seed, n, q, tol).
# tests/test_ica_reference_cpu.py checks their condition: lim at the deciding iteration and the one before outside [tol/2, 2 tol].
RUN_CASES = [("logcosh", 1.0, 4, 1024, 4, 1e-4), ("exp", 1.0, 6, 1500, 5, 1e-4), ("cube", 1.0, 4, 1024, 4, 1e-4),
             ("logcosh", 1.5, 6, 2049, 8, 1e-4)]


# ------------------------------------------------------------------------------------------------- the planted field of the model
PLANTED_SEED = 12              # of the field
PLANTED_START = 3              # random_state of the fit: the start (and the inner PCA's sketch)


def planted_field(seed=PLANTED_SEED, n=1024, P=96, noise=0.05):
    """X [n x P] float32 = four sources of unit variance (uniform, Laplace, bimodal, a sine) in P mixing patterns of unequal
    strength, plus small noise -> (X, the sources [n x 4])"""
    rs = np.random.RandomState(seed)
    S = sources(n, rs)
    A = rs.standard_normal((4, P)) * np.array([3.0, 2.2, 1.6, 1.2])[:, None]
    return (S @ A + noise * rs.standard_normal((n, P))).astype(np.float32), S


def pca_white(X, q):
    """numpy's float64 PCA of the centred X -> (the white float32 panel Z, sigma, V [P x q], lambda)"""
    X = np.asarray(X, dtype=np.float64)
    X = X - X.mean(axis=0)
    _, s, Vt = np.linalg.svd(X, full_matrices=False)
    V = Vt[:q].T
    Z, sigma = whiten((X @ V).astype(np.float32))
    return Z, sigma, V, s[:q] ** 2 / (X.shape[0] - 1)


def recovery(est, S):
    """min over the true sources of the largest |correlation| with an estimated one"""
    q = S.shape[1]
    C = np.abs(np.corrcoef(np.asarray(est, dtype=np.float64).T, np.asarray(S, dtype=np.float64).T)[:est.shape[1], est.shape[1]:])
    return float(C.max(axis=0).min()) if q else 1.0


def well_conditioned(run, tol, lo=0.5, hi=2.0):
    """no lim of the run inside [lo tol, hi tol]: a device that follows the run within its bounds stops at the same iteration"""
    return all(not lo * tol <= x <= hi * tol for x in run["lims"])
