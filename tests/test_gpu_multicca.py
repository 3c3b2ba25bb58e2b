"""GPU tests of multi-view canonical correlation analysis (xeofs_amd.multi.CCA, engine.viewcov).

The checker is a float64 numpy / scipy restatement of the reference's algorithm (xeofs/multi/cca.py:307-384, 412-429, 480-494,
558-586) written from its equations: np.cov of the concatenated views less the np.cov of every view, scipy.linalg.eigh(C, D)
with the subset driver.  It is fed the model's own inner PCA (scores, patterns and explained variance per view, float32 and
float64, promoted to float64) and the preprocessed views the engine holds, so everything downstream of the PCA is float64 on
both sides.  The reference itself cannot run here (xarray and dask are absent), so no golden file is recorded.

Tolerances (perturbation theory, none of them found by running the code under test):
  dC        the elementwise bound of tests/test_gpu_viewcov.py on engine.viewcov, over m; dCt = D^-1/2 dC D^-1/2;
  lam       |lam - lam_ref| <= ||dCt||_F + 8 p 2^-53 ||Ct||_2                       (Weyl + the solvers' backward error);
  x         ||D^1/2 (x - x_ref)||_2 <= 2 ||dCt||_F / gap after the sign rule      (Davis-Kahan; gap: the smallest distance of
            a wanted eigenvalue to any other), so |x - x_ref|_i <= bx_i = d_i^-1/2 2 ||dCt||_F / gap;
  weights   V x rounded once to float32: 2^-24 |w| + |V| bx + (k + 2) 2^-53 |V| |x|                      (test_gpu_pcmul.py);
  variates, canonical loadings, transformed views: the projection and the X^T Z pass, 1e-5 sum_k |a_k| |b_k| per element
            (test_gpu_product_routes.py), plus the bound of the operand carried through the product.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53, U24, TOL_F32 = 2.0 ** -53, 2.0 ** -24, 1e-5
N, PS = 130, (40, 57, 23)
# the smallest distance of a wanted eigenvalue (the three largest of C x = lam D x) to any other one, over the largest one:
# computed on the CPU from the float64 restatement alone, fed an exact numpy PCA of the same data, it is 0.175 (three views,
# c = 0), 0.150 (two views), 0.036 (c = (0, 0.3, 1)) and 0.112 (pca=False).  The floors are those values less 5 %: the model's
# PCA differs from the exact one by float32 rounding (1e-7 of the scores), which moves the eigenvalues by parts in 1e6, so 5 %
# is ample room and still within a few per cent of what the tolerances were sized for.  They are asserted on the restatement
# fed the model's PCA.
REL_GAP_MIN = {"three": 0.166, "two": 0.142, "ridge": 0.034, "no pca": 0.106}
K = 3


# ------------------------------------------------------------------------------------------------ data and restatement
def make_views(seed=0, n=N, ps=PS):
    """three shared latent series seen by every view through its own noise of deviation 0.3, 0.7 and 1.2 (correlations
    between two views 0.92, 0.67, 0.41), three private series per view, random loadings, white noise of deviation 0.05;
    float32"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, 3))
    views = []
    for P in ps:
        g = f + rng.standard_normal((n, 3)) * np.array([0.3, 0.7, 1.2])
        own = rng.standard_normal((n, 3)) * 0.8
        L = rng.standard_normal((6, P))
        views.append((np.concatenate([g, own], axis=1) @ L + 0.05 * rng.standard_normal((n, P))).astype(np.float32))
    return views


def sign_rule(x):
    x = np.array(x, dtype=np.float64)
    for j in range(x.shape[1]):
        if x[int(np.argmax(np.abs(x[:, j]))), j] < 0:
            x[:, j] = -x[:, j]
    return x


def block_offdiag_cov(blocks):
    """cca.py:484-494: np.cov of the blocks side by side less the np.cov of every block"""
    Cm = np.atleast_2d(np.cov(np.concatenate(blocks, axis=1), rowvar=False))
    o = 0
    for B in blocks:
        w = B.shape[1]
        Cm[o:o + w, o:o + w] -= np.atleast_2d(np.cov(B, rowvar=False))
        o += w
    return Cm


def restate(Xs, Ss, Vs, evs, c, eps, k, pca=True):
    from scipy.linalg import eigh

    Xs = [np.asarray(X, np.float64) for X in Xs]
    Ss = [np.asarray(S, np.float64) for S in Ss]
    m = len(Ss)
    cov = block_offdiag_cov(Ss)
    C = cov / m
    p = C.shape[0]
    off = np.concatenate([[0], np.cumsum([S.shape[1] for S in Ss])])
    D = np.zeros((p, p))
    for i in range(m):
        a, b = off[i], off[i + 1]
        D[a:b, a:b] = (np.diag((1 - c[i]) * np.asarray(evs[i], np.float64) + c[i]) if pca
                       else (1 - c[i]) * np.cov(Ss[i], rowvar=False) + c[i] * np.eye(b - a))
    D = (D - (min(0, np.linalg.eigvalsh(D).min()) - eps) * np.eye(p)) / m
    lam, x = eigh(C, D, subset_by_index=[p - k, p - 1])
    lam, x = lam[::-1], sign_rule(x[:, ::-1])
    xs = [x[off[i]:off[i + 1]] for i in range(m)]
    weights = [np.asarray(V, np.float64) @ xi for V, xi in zip(Vs, xs)] if pca else xs
    loadings = [w / np.linalg.norm(w, axis=0) for w in weights]
    variates = [X @ w for X, w in zip(Xs, weights)]
    can = [X.T @ v for X, v in zip(Xs, variates)]
    T = [X @ l for X, l in zip(Xs, loadings)]
    ev = [t.var(axis=0) for t in T]
    tv = [S.var(axis=0, ddof=1).sum() for S in Ss]
    ecov = np.array([np.linalg.svd(block_offdiag_cov([t[:, i:i + 1] for t in T]), compute_uv=False)[0] for i in range(k)])
    tec = np.linalg.svd(cov, compute_uv=False)[::2][:min(S.shape[1] for S in Ss)].sum()
    lam_all = eigh(C, D, eigvals_only=True)
    return dict(C=C, D=D, cov=cov, off=off, lam=lam, x=x, xs=xs, weights=weights, loadings=loadings, variates=variates,
                canonical_loadings=can, transformed=T, explained_variance=ev, total_variance=tv, explained_covariance=ecov,
                total_explained_covariance=tec, lam_all=lam_all)


def viewcov_bound(Ss):
    """the elementwise bound of tests/test_gpu_viewcov.py on engine.viewcov of the float32 blocks side by side"""
    Z = np.concatenate([np.asarray(S, np.float32) for S in Ss], axis=1).astype(np.float64)
    n = Z.shape[0]
    Zc = np.abs(Z - Z.mean(axis=0))
    delta = n * U53 * np.abs(Z).max(axis=0)
    return ((n + 6) * U53 * (Zc.T @ Zc) + n * np.outer(delta, delta)) / (n - 1)


def da(X, name="x", t0=0):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", name), {"time": np.arange(t0, t0 + n), name: np.arange(p)})


CASES = {"three": (slice(0, 3), 0), "two": (slice(0, 2), 0), "ridge": (slice(0, 3), (0, 0.3, 1.0))}
_CACHE = {}


def fitted(case):
    """(model, raw views, restatement, facts) computed once per case and left unchanged"""
    import xeofs_amd as xe

    if case not in _CACHE:
        sl, c = CASES[case]
        raw = make_views()[sl]
        model = xe.multi.CCA(n_modes=K, c=list(c) if isinstance(c, tuple) else c, variance_fraction=0.9, random_state=0)
        model.fit([da(X, f"x{i}") for i, X in enumerate(raw)], dim="time")
        cs = list(c) if isinstance(c, tuple) else [c] * len(raw)
        Xs = [mat.download() for mat in model.data["input_data"]]
        ref = restate(Xs, model.data["pca_data"], model._pca_components, model._pca_explained_variance, cs, 1e-6, K)
        _CACHE[case] = (model, raw, ref, perturbation(model.data["pca_data"], ref, len(raw)))
    return _CACHE[case]


def perturbation(Ss, ref, m):
    """-> dict(dCt_F, lam_tol, gap, rel_gap, bx): see the header"""
    d = np.diag(ref["D"])
    assert np.array_equal(ref["D"], np.diag(d))
    dinv = 1.0 / np.sqrt(d)
    dC = viewcov_bound(Ss) / m
    dCt_F = np.linalg.norm(dC * dinv[:, None] * dinv[None, :])
    Ct = ref["C"] * dinv[:, None] * dinv[None, :]
    p = d.size
    lam_all = ref["lam_all"]
    wanted = lam_all[-K:]
    gap = min(np.abs(w - np.delete(lam_all, p - K + j)).min() for j, w in enumerate(wanted))
    return dict(dCt_F=dCt_F, lam_tol=dCt_F + 8 * p * U53 * np.linalg.norm(Ct, 2), gap=gap, rel_gap=gap / lam_all[-1],
                bx=dinv * 2.0 * dCt_F / gap, d=d, p=p)


def report(what, err, bound):
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"  {what}: max err / bound = {worst:.3g}")
    return bool(np.all(err <= bound)), worst


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", list(CASES))
def test_model_matches_the_restatement(ctx, case):
    model, raw, ref, pt = fitted(case)
    m, n = len(raw), N
    data = model.data
    Xs = [mat.download().astype(np.float64) for mat in data["input_data"]]
    widths = [S.shape[1] for S in data["pca_data"]]
    print(f"CCA {case}: PCA modes {widths}, eigenvalues {ref['lam']}, relative gap {pt['rel_gap']:.3f}, "
          f"||dCt||_F = {pt['dCt_F']:.3g}, route {model.stats['eig_route']}")
    assert pt["rel_gap"] >= REL_GAP_MIN[case]                                            # what the tolerances rest on
    assert all(2 <= w <= P for w, P in zip(widths, PS)) and model.stats["n_pca_modes"] == widths
    for S, V, X in zip(data["pca_data"], model._pca_components, Xs):
        assert S.dtype == np.float32 and V.dtype == np.float32 and S.shape[0] == n
    # eigenvalues and PC-space weights
    ok, _ = report("eigenvalues", np.abs(model.eigvals - ref["lam"]), np.full(K, pt["lam_tol"]))
    assert ok
    assert np.all(np.diff(model.eigvals) < 0)
    dy = np.sqrt(pt["d"])[:, None] * (model.eigvecs - ref["x"])
    ok, _ = report("eigenvectors (D^1/2 x, 2-norm per mode)", np.linalg.norm(dy, axis=0), np.full(K, 2.0 * pt["dCt_F"] / pt["gap"]))
    assert ok
    np.testing.assert_allclose(model.eigvecs.T @ (pt["d"][:, None] * model.eigvecs), np.eye(K), atol=1e-12)
    top = np.argmax(np.abs(model.eigvecs), axis=0)
    assert np.all(model.eigvecs[top, np.arange(K)] > 0)                            # the sign rule
    off = ref["off"]
    bws = []
    for i in range(m):
        V = model._pca_components[i].astype(np.float64)
        bx = np.repeat(pt["bx"][off[i]:off[i + 1], None], K, axis=1)
        w, wr = data["weights"][i], ref["weights"][i]
        assert w.dtype == np.float32 and w.shape == (PS[i], K)
        bw = U24 * np.abs(wr) + np.abs(V) @ bx + (V.shape[1] + 2) * U53 * (np.abs(V) @ np.abs(ref["xs"][i]))
        ok, _ = report(f"view {i} weights", np.abs(w - wr), bw)
        assert ok
        bws.append(bw)
    bvs = check_downstream(data, ref, Xs, bws, data["pca_data"], pt["p"])
    for i in range(m):
        # a property: the variates have the variance x_i^T cov(S_i) x_i
        S = data["pca_data"][i].astype(np.float64)
        want = np.einsum("ak,ab,bk->k", ref["xs"][i], np.cov(S, rowvar=False), ref["xs"][i])
        v = data["variates"][i].astype(np.float64)
        vc = np.abs(ref["variates"][i] - ref["variates"][i].mean(axis=0))
        bvc = bvs[i] + bvs[i].mean(axis=0)
        slack = ((2 * vc * bvc + bvc ** 2).sum(axis=0) / (n - 1)
                 + 2 * TOL_F32 * want)      # S = X V was itself rounded to float32 and projected: the first-order share
        ok, _ = report(f"view {i} variance of the variates against x^T cov(S) x", np.abs(v.var(axis=0, ddof=1) - want), slack)
        assert ok


def check_downstream(data, ref, Xs, bws, Ss, p):
    """everything the fit derives from the feature-space weights, against the restatement, given the elementwise bounds `bws`
    on the weights: loadings, variates, canonical loadings, explained variance and its ratio, total variance, explained
    covariance per mode, total explained covariance and the ratio.  `Ss`: the blocks whose block cross-covariance the model
    took (PCA scores, or the views themselves).  -> the bounds on the variates"""
    m, n = len(Xs), Xs[0].shape[0]
    bvs, bts = [], []
    for i in range(m):
        X, wr, lr = Xs[i], ref["weights"][i], ref["loadings"][i]
        bw = bws[i]
        nw = np.linalg.norm(wr, axis=0)
        bl = U24 * np.abs(lr) + bw / nw + np.abs(lr) * np.linalg.norm(bw, axis=0) / nw
        ok, _ = report(f"view {i} loadings", np.abs(data["loadings"][i] - lr), bl)
        assert ok
        bv = TOL_F32 * (np.abs(X) @ np.abs(wr)) + np.abs(X) @ bw
        ok, _ = report(f"view {i} variates", np.abs(data["variates"][i] - ref["variates"][i]), bv)
        assert ok
        bc = TOL_F32 * (np.abs(X).T @ np.abs(ref["variates"][i])) + np.abs(X).T @ bv
        ok, _ = report(f"view {i} canonical loadings", np.abs(data["canonical_loadings"][i] - ref["canonical_loadings"][i]), bc)
        assert ok
        # explained variance (ddof = 0) of X loadings: d var <= mean(2 |Tc| bt' + bt'^2), bt' = bt + mean(bt)
        bt = TOL_F32 * (np.abs(X) @ np.abs(lr)) + np.abs(X) @ bl
        btc = bt + bt.mean(axis=0)
        Tc = np.abs(ref["transformed"][i] - ref["transformed"][i].mean(axis=0))
        bev = (2 * Tc * btc + btc ** 2).mean(axis=0)
        ok, _ = report(f"view {i} explained variance", np.abs(data["explained_variance"][i] - ref["explained_variance"][i]), bev)
        assert ok
        np.testing.assert_allclose(data["total_variance"][i], ref["total_variance"][i], rtol=1e-12)
        brat = bev / ref["total_variance"][i] + 2e-12 * ref["explained_variance"][i] / ref["total_variance"][i]
        assert np.all(np.abs(data["explained_variance_ratio"][i] - ref["explained_variance"][i] / ref["total_variance"][i]) <= brat)
        bt32 = bt + U24 * np.abs(ref["transformed"][i])      # the transformed views enter viewcov as float32
        bvs.append(bv)
        bts.append(bt32 + bt32.mean(axis=0))
    # explained covariance per mode: |d sigma_max| <= ||dM||_F of the m x m off-diagonal covariance of the transformed views
    becov = np.empty(K)
    for j in range(K):
        dM = np.zeros((m, m))
        for u in range(m):
            for v in range(m):
                if u != v:
                    Tu = np.abs(ref["transformed"][u][:, j] - ref["transformed"][u][:, j].mean())
                    Tv = np.abs(ref["transformed"][v][:, j] - ref["transformed"][v][:, j].mean())
                    dM[u, v] = (Tu * bts[v][:, j] + bts[u][:, j] * Tv + bts[u][:, j] * bts[v][:, j]).sum() / (n - 1)
        becov[j] = np.linalg.norm(dM) + 8 * m * U53 * ref["explained_covariance"][j]
    ok, _ = report("explained covariance", np.abs(data["explained_covariance"] - ref["explained_covariance"]), becov)
    assert ok
    # total explained covariance: min k singular values, each within ||d cov||_F + the solvers' backward error
    kmin = min(S.shape[1] for S in Ss)
    btec = kmin * (np.linalg.norm(viewcov_bound(Ss)) + 8 * p * U53 * np.linalg.norm(ref["cov"], 2))
    ok, _ = report("total explained covariance", np.abs(data["total_explained_covariance"] - ref["total_explained_covariance"]),
                   np.array(btec))
    assert ok
    rat = ref["explained_covariance"] / ref["total_explained_covariance"]
    assert np.all(np.abs(data["explained_covariance_ratio"] - rat)
                  <= becov / ref["total_explained_covariance"] + rat * btec / ref["total_explained_covariance"] + 1e-15)
    return bvs


def test_two_views_without_ridge_give_the_canonical_correlation(ctx):
    """with two views and c = 0 the leading eigenvalue is the first canonical correlation: the largest singular value of
    U_1^T U_2, U_i an orthonormal basis of the centred PCA scores of view i (Bjorck & Golub 1973), in float64.  The model
    shifts D by eps = 1e-6, which moves lam by at most eps lam / min d."""
    model, raw, ref, pt = fitted("two")
    Us = []
    for S in model.data["pca_data"]:
        S = S.astype(np.float64)
        Us.append(np.linalg.svd(S - S.mean(axis=0), full_matrices=False)[0])
    rho = np.linalg.svd(Us[0].T @ Us[1], compute_uv=False)[0]
    S64 = [S.astype(np.float64) for S in model.data["pca_data"]]
    d_true = np.concatenate([S.var(axis=0, ddof=1) for S in S64])
    d_used = np.concatenate(model._pca_explained_variance)
    # lam = max x^T C x / x^T D x: replacing D by another positive diagonal moves it by at most max |d_used / d_true - 1| lam,
    # and the scores' own small cross-correlations (cov(S_i) is diagonal only up to the PCA's accuracy) by ||R - I||_2 lam
    R = [np.corrcoef(S, rowvar=False) for S in S64]
    slack = rho * (np.abs((d_used + 1e-6) / d_true - 1).max() + max(np.linalg.norm(r - np.eye(r.shape[0]), 2) for r in R)) + pt["lam_tol"]
    print(f"first canonical correlation {rho:.12f}, leading eigenvalue {model.eigvals[0]:.12f}, slack {slack:.3g}")
    assert abs(model.eigvals[0] - rho) <= slack
    assert slack < 1e-3 * rho                                                      # (the comparison says something)


@pytest.mark.parametrize("case", ["three"])
def test_components_are_correlations(ctx, case):
    model, raw, ref, pt = fitted(case)
    for i, comp in enumerate(model.components(normalize=True)):
        v = comp.values
        assert v.shape == (K, PS[i]) and np.all(np.abs(v) <= 1.0) and not np.isnan(v).any()
    for i, comp in enumerate(model.components(normalize=False)):
        assert np.array_equal(comp.values, model.data["canonical_loadings"][i].T.astype(np.float64))


@pytest.mark.parametrize("case", ["three"])
def test_transform_of_the_training_views_gives_the_scores(ctx, case):
    model, raw, ref, pt = fitted(case)
    T = model.transform([da(X, f"x{i}") for i, X in enumerate(raw)])
    sc = model.scores()
    assert len(T) == len(sc) == 3                                                  # one entry per view
    for i in range(3):
        X = model.data["input_data"][i].download().astype(np.float64)
        bound = 2 * TOL_F32 * (np.abs(X) @ np.abs(model.data["weights"][i].astype(np.float64)))      # two runs of the route
        ok, _ = report(f"view {i} transform against scores", np.abs(T[i].values.T - sc[i].values.T), bound)
        assert ok and T[i].dims == ("mode", "time") and T[i].values.shape == (K, N)


def test_a_second_fit_is_bitwise_equal(ctx):
    import xeofs_amd as xe

    a, raw, _, _ = fitted("three")
    b = xe.multi.CCA(n_modes=K, variance_fraction=0.9, random_state=0).fit([da(X, f"x{i}") for i, X in enumerate(raw)], dim="time")
    assert np.array_equal(a.eigvals, b.eigvals) and np.array_equal(a.eigvecs, b.eigvecs)
    for name in ("weights", "loadings", "variates", "canonical_loadings", "explained_variance", "explained_variance_ratio"):
        for u, v in zip(a.data[name], b.data[name]):
            assert np.array_equal(u, v), name
    for name in ("explained_covariance", "explained_covariance_ratio", "total_explained_covariance", "total_variance"):
        assert np.array_equal(a.data[name], b.data[name]), name


# ------------------------------------------------------------------------------------------------ 2. pca=False
def test_without_pca_matches_its_restatement(ctx):
    """pca=False on the small case: D's blocks are dense (viewcov with keep_diag), the pencil is solved by LAPACK's generalised
    driver on both sides.  With dC and dD the viewcov bounds and D = L L^T, the standard form L^-1 C L^-T moves by at most
    pert = (||dC||_F + |lam| ||dD||_F) / lam_min(D) to first order (Stewart & Sun 1990, VI.3), and the driver's own error
    is solver = 8 p 2^-53 ||C||_2 / lam_min(D) in an eigenvalue and sqrt(cond(D)) times that in an eigenvector (LAPACK Users'
    Guide 4.10, error bounds of the generalised symmetric definite problem).  So |d lam| <= pert + solver; in y = L^T x
    Davis-Kahan gives ||dy|| <= 2 (pert + sqrt(cond(D)) solver) / gap, and x = L^-T y carries it with lam_min(D)^-1/2 plus
    the change of L itself, ||x|| ||dD||_F / lam_min(D)."""
    import xeofs_amd as xe

    raw = make_views()
    c = [0.0, 0.3, 1.0]
    model = xe.multi.CCA(n_modes=K, c=c, pca=False).fit([da(X, f"x{i}") for i, X in enumerate(raw)], dim="time")
    Xs = [mat.download() for mat in model.data["input_data"]]
    ref = restate(Xs, Xs, None, None, c, 1e-6, K, pca=False)
    m, p = 3, sum(PS)
    full = viewcov_bound(Xs)
    dC_F = np.linalg.norm(full) / m
    dD_F = np.linalg.norm(full) / m                                                # (1 - c) <= 1 times the same bound
    evD = np.linalg.eigvalsh(ref["D"])
    lam_all = ref["lam_all"]
    gap = min(np.abs(w - np.delete(lam_all, p - K + j)).min() for j, w in enumerate(lam_all[-K:]))
    pert = (dC_F + np.abs(ref["lam"]).max() * dD_F) / evD[0]
    solver = 8 * p * U53 * np.linalg.norm(ref["C"], 2) / evD[0]
    tol = pert + solver
    print(f"CCA pca=False: eigenvalues {ref['lam']}, relative gap {gap / lam_all[-1]:.3f}, lam_min(D) {evD[0]:.3g}, "
          f"cond(D) {evD[-1] / evD[0]:.3g}, eigenvalue tolerance {tol:.3g}")
    assert gap / lam_all[-1] >= REL_GAP_MIN["no pca"] and model.stats["eig_route"] == "host" and model.stats["n_pca_modes"] is None
    ok, _ = report("eigenvalues", np.abs(model.eigvals - ref["lam"]), np.full(K, tol))
    assert ok
    bx = (2 * (pert + np.sqrt(evD[-1] / evD[0]) * solver) / gap / np.sqrt(evD[0])
          + np.linalg.norm(ref["x"], axis=0) * dD_F / evD[0])
    ok, _ = report("eigenvectors (2-norm per mode)", np.linalg.norm(model.eigvecs - ref["x"], axis=0), bx)
    assert ok
    bws = []
    for i in range(m):
        w, wr = model.data["weights"][i], ref["weights"][i]
        bw = U24 * np.abs(wr) + bx[None, :]
        assert w.dtype == np.float32 and w.shape == (PS[i], K)
        ok, _ = report(f"view {i} weights", np.abs(w - wr), bw)
        assert ok
        bws.append(bw)
    check_downstream(model.data, ref, [X.astype(np.float64) for X in Xs], bws, Xs, p)


def test_without_pca_beyond_the_limit(ctx):
    import xeofs_amd as xe

    rng = np.random.default_rng(3)
    views = [da(rng.standard_normal((20, 2100)).astype(np.float32), f"x{i}") for i in range(2)]
    with pytest.raises(NotImplementedError, match="pca=True"):
        xe.multi.CCA(pca=False).fit(views, dim="time")


# ------------------------------------------------------------------------------------------------ 3. errors, accessors
def test_errors(ctx):
    import xeofs_amd as xe

    raw = make_views()
    good = [da(X, f"x{i}") for i, X in enumerate(raw)]
    with pytest.raises(ValueError, match="All views must have the same number of samples"):
        xe.multi.CCA().fit([good[0], da(raw[1][:100], "x1")], dim="time")
    with pytest.raises(ValueError, match="All views must have at least 5 features"):
        xe.multi.CCA(n_modes=5).fit([good[0], da(raw[1][:, :4], "x1")], dim="time")
    Zc = (raw[0][:65] + 1j * raw[0][65:]).astype(np.complex64)
    with pytest.raises(TypeError, match="does not support complex data"):
        xe.multi.CCA().fit([da(Zc, "x0"), da(raw[1][:65], "x1")], dim="time")
    with pytest.raises(ValueError, match="number of views passed should match number of parameter c"):
        xe.multi.CCA(c=[0.1, 0.2]).fit(good, dim="time")
    with pytest.raises(ValueError, match="number of views passed should match number of parameter init_pca_modes"):
        xe.multi.CCA(init_pca_modes=[0.5]).fit(good, dim="time")
    with pytest.raises(ValueError, match="init_pca_modes must be either"):
        xe.multi.CCA(init_pca_modes=1.5).fit(good, dim="time")


def test_accessors(ctx):
    model, raw, ref, pt = fitted("three")
    modes = np.arange(1, K + 1)
    W, Cn, Sc = model.weights(), model.components(), model.scores()
    EV, EVR = model.explained_variance(), model.explained_variance_ratio()
    assert all(isinstance(v, list) and len(v) == 3 for v in (W, Cn, Sc, EV, EVR))
    for i in range(3):
        assert W[i].dims == ("mode", f"x{i}") and W[i].values.shape == (K, PS[i]) and W[i].name == "weights"
        assert np.array_equal(W[i].values, model.data["weights"][i].T)
        assert np.array_equal(W[i].coords["mode"], modes) and np.array_equal(W[i].coords[f"x{i}"], np.arange(PS[i]))
        assert Cn[i].dims == ("mode", f"x{i}") and Cn[i].values.shape == (K, PS[i])
        assert Sc[i].dims == ("mode", "time") and np.array_equal(Sc[i].values, model.data["variates"][i].T)
        assert np.array_equal(Sc[i].coords["time"], np.arange(N)) and np.array_equal(Sc[i].coords["mode"], modes)
        assert EV[i].dims == ("mode",) and np.array_equal(EV[i].values, model.data["explained_variance"][i])
        assert np.array_equal(EVR[i].values, model.data["explained_variance_ratio"][i])
    ec, ecr = model.explained_covariance(), model.explained_covariance_ratio()
    assert ec.dims == ("mode",) and np.array_equal(ec.coords["mode"], modes)
    assert np.array_equal(ec.values, model.data["explained_covariance"])
    assert np.array_equal(ecr.values, model.data["explained_covariance_ratio"])
    for key in ("eig_route", "n_pca_modes", "p", "ms_pca", "ms_viewcov", "ms_eigen", "ms_project"):
        assert key in model.stats
    assert model.stats["eig_route"] == "host"


def test_the_device_eigensolver_agrees_with_the_host_one(ctx):
    """beyond CCA_HOST_EIG_PMAX columns the whitened problem is solved by torch.linalg.eigh on the device: the same pairs as
    the host's subset driver, on a case small enough for both (the threshold is lowered for this one fit)"""
    import xeofs_amd as xe
    from xeofs_amd.multi import cca

    a, raw, ref, pt = fitted("three")
    old = cca.CCA_HOST_EIG_PMAX
    cca.CCA_HOST_EIG_PMAX = 4
    try:
        b = xe.multi.CCA(n_modes=K, variance_fraction=0.9, random_state=0).fit([da(X, f"x{i}") for i, X in enumerate(raw)], dim="time")
    finally:
        cca.CCA_HOST_EIG_PMAX = old
    assert b.stats["eig_route"] == "device" and a.stats["eig_route"] == "host"
    assert np.all(np.abs(b.eigvals - ref["lam"]) <= pt["lam_tol"])
    dy = np.sqrt(pt["d"])[:, None] * (b.eigvecs - ref["x"])
    assert np.all(np.linalg.norm(dy, axis=0) <= 2.0 * pt["dCt_F"] / pt["gap"])
    assert abs(b.data["total_explained_covariance"] - ref["total_explained_covariance"]) <= \
        min(S.shape[1] for S in b.data["pca_data"]) * (np.linalg.norm(viewcov_bound(b.data["pca_data"]))
                                                       + 8 * pt["p"] * U53 * np.linalg.norm(ref["cov"], 2))
