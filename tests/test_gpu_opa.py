"""GPU tests of optimal persistence analysis (csrc/eofx_lagcov.hpp, engine.lagcov, xeofs_amd.single.OPA).

The checker is a float64 numpy restatement of the reference's algorithm (xeofs/single/opa.py:128-269) written from its
equations with one explicit product per lag -- it does not use the filtered form the kernel is built on:

    C_tau = S[:n - tau]^T S[tau:] / (n - tau - 1),   M = 1/2 C_0 + C_1 + ... + C_{T-1} + 1/2 C_T,   Msum = M + M^T,
    C_0 = E D E^T,  K = D^-1/2 E^T,  Tm = 1/2 K Msum K^T,  (lam, Uo) = leading eigenpairs of Tm (descending),
    Vq = K^T Uo,  Wq = C_0 Vq,  scores = S Vq,  filter patterns = Cmp Vq,  components = Cmp Wq.

Model tests feed it the model's own inner-PCA scores S and patterns Cmp (float32, promoted to float64) and compare up to
one sign per mode, which must be the same sign for components, scores and filter patterns.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the restatement
def lagged_sum(S, w):
    """sum_tau w[tau] S[:n - tau]^T S[tau:] and the same sum of absolute values (for the rounding bound)"""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    A = np.abs(S)
    M = np.zeros((S.shape[1],) * 2)
    B = np.zeros_like(M)
    for tau in range(len(w)):
        M += w[tau] * (S[:n - tau].T @ S[tau:])
        B += abs(w[tau]) * (A[:n - tau].T @ A[tau:])
    return M, B


def restate_opa(S, Cmp, T, k):
    S, Cmp = np.asarray(S, np.float64), np.asarray(Cmp, np.float64)
    n = S.shape[0]
    C0 = S.T @ S / (n - 1)
    M = 0.5 * C0
    for tau in range(1, T + 1):
        C = S[:n - tau].T @ S[tau:] / (n - tau - 1)
        M = M + (0.5 * C if tau == T else C)
    Msum = M + M.T
    d, E = np.linalg.eigh(C0)
    K = (E / np.sqrt(d)).T
    Tm = 0.5 * K @ Msum @ K.T
    Tm = 0.5 * (Tm + Tm.T)
    lam_all, U = np.linalg.eigh(Tm)
    order = np.argsort(lam_all)[::-1]
    lam_all, U = lam_all[order], U[:, order]
    Vq = K.T @ U[:, :k]
    Wq = C0 @ Vq
    return dict(lam=lam_all[:k], lam_all=lam_all, svd_order=np.argsort(-np.abs(lam_all), kind="stable")[:k], Vq=Vq, C0=C0,
                scores=S @ Vq, filter_patterns=Cmp @ Vq, components=Cmp @ Wq)


def ar1_mixture(n, P, seed=0):
    """six AR(1) series of unit variance with phi = 0.97 ... 0.1 (drawn one after the other), random loadings, white noise
    of deviation 0.3.  With seed 0 the shapes of SHAPES give positive leading decorrelation times, relative gaps of at
    least 0.14 between consecutive wanted modes and to the next one, and the order of the reference's SVD -- asserted
    where the data are used."""
    phi = np.array([0.97, 0.9, 0.8, 0.6, 0.35, 0.1])
    rng = np.random.default_rng(seed)
    z = np.empty((n, 6))
    for j in range(6):
        e = rng.standard_normal(n)
        z[0, j] = e[0]
        for t in range(1, n):
            z[t, j] = phi[j] * z[t - 1, j] + np.sqrt(1.0 - phi[j] ** 2) * e[t]
    L = rng.standard_normal((6, P))
    return (z @ L + 0.3 * rng.standard_normal((n, P))).astype(np.float32)


def da(X):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})


# ------------------------------------------------------------------------------------------------ 1. the kernel
def panel(rng, n, p, pad):
    """float32 device panel [n x p] with row stride p + pad"""
    import torch

    host = rng.standard_normal((n, p + pad)).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    return host[:, pad // 2:pad // 2 + p], dev[:, pad // 2:pad // 2 + p]


def check_lagcov(ctx, rng, n, p, ntau, pad=0):
    from xeofs_amd import engine

    host, dev = panel(rng, n, p, pad)
    w = rng.standard_normal(ntau) * rng.choice([1e-3, 1.0, 10.0], ntau)          # mixed sign and size
    M = engine.lagcov(ctx, dev, w)
    assert M.dtype.is_floating_point and M.element_size() == 8 and tuple(M.shape) == (p, p) and M.is_cuda
    M = M.cpu().numpy()
    ref, bound = lagged_sum(host, w)
    tol = 2.0 * (n + ntau + 2) * U53 * bound
    err = np.abs(M - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"lagcov n={n} p={p} ntau={ntau} pad={pad}: max err / bound = {worst:.3f}")
    assert np.all(err <= tol), (n, p, ntau, pad, worst)
    assert np.array_equal(engine.lagcov(ctx, dev, w).cpu().numpy(), M)           # bit-reproducible


@pytest.mark.parametrize("p", [1, 15, 16, 17, 64, 100, 257])
def test_lagcov_route_edges(ctx, p):
    """n = 203 is no multiple of the 64-row tile or the 16-row window; ntau = 65 | 66 is the fused | written switch;
    ntau = n - 1 is the largest lag the entry takes"""
    rng = np.random.default_rng(100 + p)
    n = 203
    for ntau in (1, 2, 51, 65, 66, n - 1):
        check_lagcov(ctx, rng, n, p, ntau)
    check_lagcov(ctx, rng, n, p, 3, pad=7)                                       # ld > p
    check_lagcov(ctx, rng, n, p, 70, pad=5)


def test_lagcov_many_tiles_per_workgroup(ctx):
    """p = 257 runs 51 row groups; 104 row tiles make every workgroup walk two or three of them"""
    rng = np.random.default_rng(7)
    for ntau in (3, 65, 66, 201):
        check_lagcov(ctx, rng, 6605, 257, ntau, pad=3)
    check_lagcov(ctx, rng, 40000, 20, 21)                                        # 625 tiles over 512 workgroups


def test_lagcov_host_input_and_asymmetry(ctx):
    """a host panel is staged by the engine; a one-sided lag is not symmetric, so a transposed write cannot pass"""
    from xeofs_amd import engine

    rng = np.random.default_rng(3)
    S = rng.standard_normal((300, 70)).astype(np.float32)
    w = np.array([0.0, 1.0])
    M = engine.lagcov(ctx, S, w).cpu().numpy()
    ref, bound = lagged_sum(S, w)
    assert np.all(np.abs(M - ref) <= 2.0 * (300 + 2 + 2) * U53 * bound)
    assert np.abs(ref - ref.T).max() > 1.0                                       # (the check above tells M from M^T)


def test_lagcov_bad_arguments(ctx):
    import torch

    from xeofs_amd import engine

    S = torch.zeros((50, 8), dtype=torch.float32, device="cuda")
    for w in (np.ones(50), np.ones(0), np.ones((2, 2))):                         # ntau > n - 1, ntau < 1, not a vector
        with pytest.raises(ValueError):
            engine.lagcov(ctx, S, w)
    engine.lagcov(ctx, S, np.ones(49))                                           # ntau = n - 1 is the last valid one
    with pytest.raises(ValueError):
        engine.lagcov(ctx, torch.zeros((50, engine.LAGCOV_PMAX + 1), dtype=torch.float32, device="cuda"), np.ones(2))
    with pytest.raises(ValueError):
        engine.lagcov(ctx, torch.zeros(50, dtype=torch.float32, device="cuda"), np.ones(2))
    with pytest.raises(ValueError):
        engine.lagcov(ctx, torch.zeros((1, 8), dtype=torch.float32, device="cuda"), np.ones(1))


# ------------------------------------------------------------------------------------------------ 2. model parity
SHAPES = [(600, 40, 12, 20, 4), (2000, 300, 30, 50, 4), (300, 500, 10, 8, 5)]


def align(model_vals, ref_vals):
    """one sign per mode: the sign of <model, ref> per column"""
    return np.sign(np.sum(np.asarray(model_vals, np.float64) * ref_vals, axis=0))


@pytest.mark.parametrize("n,P,q,T,k", SHAPES)
def test_model_matches_the_restatement(ctx, n, P, q, T, k):
    import xeofs_amd as xe

    X = ar1_mixture(n, P)
    m = xe.single.OPA(n_modes=k, tau_max=T, n_pca_modes=q, random_state=0)
    m.fit(da(X), dim="time")
    assert sorted(m.data) == sorted(["input_data", "components", "scores", "norms", "filter_patterns", "decorrelation_time"])
    S, Cmp = m._pca_scores, m._pca_components
    assert S.dtype == np.float32 and S.shape == (n, q) and Cmp.dtype == np.float32 and Cmp.shape == (P, q)
    assert np.array_equal(m.data["input_data"], S)
    ref = restate_opa(S, Cmp, T, k)
    lam = ref["lam"]
    # what the tolerances below rest on: positive, separated leading eigenvalues, the same under the reference's |lam| order
    gaps = (lam[:-1] - lam[1:]) / lam[:-1]
    print(f"OPA {n}x{P} q={q} T={T}: lam = {lam}, relative gaps = {gaps}, next = {ref['lam_all'][k]}")
    assert np.all(lam > 0) and lam[-1] / lam[0] >= 0.07
    assert np.all(gaps >= 0.14) and (lam[-1] - ref["lam_all"][k]) / lam[-1] >= 0.14
    assert np.array_equal(ref["svd_order"], np.arange(k))

    got = m.data["decorrelation_time"]
    assert got.dtype == np.float64 and got.shape == (k,)
    np.testing.assert_allclose(got, lam, rtol=1e-9, atol=0)
    sgn = align(m._Vq, ref["Vq"])
    assert np.all(np.abs(sgn) == 1)
    assert np.abs(m._Vq * sgn - ref["Vq"]).max() <= 1e-8 * np.abs(ref["Vq"]).max()
    # the float32 outputs: one rounding plus margin, and ONE sign per mode for all three
    for name in ("components", "scores", "filter_patterns"):
        out = m.data[name]
        assert out.dtype == np.float32 and out.shape == ref[name].shape
        assert np.array_equal(align(out, ref[name]), sgn), name
        err = np.abs(out.astype(np.float64) * sgn - ref[name]).max()
        print(f"  {name}: max err = {err:.3e}, bound = {2.0 ** -22 * np.abs(ref[name]).max():.3e}")
        assert err <= 2.0 ** -22 * np.abs(ref[name]).max(), name
    # the engine's sign rule on the patterns
    C = m.data["components"]
    assert np.all(np.abs(C.max(axis=0)) >= np.abs(C.min(axis=0)))
    # accessors
    assert m.components().values.shape == (k, P) and m.filter_patterns().values.shape == (k, P)
    assert m.scores().values.shape == (k, n)
    assert np.array_equal(m.decorrelation_time().values, got)
    for key in ("route", "ms_pca", "ms_lagcov", "ms_eigen"):
        assert key in m.stats


# ------------------------------------------------------------------------------------------------ 3. invariants
def fitted(n=600, P=40, q=12, T=20, k=4, **kw):
    import xeofs_amd as xe

    X = ar1_mixture(n, P)
    return xe.single.OPA(n_modes=k, tau_max=T, n_pca_modes=q, random_state=0, **kw).fit(
        da(X), dim="time"), X


def test_invariants(ctx):
    m, X = fitted()
    n, k = 600, 4
    P = m.data["scores"].astype(np.float64)
    np.testing.assert_allclose(P.T @ P / (n - 1), np.eye(k), rtol=0, atol=1e-6)
    np.testing.assert_allclose(m.data["norms"], np.sqrt(n - 1.0), rtol=1e-6)
    assert np.all(np.diff(m.data["decorrelation_time"]) < 0)
    want = m._pca_components.astype(np.float64) @ (m._C0 @ m._Vq)
    assert np.abs(m.data["components"] - want).max() <= 2.0 ** -22 * np.abs(want).max()
    # the whitened eigenvectors kept for the orthogonality check of the reference's tests
    np.testing.assert_allclose(m._U.T @ m._U, np.eye(k), rtol=0, atol=1e-12)
    # normalised scores
    sc = m.scores(normalized=True).values.astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(sc.reshape(k, -1), axis=1), 1.0, rtol=1e-6)


def test_repeated_fits_are_bitwise_equal(ctx):
    a, _ = fitted()
    b, _ = fitted()
    for name in ("components", "scores", "filter_patterns", "decorrelation_time", "norms"):
        assert np.array_equal(a.data[name], b.data[name]), name


def test_center_false_still_centres_the_pca(ctx):
    """OPA(center=False) on a field with a large mean: the inner PCA centres (opa.py:135-147).  With every PCA mode kept
    (q = P, solver="full") the decorrelation times depend on the span of the centred field only, so the restatement fed an
    explicit float64 PCA of the explicitly centred field must agree to the accuracy of the engine's float32 PCA: its
    documented parity with float64 is 1e-5 per mode (the smoke test's bound), entering Tm once per factor over q modes:
    |d lam| <= 2 q 1e-5 lam_1."""
    import xeofs_amd as xe

    n, Pf, T, k = 400, 8, 10, 3
    X = ar1_mixture(n, Pf, seed=1) + np.float32(5.0) * np.arange(1, Pf + 1, dtype=np.float32)
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    ref = restate_opa(U * np.sqrt(n - 1.0), Vt.T * s / np.sqrt(n - 1.0), T, k)
    tol = 2 * Pf * 1e-5 * ref["lam"][0]
    for center in (False, True):
        m = xe.single.OPA(n_modes=k, tau_max=T, n_pca_modes=Pf, center=center, solver="full", random_state=0)
        m.fit(da(X), dim="time")
        got = m.data["decorrelation_time"]
        print(f"center={center}: lam = {got}, reference {ref['lam']}, tolerance {tol:.2e}")
        assert np.all(np.abs(got - ref["lam"]) <= tol), (center, got, ref["lam"])
    # without the centring the answer is a different one (so the check above can fail)
    Xr = X.astype(np.float64)
    U, s, Vt = np.linalg.svd(Xr, full_matrices=False)
    raw = restate_opa(U * np.sqrt(n - 1.0), Vt.T * s / np.sqrt(n - 1.0), T, k)
    assert np.abs(raw["lam"] - ref["lam"]).max() > 100 * tol


def test_device_field_gives_the_host_fields_result(ctx):
    import torch

    import xeofs_amd as xe

    a, X = fitted()
    b = xe.single.OPA(n_modes=4, tau_max=20, n_pca_modes=12, random_state=0).fit(
        xe.DataArray(torch.from_numpy(X).cuda(), ("time", "x"), {"time": np.arange(600), "x": np.arange(40)}), dim="time")
    np.testing.assert_allclose(b.data["decorrelation_time"], a.data["decorrelation_time"], rtol=1e-4)


# ------------------------------------------------------------------------------------------------ 4. errors
def test_errors(ctx):
    import xeofs_amd as xe

    m, X = fitted()
    with pytest.raises(NotImplementedError, match=r"OPA does not \(yet\) support transform\(\)"):
        m.transform(da(X))
    with pytest.raises(NotImplementedError, match=r"OPA does not \(yet\) support inverse_transform\(\)"):
        m.inverse_transform(m.scores())
    Z = (X[:50, :6] + 1j * X[50:100, :6]).astype(np.complex64)
    with pytest.raises(TypeError, match="does not support complex data"):
        xe.single.OPA(n_modes=2, tau_max=3, n_pca_modes=4).fit(da(Z), dim="time")
    with pytest.raises(ValueError, match="tau_max must be in"):
        xe.single.OPA(n_modes=2, tau_max=599, n_pca_modes=4).fit(da(X), dim="time")
