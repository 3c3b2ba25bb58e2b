"""GPU tests of low-frequency component analysis (xeofs_amd.single.LFCA, engine.lowpass_cov, engine.lowpass).

The checker is a float64 numpy restatement of the model's definition (xeofs_amd/single/lfca.py) that shares no code with
it: Duchon's weights term by term, numpy.pad(mode="reflect") for the mirrored ends, numpy.polyfit for the trend, one shifted
slice per tap, numpy.linalg.eigh for both eigenproblems:

    d = S - trend,   Y = sum_k w_|k| d[refl(t + k)] + trend,   C0 = S^T S / (n - 1) = E D E^T,   K = D^-1/2 E^T,
    R = Y^T Y / (n - 1),   Tm = 1/2 (K R K^T + transpose),   (r, Uo) = leading eigenpairs (descending),   Vq = K^T Uo,
    scores = S Vq,   components = V C0 Vq,   filter patterns = V Vq.

Model tests feed it the model's own inner-PCA scores S and patterns V (float32, promoted to float64) and compare up to one
sign per mode, which must be the same sign for components, scores and filter patterns.

Tolerances are those of the OPA tests against their restatement and sufficed unchanged: 1e-9 relative on the ratios, 1e-8
of the largest entry on Vq, 2^-22 of the largest entry (one float32 rounding plus margin) on the float32 outputs.  Measured
on the two shapes of SHAPES (MI355X): ratios 6.8e-15 relative, Vq 9.4e-13, the float32 outputs at most 0.17 of their bound.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the restatement
def duchon(cutoff, h):
    fc = 1.0 / cutoff
    raw = [2.0 * fc]
    for k in range(1, h + 1):
        raw.append(np.sin(2.0 * np.pi * fc * k) / (np.pi * k) * np.sin(np.pi * k / (h + 1)) / (np.pi * k / (h + 1)))
    raw = np.array(raw)
    return raw / (raw[0] + 2.0 * raw[1:].sum())


def filtered(S, w, detrend):
    S = np.asarray(S, np.float64)
    n, p = S.shape
    h = len(w) - 1
    t = np.arange(n, dtype=np.float64)
    T = np.zeros((n, p))
    if detrend:
        for j in range(p):
            b, a = np.polyfit(t, S[:, j], 1)
            T[:, j] = a + b * t
    Dp = np.pad(S - T, ((h, h), (0, 0)), mode="reflect")
    Y = np.zeros((n, p))
    for k in range(-h, h + 1):
        Y += w[abs(k)] * Dp[h + k:h + k + n]
    return Y + T


def restate_lfca(S, V, cutoff, h, k, detrend=True):
    S, V = np.asarray(S, np.float64), np.asarray(V, np.float64)
    n = S.shape[0]
    w = duchon(cutoff, h)
    Y = filtered(S, w, detrend)
    C0 = S.T @ S / (n - 1)
    d, E = np.linalg.eigh(C0)
    K = (E / np.sqrt(d)).T
    Tm = K @ (Y.T @ Y / (n - 1)) @ K.T
    r_all, U = np.linalg.eigh(0.5 * (Tm + Tm.T))
    order = np.argsort(r_all)[::-1]
    r_all, U = r_all[order], U[:, order]
    Vq = K.T @ U[:, :k]
    return dict(r=r_all[:k], r_all=r_all, Vq=Vq, C0=C0, w=w, scores=S @ Vq, filter_patterns=V @ Vq, components=V @ (C0 @ Vq))


def trending_mixture(n, P, seed=0):
    """six AR(1) series of unit variance with phi = 0.97 ... 0.1 (drawn one after the other), random loadings, white noise of
    deviation 0.3, plus a planted trend 0.004 t g, g ~ N(0, I_P).  With an exact SVD as the inner PCA the shapes of SHAPES
    give leading ratios 0.9996, 0.810, 0.636, 0.318 (relative gaps >= 0.19) and 0.998, 0.893, 0.718, 0.481 (>= 0.10)."""
    phi = np.array([0.97, 0.9, 0.8, 0.6, 0.35, 0.1])
    rng = np.random.default_rng(seed)
    z = np.empty((n, 6))
    for j in range(6):
        e = rng.standard_normal(n)
        z[0, j] = e[0]
        for t in range(1, n):
            z[t, j] = phi[j] * z[t - 1, j] + np.sqrt(1.0 - phi[j] ** 2) * e[t]
    L = rng.standard_normal((6, P))
    X = z @ L + 0.3 * rng.standard_normal((n, P))
    g = rng.standard_normal(P)
    return (X + 0.004 * np.arange(n)[:, None] * g).astype(np.float32)


def da(X):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})


def align(model_vals, ref_vals):
    """one sign per mode: the sign of <model, ref> per column"""
    return np.sign(np.sum(np.asarray(model_vals, np.float64) * ref_vals, axis=0))


SHAPES = [(600, 300, 20, 40, 60), (500, 96, 30, 24, 33)]           # n, P, q, cutoff, h
K = 3
_cache = {}


def fitted(shape=SHAPES[0], detrend=True):
    """the fitted model of a shape, its data and its restatement, computed once and shared (nothing changes them)"""
    import xeofs_amd as xe

    key = (shape, detrend)
    if key not in _cache:
        n, P, q, cutoff, h = shape
        X = trending_mixture(n, P)
        m = xe.single.LFCA(n_modes=K, cutoff=cutoff, window=2 * h + 1, detrend=detrend, n_pca_modes=q, random_state=0)
        m.fit(da(X), dim="time")
        ref = restate_lfca(m._pca_scores, m._pca_components, cutoff, h, K, detrend)
        _cache[key] = (m, X, ref)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. model parity
def check_parity(shape, detrend):
    n, P, q, cutoff, h = shape
    m, X, ref = fitted(shape, detrend)
    assert sorted(m.data) == sorted(["input_data", "components", "scores", "norms", "filter_patterns", "low_frequency_ratio"])
    S, V = m._pca_scores, m._pca_components
    assert S.dtype == np.float32 and S.shape == (n, q) and V.dtype == np.float32 and V.shape == (P, q)
    assert np.array_equal(m.data["input_data"], S)
    r = ref["r"]
    # what the tolerances below rest on: separated leading ratios, on the model's own PCA
    gaps = (r[:-1] - r[1:]) / r[:-1]
    print(f"LFCA {n}x{P} q={q} cutoff={cutoff} h={h} detrend={detrend}: r = {r}, relative gaps = {gaps}, next = {ref['r_all'][K]}")
    assert np.all(gaps >= 0.08) and (r[-1] - ref["r_all"][K]) / r[-1] >= 0.08
    np.testing.assert_allclose(m._weights, ref["w"], rtol=1e-14, atol=1e-18)

    got = m.data["low_frequency_ratio"]
    assert got.dtype == np.float64 and got.shape == (K,)
    print(f"  ratios: max relative err = {np.abs(got / r - 1).max():.3e}")
    np.testing.assert_allclose(got, r, rtol=1e-9, atol=0)
    sgn = align(m._Vq, ref["Vq"])
    assert np.all(np.abs(sgn) == 1)
    print(f"  Vq: max err / max = {np.abs(m._Vq * sgn - ref['Vq']).max() / np.abs(ref['Vq']).max():.3e}")
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
    return sgn


@pytest.mark.parametrize("shape", SHAPES)
def test_model_matches_the_restatement(ctx, shape):
    check_parity(shape, True)


def test_detrend_false_matches_its_own_restatement(ctx):
    check_parity(SHAPES[1], False)
    a, b = fitted(SHAPES[1], True)[0], fitted(SHAPES[1], False)[0]
    # the planted trend makes the two settings different problems (so the check above can fail)
    assert np.abs(a.data["low_frequency_ratio"] - b.data["low_frequency_ratio"]).max() > 1e-6


# ------------------------------------------------------------------------------------------------ 2. invariants, accessors
def test_invariants(ctx):
    m, X, ref = fitted()
    n = X.shape[0]
    Pm = m.data["scores"].astype(np.float64)
    np.testing.assert_allclose(Pm.T @ Pm / (n - 1), np.eye(K), rtol=0, atol=1e-6)
    np.testing.assert_allclose(m.data["norms"], np.sqrt(n - 1.0), rtol=1e-6)
    r = m.data["low_frequency_ratio"]
    assert np.all(np.diff(r) < 0) and np.all(r >= 0) and np.all(r <= 1 + 1e-6)
    np.testing.assert_allclose(m._U.T @ m._U, np.eye(K), rtol=0, atol=1e-12)
    assert np.array_equal(m._R, m._R.T) and np.array_equal(m._C0, m._C0.T)         # the kernel mirrors bit for bit
    # LFC = X . fingerprint in the preprocessed space: S Vq with S = X V
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    lfc = Xc @ m.data["filter_patterns"].astype(np.float64)
    assert np.abs(lfc - Pm).max() <= 1e-4 * np.abs(Pm).max()


def test_accessors_and_stats(ctx):
    m, X, ref = fitted()
    n, P = X.shape
    C, F, Sc = m.components().values, m.filter_patterns().values, m.scores().values
    assert C.shape == (K, P) and F.shape == (K, P) and Sc.shape == (K, n)
    assert np.array_equal(C, m.data["components"].T) and np.array_equal(F, m.data["filter_patterns"].T)
    assert np.array_equal(Sc, m.data["scores"].T)
    assert np.array_equal(m.low_frequency_ratio().values, m.data["low_frequency_ratio"])
    for key in ("route", "n_pca_modes", "ms_pca", "ms_lowpass", "ms_eigen", "ms_project"):
        assert key in m.stats
    assert m.stats["n_pca_modes"] == SHAPES[0][2]
    for name in ("singular_values", "explained_variance", "explained_variance_ratio"):
        with pytest.raises(AttributeError):
            getattr(m, name)()


def test_transform_of_the_training_data_gives_the_scores(ctx):
    """the fit takes its PCA scores as the projection X V through the kernel transform uses; both are float64 sums over the
    q modes rounded once to float32, so they agree to two float32 roundings"""
    m, X, ref = fitted()
    T = m.transform(da(X)).values                                                  # (mode, time)
    Sc = m.data["scores"]
    assert T.shape == (K, X.shape[0]) and T.dtype == np.float32
    err = np.abs(T.T.astype(np.float64) - Sc)
    print(f"transform(X_train) against scores(): max err / (2^-22 max) = {err.max() / (2.0 ** -22 * np.abs(Sc).max()):.3f}")
    assert err.max() <= 2.0 ** -22 * np.abs(Sc).max()
    # new data: half of the samples
    T2 = m.transform(da(X[:250])).values
    assert np.abs(T2.T.astype(np.float64) - Sc[:250]).max() <= 2.0 ** -22 * np.abs(Sc).max()


def test_inverse_transform(ctx):
    """scores . components^T of the restatement over the K modes plus the mean the preprocessing took out.  Both factors
    carry one float32 rounding (2^-24 relative each), the product is summed in float64 and the result is rounded to the
    field's float32: 4 x 2^-24 of sum_j |s_j| |c_j| + |mean| covers it with a margin of about 2"""
    m, X, ref = fitted()
    n, P = X.shape
    sgn = align(m.data["scores"], ref["scores"])
    rec = np.asarray(m.inverse_transform(m.scores()).values, np.float64)
    assert rec.shape == (n, P)
    want = ref["scores"] @ ref["components"].T                                     # (the signs cancel)
    mean = np.asarray(m.preprocessor.mean_, np.float64).reshape(-1)
    size = np.abs(ref["scores"]) @ np.abs(ref["components"]).T + np.abs(mean)
    err = np.abs(rec - mean - want)
    print(f"inverse_transform: max err / bound = {(err / (4.0 * U24 * size)).max():.3f}")
    assert np.all(err <= 4.0 * U24 * size)
    assert np.all(np.abs(sgn) == 1)
    # one mode
    import xeofs_amd as xe

    sc = m.scores()
    one = xe.DataArray(sc.values[[1]], sc.dims, {"mode": np.asarray(sc.coords["mode"])[[1]], "time": sc.coords["time"]})
    rec1 = np.asarray(m.inverse_transform(one).values, np.float64)
    want1 = np.outer(ref["scores"][:, 1], ref["components"][:, 1])
    size1 = np.outer(np.abs(ref["scores"][:, 1]), np.abs(ref["components"][:, 1])) + np.abs(mean)
    assert np.all(np.abs(rec1 - mean - want1) <= 4.0 * U24 * size1)


def test_filtered_scores(ctx):
    """the fitted filter on the model's own float32 scores, in float64: |err| <= 2 (2 h + 4) 2^-53 Ybar as for the kernel,
    plus the restatement's polyfit against the closed-form trend (1e-12 of the scale)"""
    m, X, ref = fitted()
    h = SHAPES[0][4]
    Y = m.filtered_scores().values
    assert Y.shape == (K, X.shape[0]) and Y.dtype == np.float64
    Sc = m.data["scores"].astype(np.float64)
    want = filtered(Sc, ref["w"], True)
    scale = np.abs(Sc).max() * np.abs(ref["w"]).sum() * 2
    err = np.abs(Y.T - want).max()
    print(f"filtered_scores: max err = {err:.3e}, bound = {(2 * (2 * h + 4) * 2.0 ** -53 + 1e-12) * scale:.3e}")
    assert err <= (2 * (2 * h + 4) * 2.0 ** -53 + 1e-12) * scale
    # a low-pass: the filtered component keeps the low-frequency share of the variance
    assert np.var(Y[0]) / np.var(Sc[:, 0]) > 0.9


def test_land_mask_keeps_its_nans(ctx):
    import xeofs_amd as xe

    n, P, q, cutoff, h = SHAPES[1]
    X = trending_mixture(n, P).copy()
    land = np.zeros(P, bool)
    land[[0, 5, 6, 40, P - 1]] = True
    X[:, land] = np.nan
    m = xe.single.LFCA(n_modes=K, cutoff=cutoff, window=2 * h + 1, n_pca_modes=q, random_state=0).fit(da(X), dim="time")
    for vals in (m.components().values, m.filter_patterns().values):
        assert vals.shape == (K, P)
        assert np.all(np.isnan(vals[:, land])) and np.all(np.isfinite(vals[:, ~land]))
    assert np.all(np.isfinite(m.scores().values))
    # the same model as the sea points alone
    b = xe.single.LFCA(n_modes=K, cutoff=cutoff, window=2 * h + 1, n_pca_modes=q, random_state=0).fit(
        da(np.ascontiguousarray(X[:, ~land])), dim="time")
    np.testing.assert_allclose(m.data["low_frequency_ratio"], b.data["low_frequency_ratio"], rtol=1e-4)
    rec = m.inverse_transform(m.scores()).values
    assert np.all(np.isnan(rec[:, land])) and np.all(np.isfinite(rec[:, ~land]))


def test_default_window(ctx):
    """window=None: h = min(n - 1, ceil(1.5 cutoff))"""
    import xeofs_amd as xe

    X = trending_mixture(120, 40)
    m = xe.single.LFCA(n_modes=2, cutoff=24, n_pca_modes=8, random_state=0).fit(da(X), dim="time")
    assert m._half == 36 and m._weights.shape == (37,)
    m = xe.single.LFCA(n_modes=2, cutoff=100, n_pca_modes=8, random_state=0).fit(da(X), dim="time")
    assert m._half == 119


# ------------------------------------------------------------------------------------------------ 3. determinism, errors
def test_a_second_fit_is_bitwise_equal(ctx):
    import xeofs_amd as xe

    n, P, q, cutoff, h = SHAPES[0]
    a, X, _ = fitted()
    b = xe.single.LFCA(n_modes=K, cutoff=cutoff, window=2 * h + 1, n_pca_modes=q, random_state=0).fit(da(X), dim="time")
    for name in ("components", "scores", "filter_patterns", "low_frequency_ratio", "norms"):
        assert np.array_equal(a.data[name], b.data[name]), name


def test_errors(ctx):
    import xeofs_amd as xe

    X = trending_mixture(100, 40)
    with pytest.raises(ValueError, match="PCA modes kept"):
        xe.single.LFCA(n_modes=9, cutoff=10, n_pca_modes=0.5).fit(da(X), dim="time")
    Z = (X[:50, :6] + 1j * X[50:100, :6]).astype(np.complex64)
    with pytest.raises(TypeError, match="does not support complex data"):
        xe.single.LFCA(n_modes=2, cutoff=10, n_pca_modes=4).fit(da(Z), dim="time")
    with pytest.raises(ValueError, match="n_samples - 1"):
        xe.single.LFCA(n_modes=2, cutoff=10, window=201, n_pca_modes=4).fit(da(X), dim="time")
    # a field of rank 5 with ten PCA modes asked for: the covariance of the scores is singular
    rng = np.random.default_rng(1)
    low = (rng.standard_normal((100, 5)) @ rng.standard_normal((5, 40))).astype(np.float32)
    with pytest.raises(np.linalg.LinAlgError, match="singular"):
        xe.single.LFCA(n_modes=2, cutoff=10, n_pca_modes=10, solver="full").fit(da(low), dim="time")
