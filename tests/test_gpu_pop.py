"""GPU tests of principal oscillation pattern analysis (xeofs_amd.single.POP, engine.pcmul, engine.lagcov).

The checker is a float64 numpy restatement of the reference's algorithm (xeofs/single/pop.py:159-253) written from its
equations, with the per-mode loop and numpy's pinv:

    C0 = S[:-1]^T S[:-1],  C1 = S[1:]^T S[:-1],  A = C1 C0^-1,  A p = lam p,
    [Re z; Im z] = pinv([[pr.pr, pr.pi], [pr.pi, pi.pi]]) [S pr, S pi]^T,  norms = sqrt(var z),  components = V p.

It is fed the model's own inner-PCA scores S and patterns V (float32, promoted to float64).  An eigenvector is defined up to a
complex scalar c: p -> c p turns z into z / conj(c), so modes are compared through the scalar-free rank-two matrix
Re(z) Re(p)^T + Im(z) Im(p)^T in feature space (the projection of the samples onto the mode's plane).  The model's z is float64 and its p float32; the bound of the issue,
4 * 2^-24 (|Re z| |Re p|^T + |Im z| |Im p|^T) elementwise, covers two float32-rounded factors (2 * 2^-24) with a factor 2 for
the float64 accumulation and the eigenproblem's perturbation, which are orders smaller.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SHAPES = [(203, 300, 0), (600, 1000, 1), (130, 257, 1)]          # (n, P, seed); (130, 257, 0) has cond(C0) = 8.53, above the 8.5 asserted


# ------------------------------------------------------------------------------------------------ data and restatement
def oscillators(n, P, seed=0):
    """three damped rotating pairs x_t = r R(theta) x_{t-1} + sqrt(1 - r^2) eps and two AR(1) series, drawn one after the
    other; column amplitudes, random normal loadings to P features, white noise of deviation 0.3; float32"""
    rng = np.random.default_rng(seed)
    cols = []
    for r, period in [(0.95, 12.0), (0.85, 5.0), (0.7, 3.3)]:
        th = 2.0 * np.pi / period
        R = r * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        e = rng.standard_normal((n, 2))
        x = np.empty((n, 2))
        x[0] = e[0]
        for t in range(1, n):
            x[t] = R @ x[t - 1] + np.sqrt(1.0 - r * r) * e[t]
        cols.append(x)
    for phi in (0.9, 0.4):
        e = rng.standard_normal(n)
        x = np.empty(n)
        x[0] = e[0]
        for t in range(1, n):
            x[t] = phi * x[t - 1] + np.sqrt(1.0 - phi * phi) * e[t]
        cols.append(x[:, None])
    z = np.concatenate(cols, axis=1) * np.array([3.0, 3.0, 2.5, 2.5, 2.0, 2.0, 1.5, 1.2])
    L = rng.standard_normal((8, P))
    return (z @ L + 0.3 * rng.standard_normal((n, P))).astype(np.float32)


def restate_pop(S, V):
    S, V = np.asarray(S, np.float64), np.asarray(V, np.float64)
    C0 = S[:-1].T @ S[:-1]
    C1 = S[1:].T @ S[:-1]
    A = C1 @ np.linalg.inv(C0)
    lam, Pq = np.linalg.eig(A)
    Z = np.empty((S.shape[0], Pq.shape[1]), dtype=complex)
    for i in range(Pq.shape[1]):
        pr, pi = Pq[:, i:i + 1].real, Pq[:, i:i + 1].imag
        G = np.array([[pr.T @ pr, pr.T @ pi], [pr.T @ pi, pi.T @ pi]]).squeeze()
        zri = np.linalg.pinv(G) @ np.hstack([S @ pr, S @ pi]).T
        Z[:, i] = zri[0] + 1j * zri[1]
    with np.errstate(divide="ignore"):
        periods = 2.0 * np.pi / np.angle(lam)
    return dict(lam=lam, Pq=Pq, Z=Z, tau=-1.0 / np.log(np.abs(lam)), periods=periods, norms=np.sqrt(Z.var(axis=0)),
                components=V @ Pq, C0=C0, total_variance=(S * S).sum() / (S.shape[0] - 1))


def rank_two(z, p):
    z, p = np.asarray(z, np.complex128), np.asarray(p, np.complex128)
    return np.outer(z.real, p.real) + np.outer(z.imag, p.imag)


def rank_two_bound(z, p):
    return 4.0 * U24 * (np.outer(np.abs(z.real), np.abs(p.real)) + np.outer(np.abs(z.imag), np.abs(p.imag)))


def da(X, t0=0):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", "x"), {"time": np.arange(t0, t0 + n), "x": np.arange(p)})


_CACHE = {}


def fitted(n, P, seed):
    """(model, X, restatement, match) computed once per shape and left unchanged; match[j] = the restatement's mode
    nearest in eigenvalue to the model's mode j"""
    import xeofs_amd as xe

    key = (n, P, seed)
    if key not in _CACHE:
        X = oscillators(n, P, seed)
        m = xe.single.POP(n_pca_modes=8, random_state=0).fit(da(X), dim="time")
        ref = restate_pop(m._pca_scores, m._pca_components)
        match = np.argmin(np.abs(m.data["eigenvalues"][:, None] - ref["lam"][None, :]), axis=1)
        _CACHE[key] = (m, X, ref, match)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("n,P,seed", SHAPES)
def test_model_matches_the_restatement(ctx, n, P, seed):
    m, X, ref, match = fitted(n, P, seed)
    q = 8
    assert sorted(m.data) == sorted(["input_data", "components", "scores", "norms", "eigenvalues", "damping_times",
                                     "periods", "total_variance"])
    S, V = m._pca_scores, m._pca_components
    assert S.dtype == np.float32 and S.shape == (n, q) and V.dtype == np.float32 and V.shape == (P, q)
    assert np.array_equal(m.data["input_data"], S)
    # what the tolerances rest on (the conditions of the issue, asserted on the data used)
    lam = ref["lam"]
    gap = min(abs(lam[i] - lam[j]) for i in range(q) for j in range(i))
    sv = np.linalg.svd(X.astype(np.float64) - X.astype(np.float64).mean(axis=0), compute_uv=False)
    facts = dict(gap=gap, n_real=int((lam.imag == 0).sum()), cond_C0=np.linalg.cond(ref["C0"]),
                 cond_Pq=np.linalg.cond(ref["Pq"]), sv_ratio=sv[7] / sv[8])
    print(f"POP {n}x{P} seed {seed}: {facts}")
    assert gap >= 0.34 and facts["n_real"] == 2 and facts["cond_C0"] <= 8.5 and facts["cond_Pq"] <= 1.7
    assert facts["sv_ratio"] >= 24.0
    assert sorted(match) == list(range(q))                                         # the match is one to one

    got = m.data["eigenvalues"]
    assert got.dtype == np.complex128 and got.shape == (q,)
    assert np.abs(got - lam[match]).max() <= 1e-10 * np.abs(lam).max()
    np.testing.assert_allclose(got.real, lam[match].real, rtol=1e-10, atol=1e-10 * np.abs(lam).max())
    np.testing.assert_allclose(got.imag, lam[match].imag, rtol=1e-10, atol=1e-10 * np.abs(lam).max())
    np.testing.assert_allclose(m.data["periods"], ref["periods"][match], rtol=1e-10)
    np.testing.assert_allclose(m.data["damping_times"], ref["tau"][match], rtol=1e-10)
    np.testing.assert_allclose(m.data["total_variance"], ref["total_variance"], rtol=1e-10)
    # norms: |z| scales with 1 / |c|; the model's eigenvectors and LAPACK's both have unit 2-norm
    np.testing.assert_allclose(np.linalg.norm(ref["Pq"], axis=0), 1.0, rtol=1e-12)
    np.testing.assert_allclose(m.data["norms"], ref["norms"][match], rtol=1e-10)
    # scores x components, scalar-free, per mode
    Zm, Cm = m.data["scores"], m.data["components"]
    assert Zm.dtype == np.complex128 and Zm.shape == (n, q) and Cm.dtype == np.complex64 and Cm.shape == (P, q)
    worst = 0.0
    for j in range(q):
        want = rank_two(ref["Z"][:, match[j]], ref["components"][:, match[j]])
        bound = rank_two_bound(Zm[:, j], Cm[:, j])          # (in the model's phase: that is where its factors are rounded)
        err = np.abs(rank_two(Zm[:, j], Cm[:, j]) - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (j, worst)
    print(f"  rank-two matrices: max err / bound = {worst:.3f}")


@pytest.mark.parametrize("n,P,seed", SHAPES[:1])
def test_normalization_order_and_conjugates(ctx, n, P, seed):
    m, X, ref, match = fitted(n, P, seed)
    q = 8
    Pq, lam, norms = m._Pq, m.data["eigenvalues"], m.data["norms"]
    np.testing.assert_allclose(np.linalg.norm(Pq, axis=0), 1.0, rtol=1e-14)
    top = np.argmax(np.abs(Pq), axis=0)
    piv = Pq[top, np.arange(q)]
    assert np.all(piv.imag == 0.0) and np.all(piv.real > 0.0)
    assert np.all(np.diff(norms) <= 0.0)
    j, pairs = 0, 0
    while j < q:
        if lam[j].imag == 0.0:
            assert np.all(m.data["scores"][:, j].imag == 0.0) and np.all(m.data["components"][:, j].imag == 0.0)
            assert m.data["periods"][j] in (np.inf, 2.0)
            j += 1
            continue
        # a pair: Im lam > 0 first, equal norms, exact conjugates on every output
        assert lam[j].imag > 0.0 and lam[j + 1] == np.conj(lam[j]) and norms[j] == norms[j + 1]
        assert np.array_equal(Pq[:, j + 1], np.conj(Pq[:, j]))
        assert np.array_equal(m.data["scores"][:, j + 1], np.conj(m.data["scores"][:, j]))
        assert np.array_equal(m.data["components"][:, j + 1], np.conj(m.data["components"][:, j]))
        assert m.data["periods"][j + 1] == -m.data["periods"][j]
        pairs += 1
        j += 2
    assert pairs == 3
    # the components are V Pq rounded once
    want = m._pca_components.astype(np.float64) @ Pq
    got = m.data["components"].astype(np.complex128)
    assert np.all(np.abs(got.real - want.real) <= U24 * np.abs(want.real) + 1e-300)
    assert np.all(np.abs(got.imag - want.imag) <= U24 * np.abs(want.imag) + 1e-300)


# ------------------------------------------------------------------------------------------------ 2. transform / inverse
@pytest.mark.parametrize("n,P,seed", SHAPES[:1])
def test_transform_of_the_training_data_gives_the_scores(ctx, n, P, seed):
    """the fit takes its PCA scores as the projection X V through the kernel transform uses, so the training data come
    back as the scores; the bound is the one of the parity test"""
    m, X, ref, match = fitted(n, P, seed)
    T = m.transform(da(X)).values                                                  # (mode, time)
    assert T.shape == (8, n) and np.iscomplexobj(T)
    Zm, Cm = m.data["scores"], m.data["components"]
    worst = 0.0
    ok = True
    for j in range(8):
        err = np.abs(rank_two(T[j], Cm[:, j]) - rank_two(Zm[:, j], Cm[:, j]))
        bound = rank_two_bound(Zm[:, j], Cm[:, j])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        ok = ok and bool(np.all(err <= bound))
    print(f"transform(X_train) against scores(): max err / bound = {worst:.3f}")
    assert ok, worst


@pytest.mark.parametrize("n,P,seed", SHAPES[:1])
def test_inverse_transform(ctx, n, P, seed):
    m, X, ref, match = fitted(n, P, seed)
    q = 8
    sc = m.scores()
    rec = m.inverse_transform(sc).values                                           # (time, x) complex
    assert rec.shape == (n, P) and np.iscomplexobj(rec)
    # all modes: sum_j z_j p_j^T of the restatement (the reference's `Z @ P.T`), plus the mean the preprocessing took out
    want = sum(np.outer(ref["Z"][:, j], ref["components"][:, j]) for j in range(q))
    bound = sum(rank_two_bound(ref["Z"][:, j], ref["components"][:, j]) for j in range(q))
    mean = m.preprocessor.mean_
    err_re = np.abs(rec.real - mean - want.real)
    err_im = np.abs(rec.imag - want.imag)
    bound_im = sum(4.0 * U24 * (np.outer(np.abs(ref["Z"][:, j].imag), np.abs(ref["components"][:, j].real))
                                + np.outer(np.abs(ref["Z"][:, j].real), np.abs(ref["components"][:, j].imag))) for j in range(q))
    slack = 2.0 ** -52 * np.abs(mean)                                              # the mean is added in float64
    print(f"inverse_transform, all modes: max err / bound = {(err_re / np.maximum(bound + slack, 1e-300)).max():.3f} (Re), "
          f"{(err_im / np.maximum(bound_im, 1e-300)).max():.3f} (Im)")
    assert np.all(err_re <= bound + slack) and np.all(err_im <= bound_im)
    # one conjugate pair: z p^T + conj(z p^T) is real
    lam = m.data["eigenvalues"]
    j = int(np.flatnonzero(lam.imag > 0)[0])
    pair = m.inverse_transform(_modes(sc, [j, j + 1])).values
    size = 2.0 * (np.outer(np.abs(m.data["scores"][:, j]), np.abs(m.data["components"][:, j])))
    print(f"inverse_transform, pair {j + 1},{j + 2}: max |Im| / (2^-24 |z||p|) = {(np.abs(pair.imag) / (U24 * size)).max():.3f}")
    assert np.all(np.abs(pair.imag) <= 4.0 * U24 * size)
    assert np.abs(pair.real - mean).max() > 0.1 * size.max()


def _modes(sc, idx):
    """the labelled scores of the modes idx (0-based), keeping their mode numbers"""
    import xeofs_amd as xe

    return xe.DataArray(sc.values[idx], sc.dims, {"mode": np.asarray(sc.coords["mode"])[idx], "time": sc.coords["time"]})


@pytest.mark.parametrize("n,P,seed", SHAPES[:1])
def test_accessors(ctx, n, P, seed):
    m, X, ref, match = fitted(n, P, seed)
    q = 8
    C, Sc = m.components().values, m.scores().values
    assert C.shape == (q, P) and Sc.shape == (q, n)
    assert np.array_equal(C, m.data["components"].T) and np.array_equal(Sc, m.data["scores"].T)
    assert np.array_equal(m.components_amplitude().values, np.abs(C))
    assert np.array_equal(m.components_phase().values, np.angle(C))
    assert np.array_equal(m.scores_amplitude().values, np.abs(Sc / m.data["norms"][:, None]))        # normalized by default
    assert np.array_equal(m.scores_amplitude(normalized=False).values, np.abs(Sc))
    assert np.array_equal(m.scores_phase().values, np.angle(Sc))
    assert np.array_equal(m.scores(normalized=True).values, Sc / m.data["norms"][:, None])
    for name in ("eigenvalues", "damping_times", "periods"):
        assert np.array_equal(getattr(m, name)().values, m.data[name])
    for key in ("route", "n_pca_modes", "ms_pca", "ms_lagcov", "ms_eigen", "ms_project"):
        assert key in m.stats
    assert m.stats["n_pca_modes"] == q


# ------------------------------------------------------------------------------------------------ 3. determinism, errors
def test_a_second_fit_is_bitwise_equal(ctx):
    import xeofs_amd as xe

    n, P, seed = SHAPES[0]
    a, X, _, _ = fitted(n, P, seed)
    b = xe.single.POP(n_pca_modes=8, random_state=0).fit(da(X), dim="time")
    for name in ("components", "scores", "norms", "eigenvalues", "damping_times", "periods", "total_variance"):
        assert np.array_equal(a.data[name], b.data[name]), name


def test_n_pca_modes_forms(ctx):
    """a variance fraction and "all" go through the same Decomposer; n_modes does not truncate"""
    import xeofs_amd as xe

    X = oscillators(130, 40, 0)
    m = xe.single.POP(n_modes=2, n_pca_modes="all", solver="full").fit(da(X), dim="time")
    assert m.data["scores"].shape == (130, 40) and m.data["components"].shape == (40, 40)
    m = xe.single.POP(n_modes=2, n_pca_modes=0.9, pca_init_rank_reduction=0.5).fit(da(X), dim="time")
    q = m.stats["n_pca_modes"]
    assert 2 < q <= 20 and m.data["scores"].shape == (130, q)


def test_errors(ctx):
    import xeofs_amd as xe

    X = oscillators(60, 20, 0)
    with pytest.raises(NotImplementedError, match="use_pca=False"):
        xe.single.POP(use_pca=False).fit(da(X), dim="time")
    Z = (X[:30, :6] + 1j * X[30:, :6]).astype(np.complex64)
    with pytest.raises(TypeError, match="does not support complex data"):
        xe.single.POP(n_pca_modes=4).fit(da(Z), dim="time")
    with pytest.raises(ValueError, match="at least 3 samples"):
        xe.single.POP(n_pca_modes=2).fit(da(X[:2]), dim="time")
