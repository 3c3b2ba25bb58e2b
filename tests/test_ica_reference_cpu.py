"""The float64 restatement of ICA (tests/ica_reference.py) pinned without a GPU: against sklearn.decomposition.FastICA(whiten=False,
w_init=...) live on W and the iteration count for all three contrast functions; its identities (W orthogonal after a step, the
polar factor by eigh against the SVD route, the explained variances summing to the PCA's); gamma against closed forms and a fine
quadrature; the float32 emulation inside the bounds the GPU tests hold the device to; and the CONDITION of the GPU cases that
assert an iteration count: the reference's lim at the deciding iteration and the one before lies outside [tol / 2, 2 tol]."""

import warnings

import numpy as np
import pytest

import ica_reference as kr


@pytest.mark.parametrize("fun", kr.FUNS)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_against_scikit_learn(fun, seed):
    dec = pytest.importorskip("sklearn.decomposition")
    Z, _ = kr.mixed_panel(seed, 2048, 6)
    Z = Z.astype(np.float64)
    w_init = np.random.RandomState(seed).normal(size=(6, 6))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ica = dec.FastICA(n_components=6, algorithm="parallel", whiten=False, fun=fun, fun_args=dict(alpha=1.0), max_iter=200, tol=1e-4,
                          w_init=w_init).fit(Z)
    ref = kr.run(Z, kr.sym_decorrelation(w_init), fun, 1.0, 1e-4, 200)
    assert ref["iters"] == ica.n_iter_ and ref["status"] == 1
    assert np.abs(ref["W"] - ica.components_).max() <= 1e-13


def test_scikit_learn_alpha():
    dec = pytest.importorskip("sklearn.decomposition")
    Z, _ = kr.mixed_panel(9, 1500, 5)
    Z = Z.astype(np.float64)
    w_init = np.random.RandomState(9).normal(size=(5, 5))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ica = dec.FastICA(n_components=5, whiten=False, fun="logcosh", fun_args=dict(alpha=1.7), w_init=w_init).fit(Z)
    ref = kr.run(Z, kr.sym_decorrelation(w_init), "logcosh", 1.7, 1e-4, 200)
    assert ref["iters"] == ica.n_iter_ and np.abs(ref["W"] - ica.components_).max() <= 1e-13


@pytest.mark.parametrize("fun", kr.FUNS)
def test_identities(fun):
    rs = np.random.RandomState(3)
    Z, W0 = kr.mixed_panel(3, 1000, 7)
    st = kr.step(Z, W0, fun)
    assert np.abs(st["W"] @ st["W"].T - np.eye(7)).max() <= 1e-13
    assert np.abs(st["W"] - kr.polar(st["W1"])).max() <= 1e-12
    lam = np.sort(rs.uniform(0.5, 9.0, 7))[::-1]
    _, _, ev, order = kr.carry_back(st["W"], np.sqrt(lam * 999), 1000, lam)
    assert abs(ev.sum() - lam.sum()) <= 1e-12 * lam.sum() and (np.diff(ev) <= 0).all() and sorted(order) == list(range(7))
    # a row with a NaN is left out of everything
    bad = Z.copy()
    bad[17, 2] = np.nan
    W1, gmean, nused = kr.moments(bad, W0, fun)
    W1k, gmeank, _ = kr.moments(np.delete(Z, 17, axis=0), W0, fun)
    assert nused == 999 and np.array_equal(W1, W1k) and np.array_equal(gmean, gmeank)


def test_degenerate_steps():
    rs = np.random.RandomState(0)
    W = kr.random_orthogonal(5, rs)
    assert kr.step(np.zeros((10, 5)), W, "cube")["W"] is None
    st = kr.step(np.zeros((10, 5)), W, "logcosh", 1.5)
    assert np.array_equal(st["W1"], -1.5 * W) and st["lim"] <= 1e-15
    twin = W.copy()
    twin[3] = twin[0]
    Z, _ = kr.mixed_panel(1, 512, 5)
    assert kr.step(Z, twin, "logcosh")["W"] is None
    assert kr.step(np.full((4, 5), np.nan), W, "exp")["W"] is None
    assert kr.run(np.zeros((10, 5)), W, "cube")["status"] == 2


def test_gamma():
    # closed forms: E[nu^4] / 4 = 3 / 4;  E[-exp(-nu^2 / 2)] = -1 / sqrt(2)
    # logcosh: 64 Gauss-Hermite nodes against a fine trapezoid sum.  log cosh has its branch points at +-i pi / (2 alpha): the
    # nearer they come to the real axis the slower the rule converges -- 1.3e-11 at alpha = 1, 1.9e-8 at 1.5, 7.4e-7 at 2
    # (measured here); the last is three times the float32 error of the device's G and shifts every restart's contrast alike.
    x = np.linspace(-12.0, 12.0, 480001)
    pdf = np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)
    for fun, alpha, tol in (("cube", 1.0, 1e-12), ("exp", 1.0, 1e-12), ("logcosh", 1.0, 1e-10), ("logcosh", 1.5, 1e-7), ("logcosh", 2.0, 1e-6)):
        f = kr.contrast(x, fun, alpha)[2] * pdf
        fine = float(((f[1:] + f[:-1]) * 0.5 * np.diff(x)).sum())
        assert abs(kr.gamma(fun, alpha) - fine) <= tol, (fun, alpha, kr.gamma(fun, alpha) - fine)
    assert kr.gamma("cube") == 0.75 and kr.gamma("exp") == -1.0 / np.sqrt(2.0)
    from xeofs_amd.single import ica

    for fun, alpha in (("cube", 1.0), ("exp", 1.0), ("logcosh", 1.0), ("logcosh", 1.3), ("logcosh", 2.0)):
        assert abs(ica.ica_gamma(fun, alpha) - kr.gamma(fun, alpha)) <= 1e-15


def test_contrast_forms_agree():
    s = np.linspace(-9.0, 9.0, 20001)
    for fun, alpha in (("logcosh", 1.0), ("logcosh", 2.0), ("exp", 1.0), ("cube", 1.0)):
        g, gp, G = kr.contrast(s, fun, alpha)
        h = 1e-6
        dG = (kr.contrast(s + h, fun, alpha)[2] - kr.contrast(s - h, fun, alpha)[2]) / (2 * h)
        dg = (kr.contrast(s + h, fun, alpha)[0] - kr.contrast(s - h, fun, alpha)[0]) / (2 * h)
        assert np.abs(dG - g).max() <= 1e-6 * (1 + np.abs(g).max()) and np.abs(dg - gp).max() <= 1e-6 * (1 + np.abs(gp).max())
        if fun == "logcosh":
            assert np.abs(G - np.log(np.cosh(alpha * s)) / alpha).max() <= 1e-14 * 20


@pytest.mark.parametrize("n,q", [(1500, 5), (777, 32)])
@pytest.mark.parametrize("fun,alpha", [("logcosh", 1.0), ("logcosh", 2.0), ("exp", 1.0), ("cube", 1.0)])
def test_float32_emulation_inside_the_bounds(n, q, fun, alpha):
    """the inputs of tests/test_gpu_ica_step.py::test_moments_general"""
    rs = np.random.RandomState(11 * n + q)
    for Z in (rs.standard_normal((n, q)).astype(np.float32), rs.standard_t(3, size=(n, q)).astype(np.float32)):
        W = kr.random_orthogonal(q, rs)
        W1, gmean, _ = kr.moments(Z, W, fun, alpha)
        E1, egmean, _ = kr.moments(Z, W, fun, alpha, f32=True)
        b1 = kr.moment_bound(Z, W, fun, alpha)
        assert (np.abs(E1 - W1) <= b1).all(), np.max(np.abs(E1 - W1) / b1)
        assert (np.abs(egmean - gmean) <= kr.gmean_bound(Z, W, fun, alpha)).all()


def test_emulated_fmaf_chain():
    rs = np.random.RandomState(2)
    Z = rs.standard_normal((300, 9)).astype(np.float32)
    W = kr.random_orthogonal(9, rs)
    S = kr.project(Z, W, f32=True)
    assert np.array_equal(S, kr.r32(S))
    ds = 10 * kr.U32 * (np.abs(Z.astype(np.float64)) @ np.abs(W).T)
    assert (np.abs(S - kr.project(Z, W)) <= ds).all()
    # exact on integers
    Zi = rs.randint(-3, 4, size=(64, 9)).astype(np.float32)
    Wi = rs.randint(-1, 2, size=(9, 9)).astype(np.float64)
    assert np.array_equal(kr.project(Zi, Wi, f32=True), kr.project(Zi, Wi))
    g, gp, G = kr.contrast(kr.project(Zi, Wi), "cube", f32=True)
    assert np.array_equal(g, kr.contrast(kr.project(Zi, Wi), "cube")[0])


@pytest.mark.parametrize("case", kr.RUN_CASES, ids=lambda c: f"{c[0]}-{c[1]}-q{c[4]}")
def test_condition_of_the_gpu_cases(case):
    fun, alpha, seed, n, q, tol = case
    Z, W0 = kr.mixed_panel(seed, n, q)
    assert np.abs(Z.astype(np.float64).T @ Z.astype(np.float64) / n - np.eye(q)).max() <= 1e-5
    assert np.abs(W0 @ W0.T - np.eye(q)).max() <= 1e-13
    ref = kr.run(Z, W0, fun, alpha, tol, 200)
    emu = kr.run(Z, W0, fun, alpha, tol, 200, f32=True)
    assert ref["status"] == 1 and ref["iters"] >= 3 and emu["iters"] == ref["iters"]
    for lim in ref["lims"][-2:]:
        assert not 0.5 * tol <= lim <= 2.0 * tol, ref["lims"]
    assert ref["lims"][-2] >= tol > ref["lims"][-1]
    assert np.abs(emu["W"] - ref["W"]).max() <= 1e-6


def test_planted_seed_of_the_model_test():
    """tests/test_gpu_ica.py plants four sources in 96 features: the reference itself recovers them to 0.99 from this seed"""
    X, S = kr.planted_field(kr.PLANTED_SEED)
    Z, sigma, V, lam = kr.pca_white(X, 4)
    fit = kr.fit(Z, kr.starts(4, 1, kr.PLANTED_START), "logcosh")
    src = Z.astype(np.float64) @ fit["runs"][0]["W"].T
    assert kr.recovery(src, S) >= 0.99 and kr.well_conditioned(fit["runs"][0], 1e-4, 0.4, 2.5)
