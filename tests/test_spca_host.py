"""CPU tests of SparsePCA's boundary (xeofs_amd.single.SparsePCA, include/eofx.h eofx_spca_*): the class, its parameters,
the argument errors raised before any device work, the ABI rows and the explained-variance rescaling."""

import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPCA_SYMBOLS = ("eofx_spca_loop_f64", "eofx_spca_gram_f64", "eofx_spca_rowmul_f64", "eofx_spca_prox_f64")


def test_importable_from_single():
    from xeofs_amd.single import SparsePCA

    assert SparsePCA.__name__ == "SparsePCA"


def test_defaults_and_params_match_reference_names():
    from xeofs_amd.single import SparsePCA

    prm = SparsePCA().get_params()
    expect = dict(n_modes=2, alpha=1e-3, beta=1e-3, robust=False, regularizer="l1", max_iter=500, tol=1e-6, oversample=10,
                  n_subspace=1, n_blocks=1, center=True, standardize=False, use_coslat=False, check_nans=True,
                  sample_name="sample", feature_name="feature", compute=True, random_state=None, solver="auto",
                  solver_kwargs={})
    for key, val in expect.items():
        assert prm[key] == val, key
    prm = SparsePCA(n_modes=3, alpha=0.5, regularizer="l0", max_iter=7, random_state=4).get_params()
    assert (prm["n_modes"], prm["alpha"], prm["regularizer"], prm["max_iter"], prm["random_state"]) == (3, 0.5, "l0", 7, 4)


def _da(values):
    from xeofs_amd import labelled

    return labelled.DataArray(values, ("sample", "feature"))


def _no_device(monkeypatch):
    from xeofs_amd import engine

    def boom(*a, **k):
        raise AssertionError("device work before the argument check")

    monkeypatch.setattr(engine, "default_context", boom)


def test_complex_input_raises_type_error(monkeypatch):
    from xeofs_amd.single import SparsePCA

    _no_device(monkeypatch)
    X = _da(np.ones((10, 4), np.complex64))
    with pytest.raises(TypeError):
        SparsePCA().fit(X, "sample")


@pytest.mark.parametrize("kw, err", [(dict(solver="arpack"), ValueError), (dict(regularizer="l2"), ValueError),
                                     (dict(robust=True, regularizer="l0"), NotImplementedError)])
def test_bad_arguments_raise_before_device_work(monkeypatch, kw, err):
    from xeofs_amd.single import SparsePCA

    _no_device(monkeypatch)
    X = _da(np.random.default_rng(0).standard_normal((10, 4)).astype(np.float32))
    with pytest.raises(err):
        SparsePCA(**kw).fit(X, "sample")


def test_abi_symbols_declared_and_exported():
    from xeofs_amd import _lib

    header = open(os.path.join(ROOT, "include", "eofx.h")).read()
    lib = _lib.load()
    for s in SPCA_SYMBOLS:
        assert f"int {s}(" in header, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s


def test_explained_variance_rescaling():
    from xeofs_amd.single.sparse_pca import explained_variance

    dt = np.array([30.0, 20.0, 10.0])
    # exact route: Dtilde / (n - 1)
    np.testing.assert_allclose(explained_variance(dt, 51, 51, 3, 10, True), dt / 50)
    # randomized route, m_c = l = k + oversample rows: Dtilde / (l - 1) * (l - 1) / (n - 1) = Dtilde / (n - 1)
    np.testing.assert_allclose(explained_variance(dt, 101, 13, 3, 10, False), dt / 100)
    # randomized route with fewer samples than l: m_c = min(n, l) = n
    n = 9
    np.testing.assert_allclose(explained_variance(dt, n, n, 3, 10, False), dt / (n - 1) * 12 / (n - 1))


def test_auto_solver_rule():
    from xeofs_amd.single import SparsePCA

    m = SparsePCA(n_modes=9)
    assert m.use_exact(20, 10)                  # 9 > int(0.8 * 10) = 8, max(n, p) < 500
    assert not m.use_exact(20, 12)              # int(0.8 * 12) = 9
    assert not m.use_exact(600, 10)
    assert SparsePCA(n_modes=1, solver="full").use_exact(10000, 10000)
    assert not SparsePCA(n_modes=9, solver="randomized").use_exact(20, 10)
