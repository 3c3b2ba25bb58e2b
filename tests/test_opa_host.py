"""Host tests of optimal persistence analysis (xeofs_amd.single.OPA): the lag weights of the filtered form against the
weights the reference's loop applies (xeofs/single/opa.py:154-166), the constructor's errors, the export.  No GPU."""

import numpy as np
import pytest


def loop_weights(n, T):
    """the factor each C_tau = S[:n - tau]^T S[tau:] / (n - tau - 1) carries in M = 1/2 C_0 + C_1 + ... + 1/2 C_T"""
    w = np.zeros(T + 1)
    w[0] += 0.5 / (n - 1)
    for tau in range(1, T + 1):
        f = 0.5 if tau == T else 1.0
        w[tau] += f / (n - tau - 1)
    return w


def test_opa_is_exported():
    import xeofs_amd as xe

    assert hasattr(xe.single, "OPA")
    from xeofs_amd.single.opa import OPA, opa_lag_weights  # noqa: F401

    assert xe.single.OPA is OPA


@pytest.mark.parametrize("n,T", [(3, 1), (10, 1), (10, 2), (10, 8), (600, 20), (2000, 50), (300, 8), (301, 299), (64, 62)])
def test_lag_weights_are_the_loops(n, T):
    from xeofs_amd.single.opa import opa_lag_weights

    w = opa_lag_weights(n, T)
    assert w.dtype == np.float64 and w.shape == (T + 1,)
    np.testing.assert_allclose(w, loop_weights(n, T), rtol=4e-16, atol=0)


def test_lag_weights_reproduce_the_lagged_sum():
    """M of the filtered form = the loop over tau, on a small float64 example"""
    from xeofs_amd.single.opa import opa_lag_weights

    rng = np.random.default_rng(0)
    n, q, T = 57, 5, 9
    S = rng.standard_normal((n, q))
    M = 0.5 * S.T @ S / (n - 1)
    for tau in range(1, T + 1):
        C = S[:n - tau].T @ S[tau:] / (n - tau - 1)
        M += 0.5 * C if tau == T else C
    w = opa_lag_weights(n, T)
    Y = np.zeros_like(S)
    for tau in range(T + 1):
        Y[:n - tau] += w[tau] * S[tau:]
    np.testing.assert_allclose(S.T @ Y, M, rtol=0, atol=1e-14 * np.abs(M).max())


def test_lag_weights_range():
    from xeofs_amd.single.opa import opa_lag_weights

    for n, T in [(10, 9), (10, 10), (10, -1), (2, 1)]:
        with pytest.raises(ValueError, match="tau_max must be in"):
            opa_lag_weights(n, T)


def test_constructor_errors_and_defaults():
    from xeofs_amd.single import OPA

    with pytest.raises(ValueError, match=r"n_modes must be smaller or equal to n_pca_modes \(n_modes=11, n_pca_modes=10\)"):
        OPA(n_modes=11, tau_max=5, n_pca_modes=10)
    with pytest.raises(TypeError):
        OPA()                                               # n_modes and tau_max have no defaults (opa.py:68-83)
    m = OPA(n_modes=10, tau_max=50)
    prm = m.get_params()
    assert prm["n_pca_modes"] == 100 and prm["tau_max"] == 50 and prm["n_modes"] == 10
    assert prm["center"] is True and prm["standardize"] is False and prm["use_coslat"] is False
    assert prm["solver"] == "auto" and prm["random_state"] is None and prm["check_nans"] is True
    assert m.attrs["model"] == "OPA"
    assert OPA(n_modes=100, tau_max=5).get_params()["n_modes"] == 100        # n_modes == n_pca_modes is allowed


def test_transform_is_not_implemented():
    from xeofs_amd.single import OPA

    m = OPA(n_modes=2, tau_max=3, n_pca_modes=4)
    with pytest.raises(NotImplementedError, match=r"OPA does not \(yet\) support transform\(\)"):
        m.transform(np.zeros((5, 3), np.float32))
    with pytest.raises(NotImplementedError, match=r"OPA does not \(yet\) support inverse_transform\(\)"):
        m.inverse_transform(np.zeros((5, 2), np.float32))
