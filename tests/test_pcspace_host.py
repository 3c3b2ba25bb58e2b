"""Host tests of the steps the PC-space models share (xeofs_amd.single._pcspace): the whitened symmetric eigenproblem
against a plain NumPy float64 restatement on three small fixed problems, and the two singularity rules.  No GPU: the
eigensolver is the library's host routine (engine.host_eigh)."""

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps


def problem(q, seed):
    """C0 = E D E^T with eigenvalues 1 .. 10 (condition number 10) and a symmetric A whose whitened form
    K A K^T, K = D^-1/2 E^T, has the eigenvalues q, q - 1, ..., 1: gaps of 1 between any two, asserted where used"""
    rng = np.random.default_rng(seed)
    E = np.linalg.qr(rng.standard_normal((q, q)))[0]
    Q = np.linalg.qr(rng.standard_normal((q, q)))[0]
    d = np.linspace(10.0, 1.0, q) if q > 1 else np.array([4.0])
    C0 = (E * d) @ E.T
    H = E * np.sqrt(d)                                       # K^-1
    A = H @ (Q * np.arange(q, 0, -1.0)) @ Q.T @ H.T
    return 0.5 * (C0 + C0.T), 0.5 * (A + A.T)


def restatement(C0, A, k):
    """whitened_modes in NumPy: numpy.linalg.eigh, descending"""
    d, E = np.linalg.eigh(C0)
    d, E = d[::-1], E[:, ::-1]
    K = E.T / np.sqrt(d)[:, None]
    Tm = K @ A @ K.T
    v, U = np.linalg.eigh(0.5 * (Tm + Tm.T))
    v, U = v[::-1], U[:, ::-1]
    Vq = K.T @ U[:, :k]
    return v, Vq, C0 @ Vq, d


@pytest.mark.parametrize("q,k,seed", [(1, 1, 0), (7, 3, 1), (12, 12, 2)])
def test_whitened_modes_against_numpy(q, k, seed):
    from xeofs_amd.single._pcspace import whitened_modes

    C0, A = problem(q, seed)
    v, Vq_ref, Wq_ref, d = restatement(C0, A, k)
    gaps = v[:min(k, q - 1)] - v[1:k + 1]                    # between consecutive wanted values and to the next one
    assert np.all(gaps >= 0.9) and gaps.size == min(k, q - 1)
    values, Uo, Vq, Wq = whitened_modes(C0, A, k)
    assert values.shape == (k,) and Uo.shape == (q, k) and Vq.shape == (q, k) and Wq.shape == (q, k)
    assert Uo.flags.c_contiguous and np.all(np.diff(values) < 0)
    # Both sides round Tm = K A K^T in float64: an error of the order q eps cond(C0) |Tm| (|K|^2 |A| <= cond(C0) |Tm|),
    # which moves an eigenvalue by at most as much (Weyl) and an eigenvector by that over the gap (Davis-Kahan).  50: the
    # constants of the two eigensolvers and of the three products.
    cond, top = d[0] / d[-1], v[0]
    tol = 50 * q * EPS * cond * top
    assert np.all(np.abs(values - v[:k]) <= tol)
    # the whitened eigenvectors carry the sign and the basis of E that the solver of C0 happened to return; Vq = K^T Uo
    # does not, up to one sign per mode
    sign = np.sign((Vq * Vq_ref).sum(axis=0))
    vtol = tol / (gaps.min() if gaps.size else top) * np.abs(Vq_ref).max()
    assert np.all(np.abs(Vq * sign - Vq_ref) <= vtol)
    assert np.all(np.abs(Wq * sign - Wq_ref) <= vtol * d[0])
    assert np.array_equal(Wq, C0 @ Vq)
    # the defining properties: Uo orthonormal, Vq^T C0 Vq = I, Vq^T A Vq = diag(values)
    assert np.all(np.abs(Uo.T @ Uo - np.eye(k)) <= 50 * q * EPS)
    assert np.all(np.abs(Vq.T @ C0 @ Vq - np.eye(k)) <= 50 * q * EPS * cond)
    assert np.all(np.abs(Vq.T @ A @ Vq - np.diag(values)) <= tol)


def test_both_rules_raise_on_a_rank_deficient_covariance():
    from xeofs_amd.single import _pcspace

    C0 = np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]])          # eigenvalues 3, 1 and an exact 0
    A = np.eye(3)
    with pytest.raises(np.linalg.LinAlgError, match="singular: fewer independent modes than n_pca_modes=3"):
        _pcspace.whitened_modes(C0, A, 2)
    with pytest.raises(np.linalg.LinAlgError, match="singular: fewer independent modes than n_pca_modes=3"):
        _pcspace.whitened_modes(C0, A, 2, rank_rows=50)


def test_the_float32_rule_alone_raises_below_its_threshold():
    """smallest eigenvalue 1e-16 > 0: its root 1e-8 is below max(n, q) eps32 sqrt(d_0) = 50 x 1.19e-7 x sqrt(3)"""
    from xeofs_amd.single import _pcspace

    C0 = np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1e-16]])
    A = np.diag([3.0, 2.0, 1.0])
    values, _, Vq, _ = _pcspace.whitened_modes(C0, A, 2)
    assert np.all(np.isfinite(values)) and np.all(np.isfinite(Vq))
    with pytest.raises(np.linalg.LinAlgError, match="singular"):
        _pcspace.whitened_modes(C0, A, 2, rank_rows=50)
    # a smallest eigenvalue of 1e-3 passes both (its root 0.03 is above the threshold 1e-5)
    C0[2, 2] = 1e-3
    assert np.array_equal(_pcspace.whitened_modes(C0, A, 2, rank_rows=50)[0], _pcspace.whitened_modes(C0, A, 2)[0])
