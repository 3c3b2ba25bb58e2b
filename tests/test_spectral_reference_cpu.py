"""The float64 restatement of spectral EOF analysis (tests/spectral_reference.py) against scipy.signal.welch / csd and against
the identities of the definition.  No GPU."""

import numpy as np
import pytest

import spectral_reference as sr

scipy_signal = pytest.importorskip("scipy.signal")


def field(n, p, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)).cumsum(axis=0) * 0.1 + rng.standard_normal((n, p))
    return X - X.mean(axis=0)


CASES = [(n_fft, ov, win) for n_fft in (16, 15) for ov in (0, 1, None, "max") for win in ("hamming", "hann", "boxcar")]


@pytest.mark.parametrize("n_fft,ov,win", CASES)
def test_diagonal_is_welch_and_pairs_are_csd(n_fft, ov, win):
    n, p, dt = 103, 4, 0.5
    ov = n_fft // 2 if ov is None else (n_fft - 1 if ov == "max" else ov)
    X = field(n, p, seed=n_fft + ov)
    Q = sr.realisations(X, n_fft, ov, win, dt)
    nblk = Q.shape[1]
    assert nblk == (n - ov) // (n_fft - ov)
    kw = dict(fs=1.0 / dt, window=win, nperseg=n_fft, noverlap=ov, detrend=False, scaling="density", return_onesided=True)
    f, P = scipy_signal.welch(X, axis=0, **kw)
    assert np.allclose(f, np.arange(n_fft // 2 + 1) / (dt * n_fft), rtol=1e-14)
    mine = np.einsum("kbj,kbj->kj", np.conj(Q), Q).real / nblk
    assert np.allclose(mine, P, rtol=1e-12, atol=1e-12 * np.abs(P).max())
    for i, j in [(0, 1), (2, 3), (3, 0)]:
        _, Pij = scipy_signal.csd(X[:, i], X[:, j], **kw)
        for k in (0, 1, n_fft // 4, n_fft // 2):
            S = sr.density_matrix(Q[k])
            assert abs(np.conj(S[i, j]) - Pij[k]) <= 1e-12 * np.abs(Pij).max()


def test_block_detrend_is_detrend_constant():
    n, p, n_fft, ov = 120, 3, 16, 8
    X = field(n, p, seed=4) + 3.0
    Q = sr.realisations(X, n_fft, ov, "hann", 1.0, block_detrend=True)
    _, P = scipy_signal.welch(X, axis=0, fs=1.0, window="hann", nperseg=n_fft, noverlap=ov, detrend="constant", scaling="density")
    mine = np.einsum("kbj,kbj->kj", np.conj(Q), Q).real / Q.shape[1]
    assert np.allclose(mine, P, rtol=1e-12, atol=1e-12 * np.abs(P).max())


@pytest.mark.parametrize("n_fft,ov", [(16, 8), (15, 4)])
def test_modes_are_orthonormal_eigenvectors_and_scores_are_projections(n_fft, ov):
    n, p, K = 160, 7, 3
    X = field(n, p, seed=9)
    d = sr.decompose(X, n_fft, ov, K)
    nblk = d["Q"].shape[1]
    for k in range(n_fft // 2 + 1):
        Phi = d["Phi"][k].T                                                  # [p x K]
        assert np.allclose(np.conj(Phi.T) @ Phi, np.eye(K), atol=1e-10)
        S = sr.density_matrix(d["Q"][k])
        assert np.allclose(S @ Phi, Phi * d["lam"][k, :K], atol=1e-10 * d["lam"][k, 0])
        assert np.allclose(np.conj(Phi.T) @ d["Q"][k].T, d["a"][k], atol=1e-10 * np.sqrt(nblk * d["lam"][k, 0]))
        assert np.isclose(d["trace"][k], d["lam"][k].sum(), rtol=1e-12)
        # the gauge: the entry of largest modulus is real and positive
        for m in range(K):
            z = Phi[np.argmax(np.abs(Phi[:, m])), m]
            assert z.real > 0 and abs(z.imag) <= 1e-14


@pytest.mark.parametrize("n_fft", [16, 15])
def test_parseval_for_the_boxcar_window_without_overlap(n_fft):
    """sum_k sum_m lambda fs / n_fft = the mean square of the blocked samples, summed over the features: exactly"""
    n, p, dt = 8 * n_fft + 3, 5, 0.25
    X = field(n, p, seed=2)
    d = sr.decompose(X, n_fft, 0, 2, "boxcar", dt)
    Xb = sr.blocks(X, n_fft, 0)
    assert np.isclose(d["lam"].sum() / (dt * n_fft), np.sum(Xb * Xb) / (Xb.shape[0] * n_fft), rtol=1e-12)
    assert np.isclose(d["trace"].sum() / (dt * n_fft), np.sum(Xb * Xb) / (Xb.shape[0] * n_fft), rtol=1e-12)


def test_the_red_noise_field_has_gaps_for_three_modes_at_every_frequency():
    """what tests/test_gpu_spectraleof.py relies on: at every frequency the leading three eigenvalues of the reference are
    separated from all others by more than ten times the bound of |M_hat - M|_F"""
    n, p, n_fft, ov, K = 400, 300, 64, 32, 3
    X = sr.red_noise_field(n, p)
    assert X.dtype == np.float32
    from xeofs_amd.single import spectral_eof as se

    B = se.coefficient_matrix(n_fft, "hamming", dtype=np.float64)
    gb, _ = sr.gram_error_bound(X, B, n_fft, ov)
    d = sr.decompose(X, n_fft, ov, K)
    nblk = d["Q"].shape[1]
    mb = sr.m_error_bound(gb, nblk)
    lam = d["lam"]
    for k in range(n_fft // 2 + 1):
        for m in range(K):
            gap = min(lam[k, m - 1] - lam[k, m] if m else np.inf, lam[k, m] - lam[k, m + 1])
            assert gap > 10.0 * mb[k], (k, m, gap, mb[k])
