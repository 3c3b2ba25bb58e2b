"""GPU tests of xeofs_amd.single.SpectralEOF against the float64 restatement of tests/spectral_reference.py.

(a) a designed field whose spectrum is known in closed form; (b) a red-noise field, where every figure is held against a bound
composed from the two operator bounds (spectral_reference.gram_error_bound) through Weyl's inequality and the Davis-Kahan
theorem; (c) chunking, the gauge, masks, weights, block_detrend and the rank-deficient rule.
"""

import numpy as np
import pytest

import spectral_reference as sr

pytestmark = pytest.mark.gpu

_cache = {}


def array(X, lat=None):
    import xeofs_amd as xe

    n, p = X.shape
    if lat is None:
        return xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})
    nlat = len(lat)
    return xe.DataArray(X.reshape(n, nlat, p // nlat), ("time", "lat", "lon"),
                        {"time": np.arange(n), "lat": np.asarray(lat), "lon": np.arange(p // nlat) * 2.5})


def fit(ctx, X, lat=None, **kw):
    import xeofs_amd as xe

    m = xe.single.SpectralEOF(**kw)
    m.ctx = ctx
    return m.fit(array(X, lat), dim="time")


def seen(ctx, m, X):
    """the preprocessed float32 field the fit saw (centred, weights applied, masked features dropped) [n x p_valid]"""
    from xeofs_amd import engine

    pre = m.preprocessor
    mat, st = engine.preprocess(ctx, X, True, False, pre.feature_weights, in_place=True)
    try:
        assert np.array_equal(st["valid_feature"], pre.valid_feature) and not mat.masked
        return mat.download()
    finally:
        mat.free()


def comps(m):
    """[nfreq x K x P] in the input's feature order"""
    C = np.asarray(m.components().values)
    return C.reshape(C.shape[0], C.shape[1], -1)


# ------------------------------------------------------------------------------------------------ (a) a designed field
N_FFT, NBLK_A, P_A = 64, 6, 300
K1, K2, K3 = 5, 11, 20
A1, A2, A3 = 2.0, 1.0, 1e-3


def designed():
    """x[t, j] = Re(A1 phi1_j e^{2 pi i K1 t / N}) + Re(A2 phi2_j e^{2 pi i K2 t / N}) + A3 phi3_j cos(2 pi K3 t / N): two
    travelling waves with orthonormal complex patterns and a weak standing one, each exactly on a bin of a boxcar window of N
    samples; n is a whole number of periods, so every column has mean zero."""
    rng = np.random.default_rng(7)
    Z = np.linalg.qr(rng.standard_normal((P_A, 2)) + 1j * rng.standard_normal((P_A, 2)))[0]
    phi1, phi2 = Z[:, 0], Z[:, 1]
    phi3 = rng.standard_normal(P_A)
    phi3 /= np.linalg.norm(phi3)
    t = np.arange(N_FFT * NBLK_A, dtype=np.float64)[:, None]
    w = 2.0 * np.pi / N_FFT
    X = (A1 * (phi1[None, :] * np.exp(1j * w * K1 * t)).real + A2 * (phi2[None, :] * np.exp(1j * w * K2 * t)).real
         + A3 * phi3[None, :] * np.cos(w * K3 * t))
    return X, (phi1, phi2, phi3.astype(np.complex128))


@pytest.mark.parametrize("n_overlap", [0, N_FFT // 2])
def test_designed_waves_come_back_with_their_closed_form_spectrum(ctx, n_overlap):
    """Closed form.  For 0 < k < N / 2 the block DFT of Re(A phi_j e^{i w k t}) at bin k is (A N / 2) phi_j e^{i w k t0} (the
    conjugate term sums to zero over a whole block, and so does every other bin), so with the boxcar scale s^2 = 2 / (fs N),
    fs = 1: Q_k[b, j] = s (A N / 2) phi_j e^{i w k t0_b}, M_k = (A^2 N / 2) e e^H / nblk with |e_b| = 1, which has the single
    eigenvalue lambda = A^2 N / 2 and the mode phi.  The standing pattern A3 phi3 cos(.) is Re(A3 phi3 e^{i.}) with a real phi3:
    lambda = A3^2 N / 2.  Nothing is estimated: the only error is float32 rounding -- the field and B rounded once (2^-24 each),
    a chain of N = 64 terms in blockxform and chains of p = 300 in rowgram, at most (64 + 300 + 2) 2^-24 = 2.2e-5 if every
    rounding fell the same way and about its square root, 1e-6, when they do not.  The tolerance 1e-5 sits between the two."""
    X, phis = designed()
    m = fit(ctx, X.astype(np.float32), n_modes=1, n_fft=N_FFT, n_overlap=n_overlap, window="boxcar")
    lam = np.asarray(m.spectrum().values)[:, 0]
    tot = np.asarray(m.total_spectrum().values)
    C = comps(m)
    nblk = (X.shape[0] - n_overlap) // (N_FFT - n_overlap)
    assert m.stats["nblk"] == nblk and lam.shape == (N_FFT // 2 + 1,)
    np.testing.assert_allclose(np.asarray(m.frequencies().values), np.arange(N_FFT // 2 + 1) / N_FFT, rtol=1e-15)
    for k, A, phi in ((K1, A1, phis[0]), (K2, A2, phis[1]), (K3, A3, phis[2])):
        want = A * A * N_FFT / 2.0
        print(f"bin {k}: lambda {lam[k]:.9g} against {want:.9g} ({abs(lam[k] - want) / want:.2e}), "
              f"1 - |<phi_hat, phi>| = {1.0 - abs(np.vdot(C[k, 0], phi)):.2e}")
        assert abs(lam[k] - want) <= 1e-5 * want
        assert abs(tot[k] - want) <= 1e-5 * want
        assert abs(np.vdot(C[k, 0], phi)) >= 1.0 - 1e-5
        assert abs(np.vdot(C[k, 0], C[k, 0]) - 1.0) <= 1e-5
    # every other bin is empty to rounding: its exact realisations are zero, so what is there is at most the blockxform bound
    # E = (N + 2) 2^-24 |B| |x| (the chain, and one rounding each of B and of the field), and trace M = sum E^2 / nblk
    from xeofs_amd.single.spectral_eof import coefficient_matrix

    B = np.abs(coefficient_matrix(N_FFT, "boxcar", dtype=np.float64))
    Xb = np.abs(sr.blocks(X, N_FFT, n_overlap))
    E = (N_FFT + 2) * sr.U24 * np.einsum("ct,btj->cbj", B, Xb)
    empty = 1.01 * (np.sum(E[0::2] ** 2, axis=(1, 2)) + np.sum(E[1::2] ** 2, axis=(1, 2))) / nblk
    others = [k for k in range(N_FFT // 2 + 1) if k not in (K1, K2, K3)]
    print(f"empty bins: largest trace {tot[others].max():.3e}, bound {empty[others].min():.3e}")
    assert np.all(tot[others] <= empty[others]) and np.all(tot[others] <= 1e-9 * lam[K1])


# ------------------------------------------------------------------------------------------------ (b) red noise
def red(ctx):
    if "red" not in _cache:
        from xeofs_amd.single.spectral_eof import coefficient_matrix

        n, p, n_fft, K = 400, 300, 64, 3
        X = sr.red_noise_field(n, p)
        m = fit(ctx, X, n_modes=K, n_fft=n_fft)
        Xc = seen(ctx, m, X)
        ref = sr.decompose(Xc, n_fft, n_fft // 2, K)
        gb, R = sr.gram_error_bound(Xc, coefficient_matrix(n_fft, "hamming", dtype=np.float64), n_fft, n_fft // 2)
        nblk = ref["Q"].shape[1]
        assert np.allclose(R[:, :nblk] + 1j * R[:, nblk:], ref["Q"], rtol=0, atol=1e-11 * np.abs(ref["Q"]).max())
        _cache["red"] = (m, Xc, ref, sr.m_error_bound(gb, nblk))
    return _cache["red"]


def test_red_noise_snapshot_matrices_within_the_composed_bound(ctx):
    m, Xc, ref, mb = red(ctx)
    dM = np.sqrt(np.sum(np.abs(m.data["snapshot_matrix"] - ref["M"]) ** 2, axis=(1, 2)))
    print(f"|M_hat - M|_F / bound: largest {np.max(dM / mb):.3e}")
    assert np.all(dM <= mb)
    assert m.stats["nblk"] == 11 and m.stats["nfreq"] == 33


def test_red_noise_eigenvalues_by_weyl(ctx):
    m, Xc, ref, mb = red(ctx)
    dM = np.sqrt(np.sum(np.abs(m.data["snapshot_matrix"] - ref["M"]) ** 2, axis=(1, 2)))
    lam = m.data["spectrum_all"]
    assert np.all(np.abs(lam - ref["lam"]) <= dM[:, None] * (1 + 1e-9) + 1e-12 * ref["lam"][:, :1])
    np.testing.assert_array_equal(np.asarray(m.spectrum().values), lam[:, :3])
    np.testing.assert_allclose(np.asarray(m.total_spectrum().values), lam.sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(np.asarray(m.explained_variance_ratio().values), lam[:, :3] / lam.sum(axis=1, keepdims=True), rtol=1e-12)


def test_red_noise_eigenvectors_by_davis_kahan(ctx):
    """sin(theta_hat, theta) <= |M_hat - M|_F / gap, gap = the distance of lambda_m of M from every OTHER eigenvalue of M_hat
    (the form in which the theorem holds as stated); the reference's own gaps exceed ten times the bound
    (tests/test_spectral_reference_cpu.py), so these do by nine.  theta_hat is read off the scores: a = sqrt(nblk lambda)
    conj(theta) times a unit factor."""
    m, Xc, ref, mb = red(ctx)
    dM = np.sqrt(np.sum(np.abs(m.data["snapshot_matrix"] - ref["M"]) ** 2, axis=(1, 2)))
    a = m.data["scores"]
    lam_hat = m.data["spectrum_all"]
    nfreq, K, nblk = a.shape
    worst = 0.0
    for k in range(nfreq):
        _, Th = np.linalg.eigh(ref["M"][k])
        Th = Th[:, ::-1]
        for j in range(K):
            gap = np.min(np.abs(np.delete(lam_hat[k], j) - ref["lam"][k, j]))
            assert gap > 9.0 * mb[k]
            th = np.conj(a[k, j]) / np.linalg.norm(a[k, j])
            sin = np.sqrt(max(0.0, 1.0 - abs(np.vdot(Th[:, j], th)) ** 2))
            worst = max(worst, sin * gap / max(dM[k], 1e-300))
            assert sin <= dM[k] / gap + 1e-7                               # (1e-7: the square root of float64 rounding in 1 - c^2)
            np.testing.assert_allclose(np.linalg.norm(a[k, j]), np.sqrt(nblk * lam_hat[k, j]), rtol=1e-12)
    print(f"sin theta gap / |M_hat - M|_F: largest {worst:.3e}")


def test_red_noise_modes_are_orthonormal_and_expand_the_realisations(ctx):
    """Phi_hat^H Phi_hat - I = C^H (conj(Q_hat) Q_hat^T - nblk M_hat) C plus the rounding of slabmul (chains of 2 nblk terms,
    far below).  The middle matrix D is rowgram's error on four blocks of G: |D|_F <= 2 span 2^-24 nblk trace M_hat, and the
    columns of C have norm 1 / sqrt(nblk lambda_m): every entry is at most 2.02 span 2^-24 trace / sqrt(lambda_m lambda_m')."""
    m, Xc, ref, mb = red(ctx)
    C = comps(m).astype(np.complex128)
    lam, tr = m.data["spectrum"], m.data["total_spectrum"]
    worst = 0.0
    for k in range(C.shape[0]):
        D = np.abs(np.conj(C[k]) @ C[k].T - np.eye(3))
        bound = 2.02 * 2048 * sr.U24 * tr[k] / np.sqrt(np.outer(lam[k], lam[k]))
        worst = max(worst, float(np.max(D / bound)))
        assert np.all(D <= bound)
        # and they are the reference's modes: |<phi_hat, phi>| = cos of an angle whose sine Davis-Kahan bounds in block space;
        # in feature space the realisations add their own error, so this is a plain sanity level, not a bound
        for j in range(3):
            assert abs(np.vdot(ref["Phi"][k, j], C[k, j])) >= 0.999
    print(f"|Phi^H Phi - I| / bound: largest {worst:.3e}")


# ------------------------------------------------------------------------------------------------ (c) further cases
def test_results_do_not_depend_on_the_chunk(ctx):
    X = sr.red_noise_field(200, 261, seed=5)
    runs = [fit(ctx, X, n_modes=2, n_fft=16, freq_chunk=fc) for fc in (1, 2, None)]
    assert [r.stats["freq_chunk"] for r in runs] == [1, 2, 9]
    for r in runs[1:]:
        for key in ("components", "scores", "spectrum_all", "total_spectrum", "snapshot_matrix"):
            assert np.array_equal(runs[0].data[key].view(np.uint8), r.data[key].view(np.uint8)), key


def test_the_gauge_rule(ctx):
    m, Xc, ref, mb = red(ctx)
    C = comps(m)
    for k in range(C.shape[0]):
        for j in range(C.shape[1]):
            i = int(np.argmax(np.abs(C[k, j])))
            z = C[k, j, i]
            assert z.real > 0 and abs(z.imag) <= 4 * 2.0 ** -24 * abs(z)      # real and positive to float32 rounding
    # the scores carry the conjugate factor: a = Phi_hat^H q with the gauged Phi_hat.  Phi_hat^H q_b = conj(u) C^H conj(Q_hat) q_b
    # and conj(Q_hat) Q^T = nblk M_hat + D with |D|_F <= nblk |M_hat - M|_F-bound (the terms of gram_error_bound), so the row
    # of mode m differs from sqrt(nblk lambda_m) conj(theta_m) conj(u) by at most |C_m| |D|_F = bound sqrt(nblk / lambda_m);
    # 1.1 covers the rounding of slabmul
    a_ref = np.einsum("kmj,kbj->kmb", np.conj(C.astype(np.complex128)), ref["Q"])
    nblk = m.stats["nblk"]
    err = np.sqrt(np.sum(np.abs(m.data["scores"] - a_ref) ** 2, axis=2))
    lim = 1.1 * mb[:, None] * np.sqrt(nblk / m.data["spectrum"])
    print(f"scores against Phi_hat^H q: largest error / bound = {np.max(err / lim):.3e}")
    assert np.all(err <= lim)
    # equal moduli: the lowest index decides.  Column 4 is the exact negative of column 1, so their moduli are equal bit for
    # bit; the rule makes entry 1 real and positive and entry 4 its negative
    X = np.zeros((64, 6), dtype=np.float32)
    t = np.arange(64)
    X[:, 1] = np.cos(2 * np.pi * 3 * t / 16 + 0.3)
    X[:, 4] = -X[:, 1]
    m2 = fit(ctx, X, n_modes=1, n_fft=16, n_overlap=0, window="boxcar")
    c = comps(m2)[3, 0]
    assert abs(c[1]) == abs(c[4]) and c[1].real > 0 and abs(c[1].imag) <= 1e-6 and c[4].real < 0
    np.testing.assert_allclose(abs(c[1]), np.sqrt(0.5), rtol=1e-5)


def test_land_mask_coslat_and_block_detrend(ctx):
    from xeofs_amd.single.spectral_eof import coefficient_matrix

    n, p, n_fft, K = 200, 264, 32, 2
    lat = np.array([-60.0, -20.0, 10.0, 45.0])
    X = sr.red_noise_field(n, p, seed=9) + 3.0
    X[:, np.arange(p) % 7 == 2] = np.nan
    m = fit(ctx, X, lat=lat, n_modes=K, n_fft=n_fft, use_coslat=True, block_detrend=True)
    C = comps(m)
    vf = m.preprocessor.valid_feature
    assert np.array_equal(vf, np.arange(p) % 7 != 2)
    assert np.isnan(C[:, :, ~vf]).all() and np.isfinite(C[:, :, vf]).all()
    assert tuple(m.components().dims) == ("frequency", "mode", "lat", "lon")
    assert tuple(m.components_amplitude().dims) == tuple(m.components_phase().dims) == ("frequency", "mode", "lat", "lon")
    assert tuple(m.scores().dims) == ("frequency", "mode", "block")
    np.testing.assert_array_equal(np.asarray(m.scores().coords["block"]), np.arange(11) * 16 + 15.5)
    # the weights are in the field the fit saw: sqrt(cos(lat)) per row of the grid
    w = np.repeat(np.sqrt(np.cos(np.deg2rad(lat))), p // 4)
    np.testing.assert_allclose(m.preprocessor.feature_weights, w, rtol=1e-6)
    Xc = seen(ctx, m, X)
    ref = sr.decompose(Xc, n_fft, n_fft // 2, K, block_detrend=True)
    gb, _ = sr.gram_error_bound(Xc, coefficient_matrix(n_fft, "hamming", block_detrend=True, dtype=np.float64), n_fft, n_fft // 2)
    mb = sr.m_error_bound(gb, 11)
    dM = np.sqrt(np.sum(np.abs(m.data["snapshot_matrix"] - ref["M"]) ** 2, axis=(1, 2)))
    assert np.all(dM <= mb)
    assert np.all(np.abs(m.data["spectrum_all"] - ref["lam"]) <= dM[:, None] * (1 + 1e-9) + 1e-12 * ref["lam"][:, :1])
    # under a boxcar window block_detrend empties the zero frequency (a tapered window is applied AFTER the block's mean is
    # removed, as scipy does, and leaves some): row 0 of B is s - mean(s), zero to float64 rounding (at most n_fft 2^-52 s), so
    # the power there is below (32 2^-52)^2 = 5e-29 of its neighbour's; 1e-20 leaves room
    box = fit(ctx, X, lat=lat, n_modes=K, n_fft=n_fft, use_coslat=True, block_detrend=True, window="boxcar")
    assert box.data["total_spectrum"][0] <= 1e-20 * box.data["total_spectrum"][1]
    plain = fit(ctx, X, lat=lat, n_modes=K, n_fft=n_fft, use_coslat=True, window="boxcar")
    assert plain.data["total_spectrum"][0] > 1e-3 * plain.data["total_spectrum"][1]


def test_rank_deficient_modes_keep_lambda_and_lose_their_component(ctx):
    """a field that repeats with period hop: every block holds the same samples, one independent block for three modes"""
    rng = np.random.default_rng(3)
    base = rng.standard_normal((8, 130))
    X = np.tile(base, (10, 1)).astype(np.float32)                          # n = 80, n_fft = 16, hop = 8: 9 equal blocks
    m = fit(ctx, X, n_modes=3, n_fft=16)
    lam, ok, C = m.data["spectrum"], m.data["resolved"], comps(m)
    assert m.stats["nblk"] == 9
    assert np.all(np.isfinite(lam))
    np.testing.assert_array_equal(ok, lam > 9 * 2.0 ** -23 * lam[:, :1])
    live = lam[:, 0] > 1e-6 * lam[:, 0].max()                              # frequencies the period-8 field occupies
    assert live.sum() >= 3 and np.all(ok[live, 0]) and not ok[live, 1:].any()
    assert np.isnan(C[~ok]).all() and np.isfinite(C[ok]).all()
    for k in np.flatnonzero(live):
        assert abs(np.vdot(C[k, 0], C[k, 0]) - 1.0) <= 1e-4


def test_refusals_that_need_the_field(ctx):
    X = sr.red_noise_field(60, 40, seed=1)
    with pytest.raises(ValueError, match="n_fft"):
        fit(ctx, X, n_fft=61)
    with pytest.raises(ValueError, match="n_modes"):
        fit(ctx, X, n_fft=32, n_modes=3)                                   # (60 - 16) // 16 = 2 blocks
    with pytest.raises(ValueError, match="n_overlap"):
        fit(ctx, sr.red_noise_field(400, 8, seed=1), n_fft=8, n_overlap=7, n_modes=1)      # 393 blocks: beyond rowgram's rows
    m = fit(ctx, X, n_fft=32, n_modes=2)
    with pytest.raises(NotImplementedError):
        m.transform(array(X))
    with pytest.raises(NotImplementedError):
        m.inverse_transform(m.scores())
