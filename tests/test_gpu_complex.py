"""GPU parity tests of the complex / Hilbert path against the oracle.

Tolerances: Hilbert transform 2e-5 of the field scale (float32 transform vs the float64 oracle; the one-kernel
route of eofx_hfft.hpp measures 2-4e-7, asserted at 2e-6 in test_hilbert_every_plan); complex singular values rel 1e-5; vectors compared through |<v, v_ref>| >= 1 - 1e-5 because
a complex singular vector is defined up to a unit phase (the reference's LOBPCG result too)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eof_oracle as orc  # noqa: E402


def _waves(n, p, seed=0, noise=0.3):
    """travelling waves + noise: a field whose analytic signal has genuinely complex modes"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = (3.0 * np.cos(0.21 * t - 2 * x) + 1.7 * np.cos(0.37 * t + 3 * x + 0.4) + 0.9 * np.sin(0.11 * t - x)
         + 0.01 * t + noise * rng.standard_normal((n, p)))
    return X.astype(np.float32)


@pytest.mark.parametrize("n,p", [(200, 700), (151, 333)])
@pytest.mark.parametrize("padding", ["exp", None])
def test_hilbert_stage_vs_oracle(ctx, n, p, padding):
    from xeofs_amd import engine

    X = _waves(n, p, seed=n)
    mat, _ = engine.preprocess(ctx, X)
    Xc = mat.download().astype(np.float64)
    ref = orc.hilbert_transform(Xc, padding=padding, decay_factor=0.2)
    B, A2 = engine.hilbert(ctx, mat, padding, 0.2, want_real=True)
    scale = np.abs(ref).max()
    assert np.abs(B.download() - ref.imag).max() <= 2e-5 * scale
    assert np.abs(A2.download() - ref.real).max() <= 2e-5 * scale
    assert np.isclose(B.sumsq(), (ref.imag ** 2).sum(), rtol=1e-4)


@pytest.mark.parametrize("n,p", [(33, 9), (64, 130), (100, 65), (129, 8), (256, 33), (400, 21), (513, 4), (1000, 7),
                                 (1024, 2), (2000, 5), (2049, 3), (4000, 3), (4097, 2), (8000, 3), (8192, 1),
                                 (8193, 2), (10000, 3), (12001, 1), (16384, 2)])
@pytest.mark.parametrize("padding", ["exp", None])
def test_hilbert_every_plan(ctx, n, p, padding):
    """every instantiation of the one-kernel route (circular lengths 2^10 .. 2^14 with two features per transform: leading
    radix 4 / 8 / none / 2, two or three radix-16 stages, odd feature counts, series that end inside a wave; 2^15 with one
    feature per workgroup through the half-length transform of its even / odd samples) against the float64 oracle"""
    from xeofs_amd import engine

    rng = np.random.default_rng(n + p)
    X = (_waves(n, p, seed=n) + (0.002 * np.arange(n)[:, None] * rng.standard_normal(p)[None, :]).astype(np.float32)
         + rng.standard_normal(p).astype(np.float32)[None, :])            # trends and offsets: the pads matter
    dirty = engine.from_dense(ctx, np.full((n, p), 1.0e3, np.float32))   # same-shape buffers full of large values go back
    engine.hilbert(ctx, dirty, padding, 0.35, want_real=True)             # to the pool: whatever the stage leaves unwritten
    del dirty                                                             # in its padded outputs shows up below
    mat = engine.from_dense(ctx, X)                                       # not centred: the real part comes back centred
    ref = orc.hilbert_transform(X.astype(np.float64), padding=padding, decay_factor=0.35)
    ref = ref - ref.mean(axis=0)                                          # (hilbert_transform.py:40-72 centres both parts)
    B, A2 = engine.hilbert(ctx, mat, padding, 0.35, want_real=True)
    scale = np.abs(ref).max()
    assert np.abs(B.download() - ref.imag).max() <= 2e-6 * scale
    assert np.abs(A2.download() - ref.real).max() <= 2e-6 * scale
    assert np.isclose(B.sumsq(), (ref.imag ** 2).sum(), rtol=1e-5)        # (sum over the PADDED buffer: padding is zero)
    assert np.isclose(A2.sumsq(), (ref.real ** 2).sum(), rtol=1e-5)
    B2, none = engine.hilbert(ctx, mat, padding, 0.35)
    assert none is None and np.array_equal(B2.download(), B.download())   # run to run identical, with or without the real part
    import torch
    for m in (B, A2):                                                     # both layouts and the recorded absmax are usable
        D = m.download().astype(np.float64)
        Y = torch.zeros((m.p_pad, 32), device="cuda"); Y[:p] = torch.randn((p, 32), device="cuda")
        Z = torch.zeros((m.n_pad, 32), device="cuda"); Z[:n] = torch.randn((n, 32), device="cuda")
        for prec in ("f32", "f16x3"):
            got = engine.panel_mul(ctx, m, Y, prec=prec)[:n].double().cpu().numpy()
            want = D @ Y[:p].double().cpu().numpy()
            assert np.abs(got - want).max() <= 2e-5 * max(np.abs(want).max(), 1e-30), prec
            got = engine.panel_tmul(ctx, m, Z, prec=prec)[:p].double().cpu().numpy()
            want = D.T @ Z[:n].double().cpu().numpy()
            assert np.abs(got - want).max() <= 2e-5 * max(np.abs(want).max(), 1e-30), prec


def test_hilbert_long_series_route(ctx):
    """series longer than 16384 samples (circular length 2^16) take the hipFFT route; same contract"""
    from xeofs_amd import engine

    n, p = 16500, 12
    X = _waves(n, p, seed=4)
    mat, _ = engine.preprocess(ctx, X)
    ref = orc.hilbert_transform(mat.download().astype(np.float64), padding="exp", decay_factor=0.2)
    B, _ = engine.hilbert(ctx, mat, "exp", 0.2)
    assert np.abs(B.download() - ref.imag).max() <= 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize("n,p,k", [(300, 1200, 6), (900, 250, 4)])
def test_complex_rsvd_vs_exact(ctx, n, p, k):
    from xeofs_amd import engine
    from xeofs_amd.complex_svd import complex_rsvd

    rng = np.random.default_rng(5)
    r = 6
    amp = 8.0 * 0.6 ** np.arange(r)
    L = (rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r))) * amp
    R = rng.standard_normal((r, p)) + 1j * rng.standard_normal((r, p))
    Z = L @ R / np.sqrt(r) + 0.2 * (rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p)))
    Z = Z - Z.mean(axis=0)
    A = engine.from_dense(ctx, np.ascontiguousarray(Z.real, dtype=np.float32))
    B = engine.from_dense(ctx, np.ascontiguousarray(Z.imag, dtype=np.float32))
    U, s, V = complex_rsvd(ctx, A, B, k, random_state=3)
    Ue, se, Vhe = np.linalg.svd(Z, full_matrices=False)
    assert np.all(np.abs(s - se[:k]) <= 1e-5 * se[:k] + 2e-6 * se[0]), (s, se[:k])
    for j in range(k):
        assert abs(np.vdot(Vhe[j].conj(), V[:, j])) >= 1 - 1e-5, j      # V = conj(VT).T
        assert abs(np.vdot(Ue[:, j], U[:, j])) >= 1 - 1e-5, j
    rec = (U.astype(np.complex128) * s) @ V.astype(np.complex128).conj().T
    best = (Ue[:, :k] * se[:k]) @ Vhe[:k]
    assert np.linalg.norm(Z - rec) <= np.linalg.norm(Z - best) * (1 + 1e-4)
    assert np.abs(U.conj().T @ U - np.eye(k)).max() < 2e-5 and np.abs(V.conj().T @ V - np.eye(k)).max() < 2e-5
    # the returned vectors already satisfy the reference sign rule (xarray_utils.py:273-301)
    assert (orc.deterministic_sign_multiplier(V.conj().T) == 1).all()
    # against the reference's own complex solver (scipy svds lobpcg, decomposer.py:149-160)
    Uo, so, Vo = orc.decomposer_fit(Z, k, random_state=3, solver="randomized")
    assert np.all(np.abs(s - so) <= 1e-5 * so + 2e-6 * so[0])


@pytest.mark.parametrize("shape", [(220, 31, 17), (600, 12, 8)])      # Gram matrix on the sample / on the feature side
@pytest.mark.parametrize("n_modes", [60, 0.9])
def test_complex_eof_many_or_variance_based_modes(ctx, n_modes, shape):
    """more modes than the 64-column complex sketch holds, and a variance-based (float) n_modes -- int(0.3 rank) modes,
    truncated at the requested explained variance (decomposer.py:89-106, _svd.py:215-241) -- against the exact SVD"""
    import xeofs_amd as xe

    n, p = shape[0], shape[1] * shape[2]
    rng = np.random.default_rng(3)
    r = 90
    Z = ((rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r))) * (5.0 * 0.93 ** np.arange(r))) @ \
        (rng.standard_normal((r, p)) + 1j * rng.standard_normal((r, p))) / np.sqrt(r)
    Z = Z + 0.05 * (rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p)))
    da = xe.DataArray(Z.reshape(shape), dims=("time", "y", "x"))
    m = xe.single.ComplexEOF(n_modes=n_modes, random_state=1).fit(da, "time")
    Zc = Z - Z.mean(axis=0)
    Ue, se, Vhe = np.linalg.svd(Zc, full_matrices=False)
    if isinstance(n_modes, float):
        n_pre = int(0.3 * min(n, p))
        tv = (np.abs(Zc) ** 2).sum() / (n - 1)
        cum = np.cumsum(se[:n_pre] ** 2 / (n - 1) / tv)
        k = n_pre - int((cum >= n_modes).sum()) + 1
        assert 1 < k < n_pre
    else:
        k = n_modes
    s = m.singular_values().values
    assert s.shape == (k,)
    assert np.all(np.abs(s - se[:k]) <= 2e-5 * se[0])
    V = m.components().values.reshape(k, -1).T
    U = m.scores(normalized=True).values.reshape(k, -1).T
    for j in (0, 1, k // 2, k - 1):
        assert abs(np.vdot(Vhe[j].conj(), V[:, j])) / np.linalg.norm(V[:, j]) >= 1 - 1e-4, j
        assert abs(np.vdot(Ue[:, j], U[:, j])) / np.linalg.norm(U[:, j]) >= 1 - 1e-4, j
    assert (orc.deterministic_sign_multiplier(V.conj().T) == 1).all()
    # U s V^H reproduces the rank-k truncation (phases of U and V are consistent)
    rec = (U * s) @ V.conj().T
    best = (Ue[:, :k] * se[:k]) @ Vhe[:k]
    assert np.linalg.norm(rec - best) <= 1e-3 * np.linalg.norm(best)


def test_hilbert_eof_model_vs_oracle(ctx):
    import xeofs_amd as xe

    n, nlat, nlon, k = 240, 6, 40, 4
    X = _waves(n, nlat * nlon, seed=2).reshape(n, nlat, nlon)
    da = xe.DataArray(X, dims=("time", "lat", "lon"))
    m = xe.single.HilbertEOF(n_modes=k, padding="exp", decay_factor=0.2, random_state=1).fit(da, "time")
    Xc = X.reshape(n, -1).astype(np.float64)
    Xc = Xc - Xc.mean(axis=0)
    Zo = orc.hilbert_transform(Xc, "exp", 0.2)
    se = np.linalg.svd(Zo, compute_uv=False)[:k]
    s = m.singular_values().values
    assert np.all(np.abs(s - se) <= 2e-5 * se[0]), (s, se)
    tv = orc.total_variance(Zo)
    assert abs(m.data["total_variance"] - tv.real) <= 1e-4 * tv.real
    assert m.explained_variance_ratio().values.sum() <= 1 + 1e-5
    comps, scores = m.components(), m.scores()
    assert comps.dims == ("mode", "lat", "lon") and np.iscomplexobj(comps.values)
    assert scores.dims == ("mode", "time") and np.iscomplexobj(scores.values)
    amp, ph = m.components_amplitude(), m.components_phase()
    assert np.allclose(amp.values, np.abs(comps.values)) and np.allclose(ph.values, np.angle(comps.values))
    assert (m.scores_amplitude().values >= 0).all() and np.abs(m.scores_phase().values).max() <= np.pi + 1e-6
    # rank-k reconstruction of the analytic signal is as good as the exact truncated SVD's
    rec = scores.values.T @ comps.values.reshape(k, -1).conj()
    Ue, see, Vhe = np.linalg.svd(Zo, full_matrices=False)
    best = (Ue[:, :k] * see[:k]) @ Vhe[:k]
    assert np.linalg.norm(Zo - rec) <= np.linalg.norm(Zo - best) * (1 + 1e-3)


def test_complex_eof_on_reference_fixture(ctx):
    """reference tests/conftest.py:286-308 `mock_complex_data_array` (rank-2 travelling waves)"""
    import xeofs_amd as xe

    x = np.linspace(-5, 5, 128)
    t = np.linspace(0, 4 * np.pi, 256)
    Z = (1.0 / np.cosh(x[None, :] + 3) * np.exp(2.3j * t[:, None])
         + 2.0 / np.cosh(x[None, :]) * np.tanh(x) * np.exp(2.8j * t[:, None]))
    da = xe.DataArray(Z, dims=("time", "x"), coords={"time": t, "x": x})
    m = xe.single.ComplexEOF(n_modes=2, random_state=0).fit(da, "time")
    Zc = Z - Z.mean(axis=0)
    se = np.linalg.svd(Zc, compute_uv=False)[:2]
    assert np.allclose(m.singular_values().values, se, rtol=1e-5)
    rec = m.scores().values.T @ m.components().values.conj()
    assert np.abs(rec - Zc).max() <= 2e-4 * np.abs(Zc).max()      # two modes carry all of it
    assert np.isclose(m.explained_variance_ratio().values.sum(), 1.0, atol=1e-4)


def test_complex_inverse_transform_roundtrip(ctx):
    """eof.py:134-156 with complex scores / components: inverse_transform(scores) = scores . conj(V)^T un-scaled with the
    (complex) mean -- the rank-2 fixture is reproduced exactly; HilbertEOF returns the real part (eof.py:564-567);
    a scalar mode is expanded (base_model_single_set.py:276-277); the real EOFRotator refuses complex models (ComplexEOFRotator / HilbertEOFRotator rotate them)."""
    import xeofs_amd as xe

    x = np.linspace(-5, 5, 128)
    t = np.linspace(0, 4 * np.pi, 256)
    Z = (1.0 / np.cosh(x[None, :] + 3) * np.exp(2.3j * t[:, None])
         + 2.0 / np.cosh(x[None, :]) * np.tanh(x) * np.exp(2.8j * t[:, None])) + (0.3 - 0.2j)
    da = xe.DataArray(Z, dims=("time", "x"), coords={"time": t, "x": x})
    m = xe.single.ComplexEOF(n_modes=2, random_state=0).fit(da, "time")
    rec = m.inverse_transform(m.scores())
    assert rec.dims == ("time", "x") and np.iscomplexobj(rec.values)
    assert np.abs(rec.values - Z).max() <= 3e-4 * np.abs(Z).max()
    # oracle of the formula itself, mode by mode: Re(S) Re(V)^T + Im(S) Im(V)^T etc.
    S, V = m.scores().values.T, m.components().values.T          # (n, k), (p, k)
    want = S @ V.conj().T + Z.mean(axis=0)
    assert np.abs(rec.values - want).max() <= 2e-5 * np.abs(want).max()
    sc = m.scores()
    one = xe.DataArray(sc.values[1], dims=("time",), coords={"time": t, "mode": 2})
    r1 = m.inverse_transform(one)
    want1 = np.outer(S[:, 1], V[:, 1].conj()) + Z.mean(axis=0)
    assert np.abs(r1.values - want1).max() <= 2e-5 * np.abs(want1).max()

    n, nlat, nlon, k = 240, 6, 40, 4
    X = _waves(n, nlat * nlon, seed=2).reshape(n, nlat, nlon)
    dh = xe.DataArray(X, dims=("time", "lat", "lon"))
    h = xe.single.HilbertEOF(n_modes=k, random_state=1).fit(dh, "time")
    rh = h.inverse_transform(h.scores())
    assert rh.dims == ("time", "lat", "lon") and not np.iscomplexobj(rh.values)
    Sh, Vh = h.scores().values.T, h.components().values.reshape(k, -1).T
    wanth = (Sh @ Vh.conj().T).real + X.reshape(n, -1).mean(axis=0)
    assert np.abs(rh.values.reshape(n, -1) - wanth).max() <= 2e-5 * np.abs(wanth).max()
    with pytest.raises(TypeError, match="ComplexEOFRotator"):      # the real rotator refuses; the complex one rotates
        xe.single.EOFRotator(n_modes=2).fit(m)


@pytest.mark.parametrize("n,p,k,prec", [(300, 1200, 6, "f16x3"), (900, 250, 4, "f16x3"), (700, 3000, 40, "f16x3"),
                                        (2100, 600, 33, "f16x3"), (300, 1200, 6, "f32"), (64, 5000, 30, "f16x3")])
def test_engine_complex_rsvd_vs_exact(ctx, n, p, k, prec):
    """`eofx_rsvd_c64` (the complex decomposer entry: one two-matrix launch per pass, Hermitian Cholesky-QR on the host)
    against the exact complex SVD: singular values 1e-5, vectors up to a unit phase, reconstruction, orthonormality,
    the reference's sign rule; sketches up to 64 complex columns (k = 40 with 10 oversamples = 50); the exact-f32
    passes go through two launches + recombination; bitwise reproducible."""
    from xeofs_amd import engine

    rng = np.random.default_rng(5)
    r = max(6, k)
    amp = 8.0 * 0.85 ** np.arange(r)
    L = (rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r))) * amp
    R = rng.standard_normal((r, p)) + 1j * rng.standard_normal((r, p))
    Z = L @ R / np.sqrt(r) + 0.02 * (rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p)))
    Z = Z - Z.mean(axis=0)
    A = engine.from_dense(ctx, np.ascontiguousarray(Z.real, dtype=np.float32))
    B = engine.from_dense(ctx, np.ascontiguousarray(Z.imag, dtype=np.float32))
    ctx.set_precision(prec, prec)
    try:
        U, s, V = engine.rsvd_c64(ctx, A, B, k, random_state=3)
        U2, s2, V2 = engine.rsvd_c64(ctx, A, B, k, random_state=3, device_out=True)    # outputs left in HBM
    finally:
        ctx.set_precision("f16x3", "f16x3")
    assert np.array_equal(s, s2) and np.array_equal(U, U2.cpu().numpy()) and np.array_equal(V, V2.cpu().numpy())
    Ue, se, Vhe = np.linalg.svd(Z, full_matrices=False)
    assert np.all(np.abs(s - se[:k]) <= 1e-5 * se[:k] + 2e-6 * se[0]), (s, se[:k])
    gaps = np.minimum(np.abs(np.diff(se[:k + 1])), np.r_[np.inf, np.abs(np.diff(se[:k]))]) / se[:k]
    for j in range(k):
        if gaps[j] > 1e-2:
            assert abs(np.vdot(Vhe[j].conj(), V[:, j])) >= 1 - 1e-5, j      # V = conj(VT).T
            assert abs(np.vdot(Ue[:, j], U[:, j])) >= 1 - 1e-5, j
    rec = (U.astype(np.complex128) * s) @ V.astype(np.complex128).conj().T
    best = (Ue[:, :k] * se[:k]) @ Vhe[:k]
    assert np.linalg.norm(Z - rec) <= np.linalg.norm(Z - best) * (1 + 1e-4)
    assert np.abs(U.conj().T @ U - np.eye(k)).max() < 2e-5 and np.abs(V.conj().T @ V - np.eye(k)).max() < 2e-5
    assert (orc.deterministic_sign_multiplier(V.conj().T) == 1).all()
    if prec == "f16x3":
        # the panel-level driver (the feature-sharded path's single-rank form; 33 .. 64 columns: 128-wide real panels)
        from xeofs_amd.complex_svd import complex_rsvd

        Up, sp, Vp = complex_rsvd(ctx, A, B, k, random_state=3)
        assert np.all(np.abs(sp - se[:k]) <= 1e-5 * se[:k] + 2e-6 * se[0]), (sp, se[:k])
        recp = (Up.astype(np.complex128) * sp) @ Vp.astype(np.complex128).conj().T
        assert np.linalg.norm(Z - recp) <= np.linalg.norm(Z - best) * (1 + 1e-4)
        assert (orc.deterministic_sign_multiplier(Vp.conj().T) == 1).all()
    A.free(); B.free()


@pytest.mark.parametrize("n,p,k,both_in_place", [(300, 1536, 6, False), (1000, 700, 12, False), (260, 2500, 20, True),
                                                  (640, 1024, 5, True)])
def test_complex_rsvd_lean_layout(ctx, n, p, k, both_in_place):
    """The lean layout of the complex path: Re = the raw field in place (Scaler map on the fly),
    Im = the output of the Hilbert stage in its sample-contiguous layout only (or: both parts of a complex input in
    place).  `eofx_rsvd_c64` then streams every part in a layout it has (atb_f16 / axb_f16 + cpanel_combine) instead of
    the two-matrix launch over four written layouts.  Checked against the exact complex SVD of the same analytic
    signal, against the written-layout path (same sketch), and that no layout got written on the way."""
    from xeofs_amd import engine

    rng = np.random.default_rng(7 * n + k)
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = 0.002 * rng.standard_normal((n, p))
    for j in range(k + 4):          # k + 4 travelling waves with geometrically decaying amplitudes: every tested mode is signal
        X += 6.0 * 0.85 ** j * np.cos((0.05 + 0.043 * j) * t - (1 + j % 7) * x + 0.3 * j)
    X = (X + 3.0 + 0.5 * rng.standard_normal(p)).astype(np.float32)              # uncentred: the Scaler map centres
    om = engine.sketch_matrix(min(n, p), k + 10, 3)
    if both_in_place:
        Y = np.ascontiguousarray(np.roll(X, 7, axis=0) * 0.7 + 1.0, dtype=np.float32)
        A, _ = engine.preprocess(ctx, X, in_place=True)
        B, _ = engine.preprocess(ctx, Y, in_place=True)
        Aw, _ = engine.preprocess(ctx, X)
        Bw, _ = engine.preprocess(ctx, Y)
    else:
        A, _ = engine.preprocess(ctx, X, in_place=True)
        assert A.layout() == (False, True) and not A.has_sample_layout()
        B, _ = engine.hilbert(ctx, A, "exp", 0.2)
        assert not A.has_sample_layout()                       # built for the kernel only
        assert B.layout()[0] is False and B.has_sample_layout()
        Aw, _ = engine.preprocess(ctx, X)
        Bw, _ = engine.hilbert(ctx, Aw, "exp", 0.2)
        assert Bw.layout()[0] is True
    U, s, V = engine.rsvd_c64(ctx, A, B, k, omega=om)
    assert A.layout() == (False, True) and B.layout()[0] is False        # nothing was written for the passes
    if not both_in_place:
        assert not A.has_sample_layout()
    Uw, sw, Vw = engine.rsvd_c64(ctx, Aw, Bw, k, omega=om)
    U2, s2, V2 = engine.rsvd_c64(ctx, A, B, k, omega=om)
    assert np.array_equal(s, s2) and np.array_equal(V, V2) and np.array_equal(U, U2)     # bitwise reproducible
    Z = Aw.download().astype(np.float64) + 1j * Bw.download().astype(np.float64)
    Ue, se, Vhe = np.linalg.svd(Z, full_matrices=False)
    assert np.all(np.abs(s - se[:k]) <= 1e-5 * se[:k] + 2e-6 * se[0]), (s, se[:k])
    assert np.all(np.abs(s - sw) <= 2e-6 * se[0])
    gaps = np.minimum(np.abs(np.diff(se[:k + 1])), np.r_[np.inf, np.abs(np.diff(se[:k]))]) / se[:k]
    for j in range(k):
        if gaps[j] > 1e-2 and se[j] > 1e-3 * se[0]:
            assert abs(np.vdot(Vhe[j].conj(), V[:, j])) >= 1 - 1e-5, j
            assert abs(np.vdot(Ue[:, j], U[:, j])) >= 1 - 1e-5, j
    assert np.abs(U.conj().T @ U - np.eye(k)).max() < 2e-5 and np.abs(V.conj().T @ V - np.eye(k)).max() < 2e-5
    assert (orc.deterministic_sign_multiplier(V.conj().T) == 1).all()
    # the panel-level driver (eofx_cmat_mul_f32) takes the same lean route
    from xeofs_amd.complex_svd import complex_rsvd

    Up, sp, Vp = complex_rsvd(ctx, A, B, k, random_state=3)
    assert np.all(np.abs(sp - se[:k]) <= 1e-5 * se[:k] + 2e-6 * se[0])
    assert A.layout() == (False, True) and B.layout()[0] is False
    # consumers that want another layout of Im get it on demand
    E = np.zeros((p, 2), np.float32); E[0, 0] = E[p - 1, 1] = 1.0
    assert np.allclose(engine.project(ctx, B, E), Bw.download()[:, [0, p - 1]], atol=1e-5 * np.abs(Z.imag).max())
    assert np.allclose(B.download(), Bw.download(), atol=1e-6 * np.abs(Z.imag).max())
    for m in (A, B, Aw, Bw):
        m.free()


def test_complex_eof_standardize(ctx):
    """`ComplexEOF(standardize=True)` -- the reference's own docstring example (xeofs/single/eof.py:298): the Scaler
    divides the complex field by numpy's (real) std of a complex array, sqrt(var Re + var Im) (scaler.py:105-108)."""
    import xeofs_amd as xe

    rng = np.random.default_rng(3)
    n, p, k = 200, 90, 3
    amp = np.array([6.0, 3.0, 1.5])
    Z = ((rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))) * amp) @ (
        rng.standard_normal((3, p)) + 1j * rng.standard_normal((3, p)))
    Z = Z * np.linspace(0.5, 4.0, p) + 0.1 * (rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p))) + (2 - 1j)
    da = xe.DataArray(Z, dims=("time", "x"))
    m = xe.single.ComplexEOF(n_modes=k, standardize=True, random_state=0).fit(da, "time")
    Zs = (Z - Z.mean(axis=0)) / Z.std(axis=0)
    se = np.linalg.svd(Zs, compute_uv=False)[:k]
    assert np.allclose(m.singular_values().values, se, rtol=2e-5)
    assert abs(m.data["total_variance"] - (np.abs(Zs) ** 2).sum() / (n - 1)) <= 1e-5 * p
    rec = m.inverse_transform(m.scores())             # back in the original units: un-scaled with the same deviation
    Ue, see, Vhe = np.linalg.svd(Zs, full_matrices=False)
    best = ((Ue[:, :k] * see[:k]) @ Vhe[:k]) * Z.std(axis=0) + Z.mean(axis=0)
    assert np.abs(rec.values - best).max() <= 5e-4 * np.abs(Z).max()


def _bulk_field(n, p, seed, nsig=4, noise=1.0):
    """a few travelling waves over a flat noise bulk: most of the wanted modes are noise modes at the edge of the bulk --
    the case a fixed number of plain power iterations does not resolve and a Krylov-class solver (the reference's
    svds(lobpcg), decomposer.py:149-160) does"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = noise * rng.standard_normal((n, p))
    for j in range(nsig):
        X += 4.0 * 0.7 ** j * np.cos((0.07 + 0.05 * j) * t - (1 + j) * x + 0.3 * j)
    return (X + 3.0 + rng.standard_normal(p)).astype(np.float32)


def _analytic(X):
    pre = orc.preprocess(X.astype(np.float64), True, False, None)
    return pre["X"] + 1j * orc.hilbert_transform(pre["X"], padding="exp", decay_factor=0.2).imag


def _decay_field(n, p, seed, noise, nsig=26):
    """a geometric ladder of travelling waves (distinct wavenumbers: one complex mode each) that runs INTO the noise bulk around
    the k-th mode, s_k / s_{k+11} = 1.2 .. 1.3 -- the kind of spectrum the bench's config-5 gate sample has (1.18)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = noise * rng.standard_normal((n, p))
    for j in range(nsig):
        X += 5.0 * 0.88 ** j * np.cos((0.05 + 0.031 * j) * t - (1 + j) * x + 0.3 * j)
    return (X - 7.0 + rng.standard_normal(p)).astype(np.float32)


def _run_c64(ctx, X, k, n_iter="auto"):
    from xeofs_amd import engine

    A, _ = engine.preprocess(ctx, X, True, False, None, in_place=True)
    B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    U, s, V = engine.rsvd_c64(ctx, A, B, k, random_state=5, n_iter=n_iter)
    its = engine.last_iterations(ctx)
    A.free(); B.free()
    return U, s.astype(np.float64), V, its


def _reference_solver_error(Z, k, se):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (lobpcg reports the modes it leaves unconverged after its 20 iterations)
        _, sl, _ = orc.complex_svds(Z, k, random_state=5)
    return np.abs(sl - se[:k]) / se[:k]


@pytest.mark.parametrize("n,p,k,noise", [(900, 1600, 20, 6.5), (1500, 700, 20, 6.5), (500, 3000, 14, 12.0)])
def test_complex_rsvd_default_rule_vs_reference_solver_and_exact(ctx, n, p, k, noise, monkeypatch):
    """Row R9 with the DEFAULT rule (scikit-learn's count of products; block Krylov + Rayleigh-Ritz since round 5) on a spectrum
    that runs into its noise bulk: against the exact complex SVD and against the reference's own solver (scipy svds(lobpcg),
    decomposer.py:149-160) on the same matrix -- per mode |s - s_exact| / s_exact <= max(1e-5, the reference solver's error);
    subspaces of the gap-separated modes to 1 - 1e-5; reconstruction within 1 + 1e-4 of the best rank-k one.  The subspace
    iteration of rounds 1-4 (EOFX_C64_KRYLOV=0), run beside it, misses the tolerance -- the reason the rule changed."""
    X = _decay_field(n, p, n + k, noise)
    Z = _analytic(X)
    Ue, se, Vhe = np.linalg.svd(Z, full_matrices=False)
    e_ref = _reference_solver_error(Z, k, se)
    U, s, V, its = _run_c64(ctx, X, k)
    assert its == 7
    e = np.abs(s - se[:k]) / se[:k]
    assert np.all(e <= np.maximum(1e-5, e_ref) + 4e-7), (e, e_ref)          # (+ the float32 rounding of the returned values)
    assert np.abs(U.conj().T @ U - np.eye(k)).max() < 2e-5 and np.abs(V.conj().T @ V - np.eye(k)).max() < 2e-5
    for j in range(k):
        gap = min(se[j - 1] - se[j] if j else np.inf, se[j] - se[j + 1]) / se[j]
        if gap > 2e-2:
            assert abs(np.vdot(Vhe[j].conj(), V[:, j])) >= 1 - 1e-5, j
    rec = (U.astype(np.complex128) * s) @ V.astype(np.complex128).conj().T
    best = (Ue[:, :k] * se[:k]) @ Vhe[:k]
    assert np.linalg.norm(Z - rec) <= np.linalg.norm(Z - best) * (1 + 1e-4)
    monkeypatch.setenv("EOFX_C64_KRYLOV", "0")
    _, s_old, _, _ = _run_c64(ctx, X, k)
    e_old = np.abs(s_old - se[:k]) / se[:k]
    assert e_old.max() > 1e-5 and e_old.max() > 10 * e.max(), (e_old.max(), e.max())


@pytest.mark.parametrize("n,p,k", [(900, 1600, 20), (1500, 700, 20), (400, 3000, 12)])
def test_complex_rsvd_flat_bulk_vs_reference_solver_and_exact(ctx, n, p, k, monkeypatch):
    """Row R9 at its hardest: all but four of the k wanted modes are noise modes at the edge of a flat bulk.  The reference's
    lobpcg spends its full 20 iterations there; the engine's "converge" rule (block Lanczos with thick restarts until the
    residual of every wanted Ritz pair is below 1e-5 of its value, at most 20 products) must be as accurate per mode:
    |s - s_exact| / s_exact <= max(1e-5, the reference solver's error).  The default rule (7 products) is an order of
    magnitude or more ahead of the subspace iteration it replaced at the same number of passes."""
    X = _bulk_field(n, p, seed=n + k)
    Z = _analytic(X)
    se = np.linalg.svd(Z, compute_uv=False)
    e_ref = _reference_solver_error(Z, k, se)
    U, s, V, its = _run_c64(ctx, X, k, "converge")
    assert 7 <= its <= 20
    e = np.abs(s - se[:k]) / se[:k]
    assert np.all(e <= np.maximum(1e-5, e_ref) + 4e-7), (its, e, e_ref)
    assert np.abs(U.conj().T @ U - np.eye(k)).max() < 2e-5 and np.abs(V.conj().T @ V - np.eye(k)).max() < 2e-5
    _, s7, _, its7 = _run_c64(ctx, X, k)
    e7 = np.abs(s7 - se[:k]) / se[:k]
    assert its7 == 7 and e7.max() <= 2e-3, e7
    monkeypatch.setenv("EOFX_C64_KRYLOV", "0")
    _, s_old, _, _ = _run_c64(ctx, X, k)
    e_old = np.abs(s_old - se[:k]) / se[:k]
    assert e_old.max() > 10 * e7.max(), (e_old.max(), e7.max())


@pytest.mark.parametrize("case", ["wide_sketch", "full_width", "rank_deficient", "n_iter_1", "n_iter_2", "converge", "feature_side",
                                  "thick_restart"])
def test_complex_rsvd_krylov_edge_cases(ctx, case):
    """The block Lanczos recurrence where it ends early or runs in another shape: a sketch wider than 32 complex columns
    (128-column real panels), a full-width sketch (identity start: the first product exhausts the space), an exactly
    rank-deficient matrix (blocks die), one and two products, restarted cycles ("converge"), the sketch on the feature
    side (n > p), and a sketch of 52 columns at seven products, whose eighth block would take the Rayleigh-Ritz problem past
    order 384 (one thick restart) -- values against the exact SVD for every mode clear of the bulk."""
    from xeofs_amd import engine

    rng = np.random.default_rng(11)
    n, p, k, n_iter, noise = 300, 900, 6, "auto", 0.02
    if case == "wide_sketch":
        n, p, k = 60, 400, 28             # l = 38 -> LP = 128, k >= 0.1 rank -> 4 products, Krylov order 190
    elif case == "full_width":
        n, p, k = 24, 300, 14             # l = 24 = rank
    elif case == "n_iter_1":
        n_iter = 1
    elif case == "n_iter_2":
        n_iter = 2
    elif case == "converge":
        n_iter, noise = "converge", 0.3
    elif case == "feature_side":
        n, p = 900, 260
    elif case == "thick_restart":
        n, p, k, n_iter = 400, 600, 42, 7   # l = 52: 7 blocks fit below order 384, the sample side holds them (7 * 52 <= 400)
    r = 5 if case == "rank_deficient" else 9
    L = (rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r))) * (6.0 * 0.6 ** np.arange(r))
    Z = L @ (rng.standard_normal((r, p)) + 1j * rng.standard_normal((r, p))) / np.sqrt(p)
    if case != "rank_deficient":
        Z = Z + noise * (rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p))) / np.sqrt(p)
    Z = Z.astype(np.complex64)
    A = engine.from_dense(ctx, np.ascontiguousarray(Z.real))
    B = engine.from_dense(ctx, np.ascontiguousarray(Z.imag))
    U, s, V = engine.rsvd_c64(ctx, A, B, k, random_state=2, n_iter=n_iter)
    A.free(); B.free()
    se = np.linalg.svd(Z.astype(np.complex128), compute_uv=False)
    tol = {"n_iter_1": 2e-3, "n_iter_2": 1e-4}.get(case, 1e-5)
    kk = min(k, r) if case == "rank_deficient" else k
    clear = se[:kk] > (1.0 if case in ("full_width", "wide_sketch", "rank_deficient") else 3.0) * se[min(k + 10, len(se) - 1)]
    assert clear.sum() >= min(kk, 5)
    assert np.all(np.abs(s[:kk] - se[:kk])[clear] <= tol * se[:kk][clear] + 2e-6 * se[0]), (case, s, se[:k])
    if case == "rank_deficient":
        assert np.all(s[kk:] <= 1e-5 * se[0])
    good = s > 1e-5 * se[0]
    Ug, Vg = U[:, good], V[:, good]
    assert np.abs(Ug.conj().T @ Ug - np.eye(good.sum())).max() < 3e-5 and np.abs(Vg.conj().T @ Vg - np.eye(good.sum())).max() < 3e-5
    rec = (Ug.astype(np.complex128) * s[good]) @ Vg.astype(np.complex128).conj().T
    if case not in ("n_iter_1", "n_iter_2"):
        tail = np.sqrt((se[int(good.sum()):] ** 2).sum())
        assert np.linalg.norm(Z - rec) <= tail * (1 + 1e-3) + 1e-5 * se[0]


@pytest.mark.parametrize("n,p", [(200, 700), (333, 1028), (1000, 260), (4100, 96), (8000, 64)])
@pytest.mark.parametrize("std,use_w", [(False, False), (True, True)])
def test_hilbert_reads_the_raw_layout_of_the_statistics_pass(ctx, n, p, std, use_w):
    """Round 5: with `for_hilbert=True` the statistics pass of the in-place preprocess writes the raw field in the
    sample-contiguous layout on its way (colstats4_tr_kernel) and the Hilbert kernel applies the Scaler map on load -- the
    transposing copy of the stage disappears.  Same statistics, and the imaginary part is BIT-IDENTICAL to the route that
    builds the transient copy (the map is the same float32 expression); the buffer goes back to the pool."""
    from xeofs_amd import engine

    rng = np.random.default_rng(n + p)
    X = (_waves(n, p, seed=p) * rng.uniform(0.5, 2.0, size=p).astype(np.float32) + 250.0 + rng.standard_normal(p).astype(np.float32))
    w = rng.uniform(0.3, 1.5, size=p) if use_w else None
    A0, st0 = engine.preprocess(ctx, X, True, std, w, in_place=True)
    B0, _ = engine.hilbert(ctx, A0, "exp", 0.2)
    A1, st1 = engine.preprocess(ctx, X, True, std, w, in_place=True, for_hilbert=True)
    assert A1.layout() == A0.layout()
    B1, _ = engine.hilbert(ctx, A1, "exp", 0.2)
    assert np.allclose(st0["mean"], st1["mean"], rtol=1e-12, atol=0) and np.isclose(st0["total_variance"], st1["total_variance"], rtol=1e-9)   # (float64 sums in another order)
    b0, b1 = B0.download(), B1.download()
    if np.array_equal(st0["mean"], st1["mean"]) and (not std or np.array_equal(st0["std"], st1["std"])):
        assert np.array_equal(b0, b1)
    else:       # (the row splits of the statistics pass differ by a multiple of 32 rows: the last bit of a mean may)
        assert np.abs(b0 - b1).max() <= 2e-6 * np.abs(b0).max()
    ref = orc.preprocess(X.astype(np.float64), True, std, w)["X"]
    href = orc.hilbert_transform(ref, padding="exp", decay_factor=0.2).imag
    assert np.abs(b1 - href).max() <= 2e-5 * np.abs(href).max()
    # a second Hilbert call on the same matrix (buffer already consumed) takes the transient-copy route
    B2, _ = engine.hilbert(ctx, A1, "exp", 0.2)
    assert np.array_equal(B2.download(), b1) or np.abs(B2.download() - b1).max() <= 2e-6 * np.abs(b1).max()
    for m in (A0, B0, A1, B1, B2):
        m.free()


@pytest.mark.parametrize("for_hilbert", [False, True])
@pytest.mark.parametrize("n,P,k", [(300, 1600, 6), (520, 4096, 12)])
def test_masked_field_through_hilbert_and_complex_rsvd_in_place(ctx, n, P, k, for_hilbert):
    """VERDICT r04 item 7 (sanitizer.py:80-126 ahead of eof.py:546-555): a field with a 30 % land mask (all-NaN grid points)
    stays IN PLACE through the Hilbert stage and the complex decomposition -- zero columns in the real part (the MASK forms of
    the streaming kernels), zero columns in the written imaginary part, the sign rule over the valid features only -- and gives
    the factors of the compaction route (which writes the compacted matrix in both layouts: 3x the field) to 2e-6."""
    from xeofs_amd import engine

    rng = np.random.default_rng(P)
    X = _waves(n, P, seed=n, noise=0.2) + 11.0
    dead = rng.choice(P, size=int(0.3 * P), replace=False)
    X[:, dead] = np.nan
    w = rng.uniform(0.4, 1.3, size=P)
    A0, st0 = engine.preprocess(ctx, X, True, False, w)                         # compacted, written layouts
    assert not A0.masked and A0.p == P - dead.size
    B0, _ = engine.hilbert(ctx, A0, "exp", 0.2)
    U0, s0, V0 = engine.rsvd_c64(ctx, A0, B0, k, random_state=3)
    A1, st1 = engine.preprocess(ctx, X, True, False, w, in_place=True, allow_masked=True, for_hilbert=for_hilbert)
    assert A1.masked and A1.p == A0.p and A1.p_phys == P and A1.layout() == (False, True)
    B1, _ = engine.hilbert(ctx, A1, "exp", 0.2)
    assert B1.p == P and not B1.masked
    U1, s1, V1 = engine.rsvd_c64(ctx, A1, B1, k, random_state=3)
    assert A1.layout() == (False, True) and not B1.layout()[0]                   # nothing else was written
    b1 = B1.download()                                                           # (builds B1's other layout: after the check)
    assert not b1[:, dead].any()
    b0 = B0.download()
    assert np.abs(b1[:, np.setdiff1d(np.arange(P), dead)] - b0).max() <= 2e-6 * np.abs(b0).max()
    assert V1.shape == V0.shape == (A0.p, k)
    assert np.all(np.abs(s1 - s0) <= 2e-6 * s0[0])
    for j in range(k):
        if min(s0[j - 1] - s0[j] if j else np.inf, s0[j] - (s0[j + 1] if j + 1 < k else 0.0)) > 1e-3 * s0[0]:
            assert abs(np.vdot(V0[:, j], V1[:, j])) >= 1 - 1e-5, j        # (a complex mode is defined up to a unit phase)
            assert abs(np.vdot(U0[:, j], U1[:, j])) >= 1 - 1e-5, j
    assert (orc.deterministic_sign_multiplier(V1.conj().T) == 1).all()
    for m in (A0, B0, A1, B1):
        m.free()


def test_hilbert_eof_model_on_a_land_masked_field(ctx):
    """xe.single.HilbertEOF on a field with a land mask: the masked in-place route (round 5) against the compaction route of
    the same model, and against the oracle's analytic signal -- components carry NaN at the masked grid points either way."""
    import xeofs_amd as xe

    n, ny, nx, k = 260, 24, 50, 4
    rng = np.random.default_rng(5)
    X = (_waves(n, ny * nx, seed=3, noise=0.2) + 4.0).reshape(n, ny, nx)
    land = rng.random((ny, nx)) < 0.3
    X[:, land] = np.nan
    da = xe.DataArray(X, dims=("time", "lat", "lon"), coords={"lat": np.linspace(-60, 60, ny)})
    ms = []
    for masked_ok in (True, False):
        m = xe.single.HilbertEOF(n_modes=k, use_coslat=True, random_state=2, padding="exp")
        m.ctx = ctx
        m._hilbert_masked_ok = masked_ok
        m.fit(da, "time")
        assert m.data["input_data"][0].masked == masked_ok
        ms.append(m)
    s1, s0 = (np.asarray(m.singular_values().values, dtype=np.float64) for m in ms)
    assert np.all(np.abs(s1 - s0) <= 2e-6 * s0[0])
    c1, c0 = (np.asarray(m.components().values) for m in ms)
    assert c1.shape == c0.shape == (k, ny, nx)
    assert np.isnan(c1[:, land]).all() and not np.isnan(c1[:, ~land]).any()
    for j in range(k):
        a, b = c0[j][~land], c1[j][~land]
        assert abs(np.vdot(a, b)) >= (1 - 1e-5) * np.linalg.norm(a) * np.linalg.norm(b)
    # against the oracle: Scaler / Sanitizer restatement + Hilbert transform + exact complex SVD of the compacted matrix
    w = np.repeat(orc.sqrt_cos_lat_weights(np.linspace(-60, 60, ny)), nx)
    pre = orc.preprocess(X.reshape(n, -1).astype(np.float64), True, False, w)
    Z = pre["X"] + 1j * orc.hilbert_transform(pre["X"], padding="exp", decay_factor=0.2).imag
    se = np.linalg.svd(Z, compute_uv=False)[:k]
    assert np.all(np.abs(s1 - se) <= 1e-5 * se)


@pytest.mark.parametrize("route", ["two_part", "operator"])
def test_more_modes_than_numerical_rank_keeps_both_factors_orthonormal(ctx, route):
    """The analytic signal of a short series has about n / 2 + 1 independent rows: with n = 55 and k = 35 the trailing modes are
    numerically null (values 1e-7 ... 1e-9 of the leading one).  The reference's solver ends with a dense SVD of A V (scipy svds),
    so its factors are orthonormal whatever the values; the engine re-orthonormalises such columns of the small-side factor
    (found by tools/fuzz_complex.py, case 34 of the bulk sweep: U^H U - I was 0.24 there)."""
    from xeofs_amd import engine

    n, p, k = 55, 112, 35
    rng = np.random.default_rng(34)
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = 0.5 * rng.standard_normal((n, p))
    for j in range(11):
        X += 6.0 * 0.85 ** j * np.cos((0.05 + 0.043 * j) * t - (1 + j % 7) * x + 0.3 * j)
    X = (X + 20.0).astype(np.float32)
    A, _ = engine.preprocess(ctx, X, True, False, None, in_place=(route == "operator"))
    if route == "operator":
        U, s, V = engine.rsvd_hilbert_c64(ctx, A, k, "exp", 0.2, random_state=260, n_iter="converge")
    else:
        B, _ = engine.hilbert(ctx, A, "exp", 0.2)
        U, s, V = engine.rsvd_c64(ctx, A, B, k, random_state=260, n_iter="converge")
        B.free()
    A.free()
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    Z = orc.hilbert_transform(Xc, padding="exp", decay_factor=0.2)
    se = np.linalg.svd(Z, compute_uv=False)[:k]
    assert se[-1] < 1e-5 * se[0]                                  # (the case is what it claims to be)
    assert np.abs(U.conj().T @ U - np.eye(k)).max() < 3e-5
    assert np.abs(V.conj().T @ V - np.eye(k)).max() < 3e-5
    clear = se > 1e-3 * se[0]
    assert np.all(np.abs(s - se)[clear] <= 2e-5 * se[0])
    assert np.all(s[~clear] <= 2e-3 * se[0])


def test_bench_field_spectrum_converge_rule_vs_reference_solver_and_exact(ctx):
    """the config-5 FIELD of bench.py (its leading modes stand clear, modes 15-20 sit a per cent above a flat
    noise bulk) at a size the host follows in seconds, through tools/r9_evidence.py -- the analytic signal's exact singular values
    (float64 Gram + LAPACK), the REFERENCE'S solver scipy svds(lobpcg) (xeofs/linalg/decomposer.py:149-160) and the engine's
    operator route.  `n_iter="converge"` (the rule the Hilbert / complex models use since round 6) meets max(1e-5, the reference
    solver's own error) on EVERY mode; scikit-learn's count (`n_iter="auto"`, 7 products) is reported by the tool and does not
    on the modes next to the bulk (profiles/r06_r9_evidence*.txt: the full table at 8000 x 65 536)."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import r9_evidence

    out = r9_evidence.run(n=3000, nlat=64, nlon=256, k=20, ctx=ctx)
    assert all(out["converge_ok"]), [f"{e:.2e}" for e in out["err_converge"]]
    assert max(out["err_converge"]) <= 1e-5
    assert max(out["err_lobpcg"]) <= 1e-4                  # (the reference solver itself is a converged solver on this field)
    assert 2 <= out["converge_products"] <= 20
    # the leading, gap-separated modes are converged by either rule
    assert max(out["err_auto"][:8]) <= 1e-5
