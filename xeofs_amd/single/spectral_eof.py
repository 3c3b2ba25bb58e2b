"""xeofs_amd.single.SpectralEOF -- spectral EOF analysis [Schmidt, Mengaldo, Balsamo & Wedi 2019, Mon. Wea. Rev. 147, 2979-2995,
"Spectral empirical orthogonal function analysis of weather and climate data"], the same method as spectral proper orthogonal
decomposition [Towne, Schmidt & Colonius 2018, J. Fluid Mech. 847, 821-867]: a Welch estimate of the cross-spectral density
of the whole field and an eigen-decomposition of it at every frequency.  The modes at a frequency are the spatial patterns --
complex, so they can propagate -- that carry the most variance there.  The reference has no such model; the
definition is stated here in full.

With Xc [n x p] the engine's preprocessed float32 matrix of the fit (centred, weights applied; with center=False its centred
twin stands in for it, `EOF._centred_twin`, as in EOT), a window w [n_fft], fs = 1 / sampling_interval,

    hop   = n_fft - n_overlap
    nblk  = (n - n_overlap) // hop                            (block_count; trailing samples are dropped)
    nfreq = n_fft // 2 + 1,   f_k = k fs / n_fft              (frequency_axis)
    c_k   = 2 for interior frequencies, 1 for k = 0 and for the Nyquist frequency of an even n_fft   (one-sided density)
    s_k   = sqrt(c_k / (fs sum_t w_t^2))

the Fourier realisations of block b (coefficient_matrix: rows 2k and 2k + 1 of B are s_k w_t cos(2 pi k t / n_fft) and
-s_k w_t sin(2 pi k t / n_fft) in float64, rounded once to float32; with block_detrend, B is right-multiplied by
I - 1 1^T / n_fft first, which removes each block's own mean)

    Q_k[b, j] = s_k sum_t w_t e^{-2 pi i k t / n_fft} Xc[b hop + t, j]        (engine.mat_blockxform, csrc/eofx_spectral.hpp:
                                                                              float32 on the matrix cores, the overlapped
                                                                              blocks are never materialised)

and per frequency, with the method of snapshots (the p x p spectral density matrix S_k = Q_k^T conj(Q_k) / nblk never exists):

    M_k[b, b'] = sum_j conj(Q_k[b, j]) Q_k[b', j] / nblk      (engine.rowgram on [Re Q_k; Im Q_k] -> float64 G;
                                                               Re M = G_rr + G_ii, Im M = G_ri - G_ir: hermitian_from_gram)
    M_k Theta = Theta Lambda                                   (numpy.linalg.eigh in float64 on the host; lambda descending)
    Phi_k = Q_k^T Theta Lambda^{-1/2} / sqrt(nblk)             (engine.slabmul with W = [[Cr^T, -Ci^T], [Ci^T, Cr^T]],
                                                               C = Theta Lambda^{-1/2} / sqrt(nblk): mode_weights)
    a_k[m, b] = sqrt(nblk lambda_m) conj(Theta[b, m])         (= phi_m^H q_b, the expansion coefficient of block b)

The modes of a frequency are orthonormal, Phi^H Phi = I, and S_k Phi = Phi Lambda.  Phase gauge: every mode is
multiplied by the unit complex number that makes its entry of largest modulus real and positive (the lowest index among equal
moduli; torch on the device -- the complex family's rule works on [Re | Im] panels of one decomposition, not on a batch of
frequencies); the scores get the conjugate factor.  A mode with lambda_m <= nblk 2^-23 lambda_0 at its frequency is not
resolved by float32 realisations: it keeps its lambda, its component is NaN.

    frequencies()              f_k [nfreq]
    spectrum()                 lambda [nfreq x n_modes]: a power spectral density; sum_k sum_{all m} lambda fs / n_fft recovers
                               the variance of the blocked samples up to the window
    total_spectrum()           trace M_k [nfreq]
    explained_variance_ratio() lambda / trace, per frequency
    components()               complex, dims (frequency, mode, the input's feature dims); NaN at masked points
    components_amplitude(), components_phase()
    scores()                   complex a [frequency x mode x block]; the block coordinate is the centre sample of each block
    transform, inverse_transform   raise NotImplementedError

Q for all frequencies is 2 nfreq nblk p floats, about twice the field at the default overlap, so `fit` walks the frequencies
in chunks (chunk_schedule): freq_chunk=None takes at most a quarter of the free device memory (in whole tiles of 64
frequencies where that many fit), an integer forces the size.  The field is read once per chunk, Q is never kept, and the
results do not depend on the chunk size, bit for bit: every operator computes an element in one fixed order whatever the batch.

Out of scope: the sharded path, the bootstrapper, rotation, complex data.  Samples dropped by check_nans are closed up, as in
every model: the blocks are taken over the samples that remain.

The host steps are module-level functions that need no GPU: window_values, block_count, frequency_axis, coefficient_matrix,
hermitian_from_gram, mode_weights, chunk_schedule, auto_chunk, blockxform_plan, rowgram_plan.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled
from .eof import EOF

RANK_EPS = 2.0 ** -23
CHUNK_TILE = 64           # frequencies whose 128 coefficient rows fill one tile of blockxform


def window_values(window, n_fft: int) -> np.ndarray:
    """the window as float64 [n_fft]: "hamming", "hann" (both periodic, as scipy.signal.get_window gives them to welch),
    "boxcar", or an array of n_fft values"""
    n_fft = int(n_fft)
    if isinstance(window, str):
        t = np.arange(n_fft, dtype=np.float64)
        if window == "boxcar":
            w = np.ones(n_fft)
        elif window == "hann":
            w = 0.5 - 0.5 * np.cos(2.0 * np.pi * t / n_fft)
        elif window == "hamming":
            w = 0.54 - 0.46 * np.cos(2.0 * np.pi * t / n_fft)
        else:
            raise ValueError(f"window must be 'hamming', 'hann', 'boxcar' or an array of n_fft values, got {window!r}")
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.ndim != 1 or w.shape[0] != n_fft:
            raise ValueError(f"window must have n_fft = {n_fft} values, got shape {w.shape}")
        if not np.all(np.isfinite(w)):
            raise ValueError("window must be finite")
    if not np.sum(w * w) > 0.0:
        raise ValueError("window must have a sum of squares above zero")
    return w


def block_count(n: int, n_fft: int, n_overlap: int) -> int:
    """nblk = (n - n_overlap) // (n_fft - n_overlap)"""
    return (int(n) - int(n_overlap)) // (int(n_fft) - int(n_overlap))


def frequency_axis(n_fft: int, sampling_interval: float = 1.0) -> np.ndarray:
    """f_k = k fs / n_fft, k = 0 .. n_fft // 2"""
    return np.arange(int(n_fft) // 2 + 1, dtype=np.float64) / (float(sampling_interval) * int(n_fft))


def onesided_factors(n_fft: int) -> np.ndarray:
    """c_k: 2 for interior frequencies, 1 for k = 0 and for the Nyquist frequency of an even n_fft"""
    c = np.full(int(n_fft) // 2 + 1, 2.0)
    c[0] = 1.0
    if n_fft % 2 == 0:
        c[-1] = 1.0
    return c


def coefficient_matrix(n_fft: int, window, sampling_interval: float = 1.0, block_detrend: bool = False,
                       dtype=np.float32) -> np.ndarray:
    """B [2 nfreq x n_fft]: rows 2k, 2k + 1 = s_k w_t cos, -s_k w_t sin of 2 pi k t / n_fft (the angle from (k t) mod n_fft, so
    it is exact in the integers), in float64, times (I - 1 1^T / n_fft) with block_detrend, rounded once to `dtype`"""
    n_fft = int(n_fft)
    w = window_values(window, n_fft)
    fs = 1.0 / float(sampling_interval)
    s = np.sqrt(onesided_factors(n_fft) / (fs * np.sum(w * w)))
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
    t = np.arange(n_fft, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((k * t) % n_fft).astype(np.float64) / n_fft
    B = np.empty((2 * (n_fft // 2 + 1), n_fft), dtype=np.float64)
    B[0::2] = s[:, None] * w[None, :] * np.cos(ang)
    B[1::2] = -s[:, None] * w[None, :] * np.sin(ang)
    if block_detrend:
        B = B - B.sum(axis=1, keepdims=True) / n_fft
    return np.ascontiguousarray(B, dtype=dtype)


def hermitian_from_gram(G, nblk: int) -> np.ndarray:
    """M [.. x nblk x nblk] complex128 from G = [Re Q; Im Q] [Re Q; Im Q]^T [.. x 2 nblk x 2 nblk]:
    Re M = (G_rr + G_ii) / nblk, Im M = (G_ri - G_ir) / nblk"""
    G = np.asarray(G, dtype=np.float64)
    b = int(nblk)
    if G.shape[-1] != 2 * b or G.shape[-2] != 2 * b:
        raise ValueError(f"G must be [.. x {2 * b} x {2 * b}], got shape {G.shape}")
    rr, ri, ir, ii = G[..., :b, :b], G[..., :b, b:], G[..., b:, :b], G[..., b:, b:]
    return ((rr + ii) + 1j * (ri - ir)) / b


def eig_descending(M):
    """numpy.linalg.eigh of one Hermitian M: -> (lambda descending, Theta with the columns in that order)"""
    lam, Th = np.linalg.eigh(M)
    return lam[::-1].copy(), Th[:, ::-1].copy()


def resolved_modes(lam, nblk: int) -> np.ndarray:
    """the modes a float32 realisation resolves: lambda_m > nblk 2^-23 lambda_0 (and finite)"""
    lam = np.asarray(lam, dtype=np.float64)
    return np.isfinite(lam) & (lam > nblk * RANK_EPS * lam[..., :1])


def mode_weights(lam, Th, n_modes: int) -> np.ndarray:
    """W [2 n_modes x 2 nblk] float64 = [[Cr^T, -Ci^T], [Ci^T, Cr^T]], C = Theta Lambda^{-1/2} / sqrt(nblk) of the leading
    n_modes; the columns of an unresolved mode are zero"""
    b, K = Th.shape[0], int(n_modes)
    ok = resolved_modes(lam, b)[:K]
    C = np.zeros((b, K), dtype=np.complex128)
    C[:, ok] = Th[:, :K][:, ok] / np.sqrt(lam[:K][ok] * b)
    W = np.empty((2 * K, 2 * b), dtype=np.float64)
    W[:K, :b], W[:K, b:] = C.real.T, -C.imag.T
    W[K:, :b], W[K:, b:] = C.imag.T, C.real.T
    return W


def chunk_schedule(nfreq: int, freq_chunk: int):
    """[(k0, k1), ...]: the frequencies 0 .. nfreq - 1 in chunks of freq_chunk, ascending; the last may be shorter"""
    nfreq, fc = int(nfreq), int(freq_chunk)
    if fc < 1:
        raise ValueError(f"freq_chunk must be a positive integer or None, got {freq_chunk!r}")
    return [(k0, min(k0 + fc, nfreq)) for k0 in range(0, nfreq, fc)]


def auto_chunk(nfreq: int, nblk: int, p: int, n_modes: int, free_bytes: int) -> int:
    """the chunk `fit` takes for freq_chunk=None: the frequencies whose Q (2 nblk p floats each) and modes (2 n_modes p floats,
    twice: the product and its gauged copy) fit into a quarter of the free device memory; a multiple of CHUNK_TILE where
    that many fit; at least 1, at most min(nfreq, the slabs one call takes)"""
    per = 4 * (2 * int(nblk) + 6 * int(n_modes)) * max(int(p), 1)
    fc = int(free_bytes // 4 // per)
    if CHUNK_TILE <= fc < int(nfreq):
        fc -= fc % CHUNK_TILE
    return max(1, min(fc, int(nfreq), engine.SPECTRAL_NBMAX))


def blockxform_plan(p: int, ncoef: int, nblk: int):
    """(series tiles, coefficient tiles, block groups) of the blockxform grid: csrc/eofx_spectral.hpp restated"""
    stiles, ctiles = -(-int(p) // 128), -(-int(ncoef) // 128)
    g = -(-1024 // (max(stiles, 1) * max(ctiles, 1)))
    return stiles, ctiles, max(1, min(g, int(nblk), 65535))


def rowgram_plan(r: int, p: int, nb: int):
    """(row tiles, spans, splits) of the rowgram grid: csrc/eofx_spectral.hpp restated; the split does not depend on nb"""
    rt, spans = -(-int(r) // 128), -(-int(p) // engine.ROWGRAM_SPAN)
    return rt, spans, max(1, min(16 // max(rt * (rt + 1) // 2, 1), spans))


def gauge_factors(z) -> np.ndarray:
    """u = conj(z) / |z| for the pivots z (complex128); 1 where z is 0 or not finite"""
    z = np.asarray(z, dtype=np.complex128)
    a = np.abs(z)
    ok = np.isfinite(a) & (a > 0.0)
    u = np.ones(z.shape, dtype=np.complex128)
    u[ok] = np.conj(z[ok]) / a[ok]
    return u


def _check_int(name, v, lo, hi, what):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not (lo <= v <= hi):
        raise ValueError(f"{name} must be an integer {what}, got {v!r}")
    return int(v)


class SpectralEOF(EOF):
    """Frequency-resolved EOFs.  spectrum() is lambda [frequency x mode], components() the complex modes per frequency,
    scores() the expansion coefficients of every block."""

    def __init__(self, n_modes: int = 3, n_fft: int | None = None, n_overlap: int | None = None, window="hamming",
                 sampling_interval: float = 1.0, block_detrend: bool = False, freq_chunk: int | None = None,
                 center: bool = True, standardize: bool = False, use_coslat: bool = False, check_nans=True,
                 sample_name: str = "sample", feature_name: str = "feature", compute: bool = True,
                 random_state: int | None = None, solver: str = "auto", solver_kwargs: dict = {}, **kwargs):
        n_modes = _check_int("n_modes", n_modes, 1, 2 ** 31, "of at least 1")
        if 2 * n_modes > engine.SLABMUL_QMAX:
            raise ValueError(f"n_modes must be at most {engine.SLABMUL_QMAX // 2} per frequency (the slab-product kernel takes "
                             f"{engine.SLABMUL_QMAX} rows), got {n_modes}")
        if n_fft is None:
            raise ValueError("n_fft must be given: the number of samples per block")
        n_fft = _check_int("n_fft", n_fft, 2, engine.BLOCKXFORM_NFFT_MAX, f"in [2, {engine.BLOCKXFORM_NFFT_MAX}]")
        n_overlap = n_fft // 2 if n_overlap is None else _check_int("n_overlap", n_overlap, 0, n_fft - 1,
                                                                    f"in [0, n_fft - 1] = [0, {n_fft - 1}]")
        if not isinstance(sampling_interval, (int, float, np.integer, np.floating)) or not (sampling_interval > 0.0) \
                or not np.isfinite(sampling_interval):
            raise ValueError(f"sampling_interval must be a positive number, got {sampling_interval!r}")
        if freq_chunk is not None:
            freq_chunk = _check_int("freq_chunk", freq_chunk, 1, 2 ** 31, "of at least 1, or None")
        w = window_values(window, n_fft)
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs, **kwargs)
        wname = window if isinstance(window, str) else "custom"
        self.attrs.update({"model": "Spectral EOF analysis", "n_fft": n_fft, "n_overlap": n_overlap, "window": wname,
                           "sampling_interval": float(sampling_interval), "block_detrend": str(bool(block_detrend))})
        self._params.update({"n_fft": n_fft, "n_overlap": n_overlap, "window": window,
                             "sampling_interval": float(sampling_interval), "block_detrend": bool(block_detrend),
                             "freq_chunk": freq_chunk, "solver_kwargs": dict(solver_kwargs)})
        self._window = w

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        mat = self._preprocess(X, dim, weights)
        try:
            pmat = self._centred_twin(mat, X, dim, weights)
        except BaseException:
            mat.free()
            raise
        if pmat is not mat:
            mat.free()
        try:
            return self._fit_algorithm(pmat)
        finally:
            pmat.free()

    def _fit_algorithm(self, mat, omega=None, dec=None):
        """the module's equations on the resident, centred, preprocessed field `mat`"""
        torch = engine._torch()
        ctx, prm = self.ctx, self._params
        n, p = mat.shape
        K, n_fft, n_overlap = int(self.n_modes), prm["n_fft"], prm["n_overlap"]
        if n_fft > n:
            raise ValueError(f"n_fft must not exceed the number of samples: n_fft = {n_fft}, n_samples = {n}")
        hop, nblk = n_fft - n_overlap, block_count(n, n_fft, n_overlap)
        if K > nblk:
            raise ValueError(f"n_modes must be less than or equal to the number of blocks: n_modes = {K}, nblk = {nblk} "
                             f"(n_samples = {n}, n_fft = {n_fft}, n_overlap = {n_overlap})")
        if 2 * nblk > engine.ROWGRAM_RMAX:
            raise ValueError(f"n_fft and n_overlap give {nblk} blocks; the row-Gram kernel takes at most "
                             f"{engine.ROWGRAM_RMAX // 2}: raise n_fft or lower n_overlap")
        nfreq = n_fft // 2 + 1
        B = coefficient_matrix(n_fft, self._window, prm["sampling_interval"], prm["block_detrend"])
        fc = prm["freq_chunk"]
        if fc is None:
            fc = auto_chunk(nfreq, nblk, p, K, torch.cuda.mem_get_info(ctx.device)[0])
        fc = min(fc, engine.SPECTRAL_NBMAX, engine.BLOCKXFORM_NCOEF_MAX // 2)
        ms = dict(blockxform=0.0, rowgram=0.0, eigh=0.0, slabmul=0.0, gauge=0.0, download=0.0)
        tick = time.perf_counter
        lam_all = np.empty((nfreq, nblk), dtype=np.float64)
        trace = np.empty(nfreq, dtype=np.float64)
        scores = np.empty((nfreq, K, nblk), dtype=np.complex128)
        comps = np.empty((nfreq, K, p), dtype=np.complex64)
        M_all = np.empty((nfreq, nblk, nblk), dtype=np.complex128)
        had_layout = mat.has_sample_layout()
        try:
            Bd = torch.from_numpy(B).to(f"cuda:{ctx.device}")
            for k0, k1 in chunk_schedule(nfreq, fc):
                nf = k1 - k0
                t0 = tick()
                Q = engine.mat_blockxform(ctx, mat, Bd[2 * k0:2 * k1], hop, nblk)
                R = Q.view(nf, 2 * nblk, p)
                t1 = tick()
                G = engine.rowgram(ctx, R).cpu().numpy()
                t2 = tick()
                M = M_all[k0:k1] = hermitian_from_gram(G, nblk)
                W = np.empty((nf, 2 * K, 2 * nblk), dtype=np.float32)
                Th = np.empty((nf, nblk, K), dtype=np.complex128)
                for f in range(nf):
                    lam, th = eig_descending(M[f])
                    lam_all[k0 + f], trace[k0 + f] = lam, float(np.trace(M[f]).real)
                    W[f] = mode_weights(lam, th, K)
                    Th[f] = th[:, :K]
                t3 = tick()
                out = engine.slabmul(ctx, W, R)
                del Q, R
                t4 = tick()
                # the gauge: the entry of largest modulus, the lowest index among equals, becomes real and positive
                re, im = out[:, :K], out[:, K:]
                mod = re * re + im * im
                top = mod.amax(dim=2, keepdim=True)
                idx = torch.where(mod == top, torch.arange(p, device=out.device).expand_as(mod),
                                  torch.full_like(mod, p, dtype=torch.int64)).amin(dim=2, keepdim=True).clamp_(max=p - 1)
                z = (torch.gather(re, 2, idx) + 1j * torch.gather(im, 2, idx)).squeeze(2).cpu().numpy()
                u = gauge_factors(z)                                                   # [nf x K]
                ur = torch.from_numpy(u.real.astype(np.float32)).to(out.device)[:, :, None]
                ui = torch.from_numpy(u.imag.astype(np.float32)).to(out.device)[:, :, None]
                gauged = torch.complex(re * ur - im * ui, re * ui + im * ur)
                torch.cuda.synchronize(out.device)
                t5 = tick()
                comps[k0:k1] = gauged.cpu().numpy()
                lam_k = np.clip(lam_all[k0:k1, :K], 0.0, None)
                scores[k0:k1] = (np.sqrt(nblk * lam_k)[:, :, None] * np.conj(np.transpose(Th, (0, 2, 1)))
                                 * np.conj(u)[:, :, None])
                del out, re, im, mod, gauged
                t6 = tick()
                for name, dt in zip(ms, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                    ms[name] += 1e3 * dt
        finally:
            if not had_layout:
                mat.release_sample_layout()
        ok = resolved_modes(lam_all, nblk)[:, :K]
        comps[~ok] = np.nan
        self.data = dict(input_data=None, components=comps, scores=scores, spectrum=lam_all[:, :K].copy(),
                         spectrum_all=lam_all, total_spectrum=trace, resolved=ok, snapshot_matrix=M_all,
                         frequencies=frequency_axis(n_fft, prm["sampling_interval"]),
                         block_centres=np.arange(nblk, dtype=np.float64) * hop + (n_fft - 1) / 2.0)
        self.stats = {f"ms_{name}": v for name, v in ms.items()}
        self.stats.update(freq_chunk=int(fc), nblk=int(nblk), nfreq=int(nfreq))
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X):
        raise NotImplementedError("SpectralEOF has no transform: the scores belong to the blocks of the fit")

    def inverse_transform(self, scores):
        raise NotImplementedError("SpectralEOF has no inverse_transform: the modes of one frequency do not expand the field")

    # ------------------------------------------------------------------ accessors
    def _freq_mode(self, values, name):
        self.compute()
        K = values.shape[1]
        return labelled.pack(values, ("frequency", "mode"), {"frequency": self.data["frequencies"], "mode": np.arange(1, K + 1)},
                             name, dict(self.attrs), self.preprocessor.fields[0].like)

    def frequencies(self):
        """f_k = k fs / n_fft [nfreq]"""
        self.compute()
        return labelled.pack(self.data["frequencies"].copy(), ("frequency",), {"frequency": self.data["frequencies"]},
                             "frequencies", dict(self.attrs), self.preprocessor.fields[0].like)

    def spectrum(self):
        """lambda [frequency x mode]: the power spectral density carried by each mode"""
        return self._freq_mode(self.data["spectrum"], "spectrum")

    def total_spectrum(self):
        """trace M_k [frequency]: the power spectral density summed over the field"""
        self.compute()
        return labelled.pack(self.data["total_spectrum"], ("frequency",), {"frequency": self.data["frequencies"]},
                             "total_spectrum", dict(self.attrs), self.preprocessor.fields[0].like)

    def explained_variance_ratio(self):
        """lambda / trace M_k, per frequency"""
        self.compute()
        tr = self.data["total_spectrum"][:, None]
        ratio = np.divide(self.data["spectrum"], tr, out=np.full(self.data["spectrum"].shape, np.nan), where=tr > 0.0)
        return self._freq_mode(ratio, "explained_variance_ratio")

    def singular_values(self):
        raise AttributeError("SpectralEOF has no singular values: see spectrum()")

    def explained_variance(self):
        raise AttributeError("SpectralEOF has no explained variance: see spectrum()")

    def _feature_maps(self, values, name):
        """[nfreq x K x p_valid] -> per-field arrays with dims (frequency, mode, *feature_dims); NaN where masked"""
        self.compute()
        pre = self.preprocessor
        F, K = values.shape[:2]
        if pre.valid_feature.all():
            full = values
        else:
            full = np.full((F, K, pre.valid_feature.size), np.nan, dtype=values.dtype)
            full[:, :, pre.valid_feature] = values
        outs, off = [], 0
        for f in pre.fields:
            blk = full[:, :, off:off + f.P].reshape((F, K) + f.feature_shape)
            off += f.P
            coords = {d: f.coords[d] for d in f.feature_dims}
            coords["frequency"], coords["mode"] = self.data["frequencies"], np.arange(1, K + 1)
            outs.append(labelled.pack(blk, ("frequency", "mode") + f.feature_dims, coords, name, dict(self.attrs), f.like))
        return pre._wrap(outs)

    def components(self):
        """the complex modes Phi_k: dims (frequency, mode, the input's feature dims)"""
        return self._feature_maps(self.data["components"], "components")

    def components_amplitude(self):
        return self._feature_maps(np.abs(self.data["components"]), "components_amplitude")

    def components_phase(self):
        return self._feature_maps(np.angle(self.data["components"]), "components_phase")

    def scores(self):
        """the expansion coefficients a_k[m, b] of every block: complex, dims (frequency, mode, block)"""
        self.compute()
        S = self.data["scores"]
        return labelled.pack(S, ("frequency", "mode", "block"),
                             {"frequency": self.data["frequencies"], "mode": np.arange(1, S.shape[1] + 1),
                              "block": self.data["block_centres"]}, "scores", dict(self.attrs),
                             self.preprocessor.fields[0].like)
