"""xeofs_amd.single.LFCA -- low-frequency component analysis [Wills et al. 2018, GRL 45; Wills et al. 2020, J. Climate 33]:
the linear combinations of the leading EOFs of a field with the largest ratio of low-pass-filtered variance to total
variance.  The reference has no such model; the definition is stated here in full.

With V [P x q] the PCA patterns of the preprocessed field X and S = X V [n x q] its PCA scores (the projection, as POP takes
them, so that `transform` of the training data returns `scores()`), w_0 .. w_h the Lanczos low-pass weights of half-width h
and cutoff period `cutoff` (`lanczos_weights`), refl the mirror of a sample index about the first and the last sample
(`reflect_index`) and a_j + b_j t the least-squares line of column j of S (`linear_trend`; a = b = 0 with detrend=False),

    d(u, j) = S[u, j] - (a_j + b_j u),      Y[t, j] = sum_{k = -h .. h} w_|k| d(refl(t + k), j) + (a_j + b_j t),
    C0 = S^T S / (n - 1) = E D E^T,   K = D^-1/2 E^T,   R = Y^T Y / (n - 1),   Tm = 1/2 (K R K^T + its transpose),
    (r, Uo) = the k leading eigenpairs of Tm, r descending,   Vq = K^T Uo,
    scores (LFCs) = S Vq,   components (LFPs) = V C0 Vq,   filter_patterns = V Vq,   low_frequency_ratio = r.

The LFCs are uncorrelated with unit variance, X ~ LFCs . LFPs^T within the q kept modes, and LFC = X . filter pattern.

The filter and both covariances are ONE engine entry (engine.lowpass_cov, csrc/eofx_lowpass.hpp): Y is float64 and never
rounded to float32 -- the whitening by K amplifies the trailing PC columns by s_1 / s_q.  The q x q algebra and the two
symmetric eigenproblems run in float64 on the host (eofx_host_eigh_f64); the products of inner length q run in float64 on
the fp64 matrix cores (engine.pcmul) and are rounded once to float32.

Deliberate choices: time-domain Lanczos weights rather than a frequency-domain filter; mirrored ends; the
linear trend removed before the filter and added back after it by default (a mirrored trending series has a kink at either
end); the symmetric whitened eigenproblem; the engine's deterministic sign per mode (positive where |max| >= |min| of its
pattern), the same on components, scores and filter patterns.
"""

from __future__ import annotations

import math
import time

import numpy as np

from .. import engine, labelled
from ..linalg.decomposer import Decomposer
from ..preprocessing import parse_scores
from . import _pcspace
from .eof import EOF, NO_EXPLAINED_VARIANCE, NO_SINGULAR_VALUES


# ---------------------------------------------------------------------------------------------------- host helpers
def lanczos_weights(cutoff: float, h: int) -> np.ndarray:
    """w [h + 1], the Lanczos low-pass weights (Duchon 1979) of half-width h >= 1 and cutoff period `cutoff` > 2 samples:
    with fc = 1 / cutoff, w~_0 = 2 fc, w~_k = sin(2 pi fc k) / (pi k) . sin(pi k / (h + 1)) / (pi k / (h + 1)), normalised
    so that w_0 + 2 sum_{k >= 1} w_k = 1 (unit response at frequency 0).  The filter is w_|k|, k = -h .. h."""
    h = int(h)
    if not cutoff > 2:
        raise ValueError(f"cutoff must be a period above 2 samples (the Nyquist period), got {cutoff}")
    if h < 1:
        raise ValueError(f"the half-width h must be >= 1, got {h}")
    fc = 1.0 / float(cutoff)
    k = np.arange(1, h + 1, dtype=np.float64)
    x = np.pi * k / (h + 1.0)
    w = np.empty(h + 1)
    w[0] = 2.0 * fc
    w[1:] = np.sin(2.0 * np.pi * fc * k) / (np.pi * k) * (np.sin(x) / x)
    return w / (w[0] + 2.0 * w[1:].sum())


def reflect_index(u, n: int) -> np.ndarray:
    """the mirror of the sample indices u about the first and the last of n samples: -u below 0, 2 (n - 1) - u above n - 1
    (one reflection: -(n - 1) <= u <= 2 (n - 1))"""
    u = np.asarray(u, dtype=np.int64)
    n = int(n)
    if np.any(u < -(n - 1)) or np.any(u > 2 * (n - 1)):
        raise ValueError(f"one reflection covers {-(n - 1)} .. {2 * (n - 1)} for n = {n}")
    return np.where(u < 0, -u, np.where(u > n - 1, 2 * (n - 1) - u, u))


def linear_trend(S) -> np.ndarray:
    """[2 x p] float64: the intercepts a and the slopes b of the least-squares lines a_j + b_j t, t = 0 .. n - 1, of the
    columns of S [n x p], in closed form about tbar = (n - 1) / 2"""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] < 2:
        raise ValueError(f"S must be a matrix of at least two rows, got shape {S.shape}")
    n = S.shape[0]
    tc = np.arange(n, dtype=np.float64) - 0.5 * (n - 1.0)
    mean = S.mean(axis=0)
    b = tc @ (S - mean) / (tc @ tc)
    return np.stack([mean - b * 0.5 * (n - 1.0), b])


def default_half_width(n: int, cutoff: float) -> int:
    """h = min(n - 1, ceil(1.5 cutoff))"""
    return min(int(n) - 1, int(math.ceil(1.5 * cutoff)))


class LFCA(EOF):
    """Low-frequency component analysis.  components() are the low-frequency patterns, scores() the low-frequency components
    (uncorrelated, unit variance), filter_patterns() the fingerprints, low_frequency_ratio() the ratios of low-pass-filtered
    to total variance, descending, and filtered_scores() the low-passed components.  `cutoff`: the cutoff period in samples;
    `window`: the odd number 2 h + 1 of filter weights (default h = min(n - 1, ceil(1.5 cutoff)))."""

    def __init__(self, n_modes: int, cutoff: float, window: int | None = None, detrend: bool = True, n_pca_modes: int = 100,
                 center: bool = True, standardize: bool = False, use_coslat: bool = False, check_nans: bool = True,
                 compute: bool = True, sample_name: str = "sample", feature_name: str = "feature", solver: str = "auto",
                 random_state: int | None = None, solver_kwargs: dict = {}):
        if not cutoff > 2:
            raise ValueError(f"cutoff must be a period above 2 samples (the Nyquist period), got {cutoff}")
        if window is not None:
            if int(window) != window or window % 2 == 0:
                raise ValueError(f"window must be an odd number of weights 2 h + 1, got {window}")
            if window < 3:
                raise ValueError(f"window must be at least 3 weights (h >= 1), got {window}")
        if isinstance(n_pca_modes, (int, np.integer)) and n_modes > n_pca_modes:      # (a variance fraction is checked at fit)
            raise ValueError(
                f"n_modes must be smaller or equal to n_pca_modes (n_modes={n_modes}, n_pca_modes={n_pca_modes})"
            )
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs)
        self.attrs.update({"model": "LFCA"})
        self._params.update({"cutoff": cutoff, "window": window, "detrend": bool(detrend), "n_pca_modes": n_pca_modes})
        self._params["solver_kwargs"] = dict(solver_kwargs)

    def _half_width(self, n: int) -> int:
        window = self._params["window"]
        h = default_half_width(n, self._params["cutoff"]) if window is None else (int(window) - 1) // 2
        if h > n - 1:
            raise ValueError(f"window = {window} needs h = {h} <= n_samples - 1 = {n - 1} (one reflection about either end)")
        if h < 1:
            raise ValueError(f"LFCA needs at least 2 samples, got n_samples = {n}")
        return h

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        mat = self._preprocess(X, dim, weights)
        pmat = self._centred_twin(mat, X, dim, weights)
        try:
            return self._fit_algorithm(mat, pmat)
        finally:
            if pmat is not mat:
                pmat.free()
            mat.free()

    def _fit_algorithm(self, mat, pmat=None, dec=None):
        """the module's equations on the resident, preprocessed field `mat`; the inner PCA decomposes its centred twin"""
        prm, ctx = self._params, self.ctx
        pmat = mat if pmat is None else pmat
        n, k = mat.n, int(self.n_modes)
        h = self._half_width(n)
        w = lanczos_weights(prm["cutoff"], h)
        # 1. inner PCA; the scores are the projection X V
        t0 = time.perf_counter()
        pca = Decomposer.for_model(prm, prm["n_pca_modes"], ctx)
        pca.fit(pmat, total_variance=self.preprocessor.total_variance)
        V32, S32 = pca.projected_scores(mat)
        q = S32.shape[1]
        if k > q:
            raise ValueError(f"n_modes must be smaller or equal to the {q} PCA modes kept (n_modes={k})")
        t1 = time.perf_counter()
        # 2. C0 = S^T S / (n - 1) and R = Y^T Y / (n - 1), one kernel call each
        trend = linear_trend(S32) if prm["detrend"] else None
        Sd = engine.device_panel(ctx, S32)
        C0 = engine.lowpass_cov(ctx, Sd, np.array([1.0])).cpu().numpy() / (n - 1.0)
        R = engine.lowpass_cov(ctx, Sd, w, trend).cpu().numpy() / (n - 1.0)
        t2 = time.perf_counter()
        # 3. whitening with the full eigendecomposition of C0 (of full rank to float32 accuracy), 4. the symmetric eigenproblem
        r, Uo, Vq, Wq = _pcspace.whitened_modes(C0, R, k, rank_rows=n)
        t3 = time.perf_counter()
        # 5. products of inner length q in float64 on the matrix cores (fixed order), rounded once; one sign per mode
        proj, sg = _pcspace.signed_projection(lambda X, B: engine.pcmul(ctx, X, B), V32, Sd, Vq, Wq)
        self.data = dict(input_data=S32, **proj, low_frequency_ratio=r)
        self._U, self._C0, self._R = Uo * sg, C0, R
        self._Vq = Vq * sg
        self._weights, self._half = w, h
        self._pca_scores, self._pca_components = S32, V32
        t4 = time.perf_counter()
        self.stats = dict(route=pca.route_, n_pca_modes=q, ms_pca=1e3 * (t1 - t0), ms_lowpass=1e3 * (t2 - t1),
                          ms_eigen=1e3 * (t3 - t2), ms_project=1e3 * (t4 - t3))
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X, normalized: bool = False):
        """new data -> the fitted preprocessing -> PC space (X V) -> the fitted combination Vq"""
        self.compute()
        Z, fields, vs = _pcspace.project_modes(self, X, self._Vq, engine._torch().float32)
        if normalized:
            Z = Z / self.data["norms"].astype(Z.dtype)
        return self.preprocessor.inverse_transform_scores(Z, "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores, normalized: bool = False):
        """Xhat = scores . components^T over the modes the scores name, float64 products of inner length k' on the matrix
        cores (engine.pcmul over blocks of 2048 features), un-scaled with the fitted preprocessing"""
        self.compute()
        S, modes, vs, fields = parse_scores(scores, self.preprocessor.fields, np.float64, scalar_mode=True)
        if normalized:
            S = S * self.data["norms"][modes - 1]
        C = self.data["components"][:, modes - 1]
        Z = engine.device_panel(self.ctx, np.ascontiguousarray(S, dtype=np.float64))
        rec = _pcspace.reconstruct(self.ctx, Z, C)
        return self.preprocessor.inverse_transform_data(rec, "reconstructed_data", fields, vs)

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the low-frequency patterns"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def filter_patterns(self):
        """the fingerprints: LFC = X . filter pattern"""
        return self.preprocessor.inverse_transform_components(self.data["filter_patterns"], "filter_patterns", self.attrs)

    def low_frequency_ratio(self):
        return self._mode_array(self.data["low_frequency_ratio"], "low_frequency_ratio")

    def filtered_scores(self):
        """the low-passed low-frequency components: the fitted filter (and `detrend` setting) applied to scores()"""
        self.compute()
        S = self.data["scores"]
        trend = linear_trend(S) if self._params["detrend"] else None
        Y = engine.lowpass(self.ctx, S, self._weights, trend).cpu().numpy()
        return self.preprocessor.inverse_transform_scores(Y, "filtered_scores", self.attrs)

    singular_values = NO_SINGULAR_VALUES
    explained_variance = explained_variance_ratio = NO_EXPLAINED_VARIANCE
