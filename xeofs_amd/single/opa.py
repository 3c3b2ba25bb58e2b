"""xeofs_amd.single.OPA -- drop-in for xeofs.single.OPA (xeofs/single/opa.py:12-295): optimal persistence analysis
[DelSole 2001, 2006], the patterns of a field whose time series have the longest decorrelation time.

With S [n x q] the PCA scores of the preprocessed field scaled to unit variance and Cmp [P x q] the matching patterns,

    C_tau = S[:n - tau]^T S[tau:] / (n - tau - 1),     M = 1/2 C_0 + C_1 + ... + C_{T-1} + 1/2 C_T,     T = tau_max,

the optimally persistent patterns solve the symmetric problem of Hannachi (2021, eq. 8.20): with C_0 = E D E^T and
K = D^-1/2 E^T, the leading eigenpairs (lam, Uo) of Tm = 1/2 K (M + M^T) K^T give the decorrelation times lam, the filter
patterns Cmp K^T Uo, the patterns Cmp C_0 K^T Uo and the time series S K^T Uo.

The reference forms the T + 1 lagged products one by one (opa.py:104-171).  Here M = S^T Y with the filtered panel
Y[t] = sum_tau w_tau S[t + tau] (`opa_lag_weights`, rows past n count as zero): one engine call (engine.lagcov,
csrc/eofx_lagcov.hpp).  The inner PCA is the engine's resident decomposition; C_0 comes from the same kernel; the q x q
algebra and the two symmetric eigenproblems run in float64 on the host (eofx_host_eigh_f64); the products over the P
features and n samples run in float64 on the device in a fixed order and are rounded once to float32.

Deliberate deviations from the reference:
  1. every mode carries the engine's deterministic sign (positive where |max| >= |min| of its pattern), the same one on
     components, scores and filter patterns; the reference keeps LAPACK's (`flip_signs=False`);
  2. Tm is built in the symmetric form K Msum K^T; the reference multiplies by K on the right as well, which coincides
     with it only because C_0 of PCA scores is diagonal to rounding;
  3. the modes are ordered by lam descending (a symmetric eigensolver); the reference takes an SVD and orders by |lam|.
     The two agree whenever the leading values are positive.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled, spca
from ..linalg.decomposer import Decomposer
from . import _pcspace
from .eof import EOF, NO_EXPLAINED_VARIANCE, NO_SINGULAR_VALUES


def opa_lag_weights(n: int, tau_max: int) -> np.ndarray:
    """w [tau_max + 1] with M = sum_tau w[tau] S[:n - tau]^T S[tau:] (opa.py:154-166): 1 / (n - tau - 1), halved at both
    ends.  The largest lag must leave two samples: 0 <= tau_max <= n - 2."""
    n, T = int(n), int(tau_max)
    if T < 0 or T > n - 2:
        raise ValueError(f"tau_max must be in [0, n_samples - 2 = {n - 2}], got {tau_max}")
    w = 1.0 / (n - np.arange(T + 1, dtype=np.float64) - 1.0)
    if T == 0:
        return 0.5 * w
    w[0] *= 0.5
    w[T] *= 0.5
    return w


class OPA(EOF):
    """Drop-in for xeofs.single.OPA (xeofs/single/opa.py:12-295).  components() are the optimally persistent patterns,
    scores() their time series (uncorrelated, unit variance), filter_patterns() the filter patterns and
    decorrelation_time() the decorrelation times, descending."""

    def __init__(self, n_modes: int, tau_max: int, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 check_nans: bool = True, n_pca_modes: int = 100, compute: bool = True, sample_name: str = "sample",
                 feature_name: str = "feature", solver: str = "auto", random_state: int | None = None,
                 solver_kwargs: dict = {}):
        if n_modes > n_pca_modes:
            raise ValueError(
                f"n_modes must be smaller or equal to n_pca_modes (n_modes={n_modes}, n_pca_modes={n_pca_modes})"
            )
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs)
        self.attrs.update({"model": "OPA"})
        self._params.update({"tau_max": tau_max, "n_pca_modes": n_pca_modes})
        self._params["solver_kwargs"] = dict(solver_kwargs)

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        mat = self._preprocess(X, dim, weights)
        pmat = self._centred_twin(mat, X, dim, weights)
        if pmat is not mat:
            mat.free()
        try:
            return self._fit_algorithm(pmat)
        finally:
            pmat.free()

    def _fit_algorithm(self, mat, omega=None, dec=None):
        """opa.py:128-269 on the resident, centred, preprocessed field"""
        prm, ctx = self._params, self.ctx
        torch = engine._torch()
        n, k = mat.n, int(self.n_modes)
        w = opa_lag_weights(n, prm["tau_max"])
        # 1. inner PCA (opa.py:135-152)
        t0 = time.perf_counter()
        pca = Decomposer.for_model(prm, prm["n_pca_modes"], ctx).fit(mat)
        root = np.sqrt(n - 1.0)
        S32 = np.ascontiguousarray(pca.U_.astype(np.float64) * pca.s_.astype(np.float64) / root, dtype=np.float32)
        Cmp32 = np.ascontiguousarray(pca.V_.astype(np.float64) * root, dtype=np.float32)
        q = S32.shape[1]
        if k > q:
            raise ValueError(f"n_modes must be smaller or equal to the {q} PCA modes kept (n_modes={k})")
        t1 = time.perf_counter()
        # 2. lag covariances: C_0 from the actual scores and M, one kernel call each
        Sd = engine.device_panel(ctx, S32)
        C0 = engine.lagcov(ctx, Sd, np.array([1.0 / (n - 1.0)])).cpu().numpy()
        M = engine.lagcov(ctx, Sd, w).cpu().numpy()
        t2 = time.perf_counter()
        C0 = 0.5 * (C0 + C0.T)
        # 3. whitening with the full eigendecomposition of C_0, 4. the symmetric eigenproblem (Hannachi 2021, eq. 8.20)
        lam, Uo, Vq, Wq = _pcspace.whitened_modes(C0, 0.5 * (M + M.T), k)
        t3 = time.perf_counter()
        # 5. products of inner length q in float64 on the device (fixed order), rounded once; one sign per mode
        proj, sg = _pcspace.signed_projection(lambda X, B: spca.spca_rowmul(ctx, X, B), spca._dev64(ctx, Cmp32),
                                              Sd.to(torch.float64), Vq, Wq)
        self.data = dict(input_data=S32, **proj, decorrelation_time=lam)
        self._U, self._C0 = Uo * sg, C0                 # kept as the reference keeps them (opa.py:267-268)
        self._Vq = Vq * sg
        self._pca_scores, self._pca_components = S32, Cmp32
        t4 = time.perf_counter()
        self.stats = dict(route=pca.route_, n_pca_modes=q, ms_pca=1e3 * (t1 - t0), ms_lagcov=1e3 * (t2 - t1),
                          ms_eigen=1e3 * (t3 - t2), ms_project=1e3 * (t4 - t3))
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X, normalized: bool = False):
        raise NotImplementedError("OPA does not (yet) support transform()")

    def inverse_transform(self, scores, normalized: bool = False):
        raise NotImplementedError("OPA does not (yet) support inverse_transform()")

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the optimally persistent patterns"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def filter_patterns(self):
        return self.preprocessor.inverse_transform_components(self.data["filter_patterns"], "filter_patterns", self.attrs)

    def decorrelation_time(self):
        return self._mode_array(self.data["decorrelation_time"], "decorrelation_time")

    singular_values = NO_SINGULAR_VALUES
    explained_variance = explained_variance_ratio = NO_EXPLAINED_VARIANCE
