"""xeofs_amd.single.TrendEOF -- trend EOF analysis [Hannachi 2007, Int. J. Climatol. 27, "Pattern hunting in climate: a new
method for finding trends in gridded climate data"]: the EOFs of the field's INVERSE RANKS -- every grid point's series replaced
by the time positions of its order statistics -- mapped back to physical space.  It finds monotone, not only linear, trends
and is insensitive to outliers and to the marginal distribution.  The reference has no such model; the
definition is stated here in full.

With Xc [n x p] the engine's preprocessed float32 matrix of the fit (centred, weights applied; with center=False its centred
twin stands in for it, `EOF._centred_twin`, as in LFCA and OPA) and w_j >= 0 the feature weight the preprocessor applied
(coslat x user weights, 1 by default -- not 1 / std),

    Q[r, j] = the time index t (0-based) of the r-th smallest value of column j of Xc, equal values in ascending time
              (numpy.argsort(kind="stable"); -0.0 equals +0.0),
    Z[r, j] = (Q[r, j] - (n - 1) / 2) w_j                       (the float64 product, rounded once to float32),
    total_variance = n (n + 1) / 12 . sum_j w_j^2                 (every column of Q is a permutation of 0 .. n - 1: exact),
    Z ~ U S V^T   of rank k: the engine's randomized SVD through Decomposer, with the engine's sign rule,
    trend_eofs() = V [p x k],    singular_values = s,    explained_variance = s^2 / (n - 1),   ..._ratio = that / total_variance,
    scores() (the trend PCs)     = S = Xc V [n x k]               (engine.project; transform(X') = fitted preprocessing, then . V),
    components() (the trend patterns) = Xc^T Sh / (n - 1),   Sh = (S - mean) / std(ddof = 1) per column:

the regression of the field on each standardized trend PC, in the field's units after preprocessing.

Q and Z are ONE engine entry over the resident matrix (engine.rank_matrix, csrc/eofx_orderpos.hpp): a workgroup reads a series
once from the sample-contiguous layout, sorts it in LDS as 64-bit (value, time) keys and writes its row of Z once, straight
into the sample-contiguous layout of a new resident matrix -- hence n <= 16384 samples.  The rank matrix is freed after the
decomposition; the sample layout of Xc is released again if this fit built it.

Deliberate choices: ranks are taken on the engine's float32 values, so a tie the Scaler's rounding creates is
a tie; the weights multiply Q rather than the data (ranks ignore positive scalings); the centring of Q is analytic; the
patterns are the regression on the STANDARDIZED PC.  There is no inverse_transform: the trend PCs are not an orthogonal
expansion of X.  With center=False, `transform` applies the fitted (uncentred) preprocessing, so it returns the scores of the
training data plus the constant mean . V.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled
from ..linalg.decomposer import Decomposer
from .eof import EOF

MAX_SAMPLES = engine.ORDERPOS_NMAX


def trend_total_variance(n: int, weights) -> float:
    """n (n + 1) / 12 . sum_j w_j^2: the variance (ddof = 1) of a permutation of 0 .. n - 1 is n (n + 1) / 12"""
    w = np.asarray(weights, dtype=np.float64)
    return float(n) * (n + 1.0) / 12.0 * float(np.dot(w, w))


class TrendEOF(EOF):
    """Trend EOF analysis.  trend_eofs() are the patterns in rank space, scores() the trend PCs, components() the trend
    patterns: the regression of the preprocessed field on the standardized trend PCs.  singular_values(),
    explained_variance() and explained_variance_ratio() are those of the rank matrix."""

    def __init__(self, n_modes: int = 2, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 check_nans=True, sample_name: str = "sample", feature_name: str = "feature", compute: bool = True,
                 random_state: int | None = None, solver: str = "auto", solver_kwargs: dict = {}, **kwargs):
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs, **kwargs)
        self.attrs.update({"model": "Trend EOF analysis"})
        self._params["solver_kwargs"] = dict(solver_kwargs)

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        self._decomposer_kwargs["lazy_input"] = labelled.is_lazy(X)
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

    def _feature_weights(self, p: int) -> np.ndarray:
        """w [p]: the weights the preprocessor applied to the valid features"""
        pre = self.preprocessor
        if pre.feature_weights is None:
            return np.ones(p)
        w = np.ascontiguousarray(np.asarray(pre.feature_weights, dtype=np.float64)[pre.valid_feature])
        if np.any(w < 0):
            raise ValueError("TrendEOF takes non-negative feature weights: a negative weight would reverse the ranks of its "
                             "feature")
        return w

    def _fit_algorithm(self, mat, omega=None, dec=None):
        """the module's equations on the resident, centred, preprocessed field `mat`"""
        ctx = self.ctx
        n, p = mat.shape
        if n > MAX_SAMPLES:
            raise ValueError(f"TrendEOF sorts a series on chip: at most {MAX_SAMPLES} samples, got n_samples = {n}")
        w = self._feature_weights(p)
        # 1. the rank matrix Z, resident; X's sample layout goes back if it was built here
        t0 = time.perf_counter()
        had_layout = mat.has_sample_layout()
        zmat = engine.rank_matrix(ctx, mat, None if self.preprocessor.feature_weights is None else w)
        if not had_layout:
            mat.release_sample_layout()
        total_variance = trend_total_variance(n, w)
        t1 = time.perf_counter()
        # 2. Z ~ U S V^T
        try:
            dec = Decomposer(ctx=ctx, **self._decomposer_kwargs)
            dec.fit(zmat, dims=(self.sample_name, self.feature_name), total_variance=total_variance)
        finally:
            zmat.free()
        t2 = time.perf_counter()
        # 3. the trend PCs S = X V and the regression of the field on the standardized PCs
        V = np.ascontiguousarray(dec.V_, dtype=np.float32)
        s = dec.s_.astype(np.float64)
        k = V.shape[1]
        S = np.ascontiguousarray(engine.project(ctx, mat, V), dtype=np.float32)
        S64 = S.astype(np.float64)
        mean, std = S64.mean(axis=0), S64.std(axis=0, ddof=1)
        if not np.all(std > 0.0):
            raise np.linalg.LinAlgError(f"trend PC {int(np.flatnonzero(~(std > 0.0))[0]) + 1} has zero variance: it has no "
                                        "standardized form to regress the field on")
        Sh = np.ascontiguousarray((S64 - mean) / std / (n - 1.0), dtype=np.float32)
        Rp = engine.panel_import(ctx, Sh, mat.n_pad, engine.panel_width(k))
        out = engine.panel_tmul(ctx, mat, Rp, prec=ctx.precision[1])
        patterns = mat.compact_rows(engine.panel_export(ctx, out, mat.p_phys, k))
        t3 = time.perf_counter()
        self.data = dict(input_data=S, components=patterns, scores=S, trend_eofs=V, norms=s,
                         explained_variance=s ** 2 / (n - 1.0), total_variance=total_variance)
        self.stats = dict(route=dec.route_, ms_rank=1e3 * (t1 - t0), ms_svd=1e3 * (t2 - t1), ms_project=1e3 * (t3 - t2))
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X, normalized: bool = False):
        """new data -> the fitted preprocessing -> X V, the projection on the rank-space patterns"""
        self.compute()
        mat, fields, vs = self.preprocessor.transform(X)
        try:
            proj = engine.project(self.ctx, mat, self.data["trend_eofs"])
        finally:
            mat.free()
        if normalized:
            proj = proj / self.data["norms"].astype(proj.dtype)
        return self.preprocessor.inverse_transform_scores(proj, "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores, normalized: bool = False):
        raise NotImplementedError("TrendEOF has no inverse_transform: the trend PCs are not an orthogonal expansion of X")

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the trend patterns: the regression of the preprocessed field on each standardized trend PC"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def trend_eofs(self):
        """the patterns in rank space: the right singular vectors of the rank matrix"""
        return self.preprocessor.inverse_transform_components(self.data["trend_eofs"], "trend_eofs", self.attrs)
