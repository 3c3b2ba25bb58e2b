"""xeofs_amd.multi.CCA -- drop-in for xeofs.multi.CCA (xeofs/multi/cca.py:47-706): regularised canonical correlation analysis
of m >= 2 views at once, after cca-zoo's MCCA [Chapman et al. 2021; Vinod 1976; Hotelling 1936].

With X_i [n x P_i] the preprocessed views, V_i [P_i x k_i] the leading PCA patterns of view i and S_i = X_i V_i its PCA
scores (`pca=True`; with `pca=False` S_i = X_i), Z = [S_1 | ... | S_m] [n x p] and c_i the ridge parameters,

    C = (cov(Z) with its diagonal blocks removed) / m,
    D = (blockdiag((1 - c_i) cov(S_i) + c_i I) - (min(0, lam_min) - eps) I) / m,
    C x = lam D x,   x^T D x = 1,   the n_modes largest lam,

weights_i = V_i x_i (feature space), loadings = weights over their 2-norm, variates_i = X_i weights_i, canonical loadings
X_i^T variates_i.

C is ONE call of the block cross-covariance kernel (engine.viewcov, csrc/eofx_viewcov.hpp): float64 on the matrix cores, only
the tiles on or above the diagonal that hold an entry of two different views.  On the PCA route D is diagonal (the explained
variances), so the generalised problem becomes the standard one of D^-1/2 C D^-1/2, solved in float64 by
scipy.linalg.eigh(subset_by_index=...) on the host up to CCA_HOST_EIG_PMAX columns and by torch.linalg.eigh on the device
beyond (`stats["eig_route"]`).  The weights are a PC-space product (engine.pcmul) rounded once to float32; variates,
canonical loadings and the transformed views go through the projection and the X^T Z pass over the resident views.

Deliberate deviations from the reference:
  1. the sign of every mode is fixed: the entry of largest modulus of the concatenated eigenvector x is positive (the lowest
     index on ties); LAPACK leaves it open;
  2. `transform` preprocesses EVERY view and returns one entry per view (the reference overwrites its own list, cca.py:646-650);
  3. limits: k_i <= engine.PCMUL_AMAX PCA modes per view and sum k_i <= engine.VIEWCOV_PMAX (ValueError naming the parameter
     to lower); `pca=False` runs while sum P_i <= engine.VIEWCOV_PMAX (NotImplementedError beyond).
"""

from __future__ import annotations

import datetime
import time

import numpy as np

from .. import __version__, engine, labelled
from .._deferred import Deferred
from ..linalg.decomposer import Decomposer
from ..preprocessing import Preprocessor

CCA_HOST_EIG_PMAX = 1024      # up to here the eigenproblem is solved on the host (LAPACK's subset driver), beyond on the device


# ---------------------------------------------------------------------------------------------------- host algebra
def process_parameter(parameter_name: str, parameter, default, n_views: int):
    """one value per view from a scalar, None (the default) or a list / tuple, whose length must be the number of views
    (the reference's message, cca.py:29-44)"""
    values = list(parameter) if isinstance(parameter, (list, tuple)) else [default if parameter is None else parameter] * n_views
    if len(values) != n_views:
        raise ValueError(f"number of views passed should match number of parameter {parameter_name}"
                         f"len(views)={n_views} and len({parameter_name})={len(values)}")
    return values


def process_init_pca_modes(n_modes, n_samples: int, n_features):
    """cca.py:108-126: a float <= 1 is that share of min(n_samples, n_features), an integer > 1 is taken as it is"""
    err_msg = "init_pca_modes must be either a float <= 1.0 or an integer > 1"
    out = []
    for n, n_feat in zip(n_modes, n_features):
        n_max = min(n_samples, n_feat)
        if isinstance(n, (float, np.floating)):
            if n > 1.0:
                raise ValueError(err_msg)
            out.append(int(n * n_max))
        elif isinstance(n, (int, np.integer)) and not isinstance(n, bool):
            if n <= 1:
                raise ValueError(err_msg)
            out.append(int(n))
        else:
            raise ValueError(err_msg)
    return out


def pca_modes_to_keep(explained_variance_ratio, variance_fraction: float):
    """cca.py:183-208 -> (modes kept, the warning the reference prints or None): the cumulative ratio less 1e-6, the modes at
    or below the fraction plus one, at least 2"""
    cum = np.cumsum(np.asarray(explained_variance_ratio, dtype=np.float64)) - 1e-6
    warning = None
    if cum[-1] <= variance_fraction and cum[-1] <= 0.9999:
        warning = ("Warning: variance fraction {:.4f} is not reached. ".format(variance_fraction)
                   + "Only {:.4f} of variance is explained.".format(cum[-1]))
    return max(int((cum <= variance_fraction).sum()) + 1, 2), warning


def shift_diagonal(d, eps: float, n_views: int):
    """cca.py:582-586 for a diagonal D: d - (min(0, min d) - eps), over the number of views"""
    d = np.asarray(d, dtype=np.float64)
    return (d - (min(0.0, float(d.min())) - eps)) / n_views


def shift_matrix(D, eps: float, n_views: int):
    """cca.py:582-586 for a dense D"""
    D = np.asarray(D, dtype=np.float64)
    return (D - (min(0.0, float(np.linalg.eigvalsh(D).min())) - eps) * np.eye(D.shape[0])) / n_views


def fix_signs(x: np.ndarray) -> np.ndarray:
    """every column with its entry of largest modulus (the lowest index on ties) positive"""
    x = np.array(x, dtype=np.float64)
    top = np.argmax(np.abs(x), axis=0)                        # (the first of equal maxima)
    x *= np.where(x[top, np.arange(x.shape[1])] < 0.0, -1.0, 1.0)
    return x


def whitened_form(C, d):
    """-> (D^-1/2 C D^-1/2, d^-1/2) for the diagonal D = diag(d) > 0: C x = lam D x becomes the standard problem of the
    first with x = D^-1/2 y"""
    dinv = 1.0 / np.sqrt(np.asarray(d, dtype=np.float64))
    return np.asarray(C, dtype=np.float64) * dinv[:, None] * dinv[None, :], dinv


def gevp_diagonal(C, d, k: int):
    """the k largest eigenpairs of C x = lam diag(d) x on the host, lam descending, x^T D x = 1, signs fixed"""
    from scipy.linalg import eigh

    Ct, dinv = whitened_form(C, d)
    p = Ct.shape[0]
    lam, Y = eigh(0.5 * (Ct + Ct.T), subset_by_index=[p - k, p - 1])
    order = np.argsort(lam)[::-1]
    return lam[order], fix_signs(Y[:, order] * dinv[:, None])


def gevp_dense(C, D, k: int):
    """cca.py:412-429: the k largest eigenpairs of C x = lam D x by LAPACK's generalised driver, signs fixed"""
    from scipy.linalg import eigh

    p = C.shape[0]
    lam, X = eigh(np.asarray(C, dtype=np.float64), np.asarray(D, dtype=np.float64), subset_by_index=[p - k, p - 1])
    order = np.argsort(lam)[::-1]
    return lam[order], fix_signs(X[:, order])


def total_explained_covariance(abs_eigenvalues, minimum_dimension: int) -> float:
    """cca.py:372-379: the singular values of the symmetric block cross-covariance are the moduli of its eigenvalues; every
    second one from the first, the first `minimum_dimension` of those"""
    s = np.sort(np.abs(np.asarray(abs_eigenvalues, dtype=np.float64)))[::-1]
    return float(s[::2][:minimum_dimension].sum())


class CCA(Deferred):
    """Drop-in for xeofs.multi.CCA (xeofs/multi/cca.py:222-706).  `fit(views, dim)` takes a list of labelled arrays sharing
    the sample dimension(s); every accessor returns one entry per view unless noted."""

    def __init__(self, n_modes: int = 2, use_coslat=False, check_nans: bool = True, c=0, pca: bool = True,
                 variance_fraction: float = 0.99, init_pca_modes=0.75, compute: bool = True, eps: float = 1e-6,
                 random_state: int | None = None, solver: str = "auto", solver_kwargs: dict = {}, ctx=None):
        self.n_modes = n_modes
        self.sample_name, self.feature_name = "sample", "feature"
        self._params = dict(n_modes=n_modes, use_coslat=use_coslat, check_nans=check_nans, c=c, pca=pca,
                            variance_fraction=variance_fraction, init_pca_modes=init_pca_modes, compute=compute, eps=eps,
                            random_state=random_state, solver=solver)
        self._solver_kwargs = dict(solver_kwargs)
        self.ctx = ctx
        self.attrs = {"model": "CCA", "software": "xeofs_amd", "version": __version__,
                      "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")}
        self.data = {}
        self._stats = {}
        self._preprocessors = None

    # fitted state: reading it runs a deferred fit first, as reading `data` does (_deferred.py)
    @property
    def preprocessors(self):
        self.compute()
        return self._preprocessors

    @property
    def stats(self):
        self.compute()
        return self._stats

    def get_params(self):
        return dict(self._params)

    # ------------------------------------------------------------------ fit
    def fit(self, views, dim):
        if labelled.is_lazy(list(views)) and not self._params["compute"]:         # the reference leaves dask graphs: defer
            return self._defer(lambda: self._fit_now(views, dim))
        return self._fit_now(views, dim)

    def _fit_now(self, views, dim):
        prm = self._params
        views = list(views)
        m = self.n_views_ = len(views)
        self.use_coslat = process_parameter("use_coslat", prm["use_coslat"], False, m)
        self.init_pca_modes = process_parameter("init_pca_modes", prm["init_pca_modes"], 0.75, m)
        self.c = process_parameter("c", prm["c"], 0, m)
        if any(labelled.is_complex(v) for v in views):
            raise TypeError("This method does not support complex data.")
        self.ctx = self.ctx or engine.default_context()
        # 1. one preprocessor per view: centred, not standardised, coslat per view; the views stay resident
        pres = [Preprocessor(True, False, bool(self.use_coslat[i]), prm["check_nans"], ctx=self.ctx, in_place=True)
                for i in range(m)]
        self._free()                               # a fit that raises leaves the model unfitted, not half of the old fit
        mats = []
        try:
            for pre, v in zip(pres, views):
                mats.append(pre.fit_transform(v, dim))
            # 2. cca.py:93-106
            if not all(mat.n == mats[0].n for mat in mats):
                raise ValueError("All views must have the same number of samples")
            if not all(mat.p >= self.n_modes for mat in mats):
                raise ValueError("All views must have at least {} features.".format(self.n_modes))
        except Exception:
            for mat in mats:
                mat.free()
            raise
        self._preprocessors = pres
        self.sample_dims = pres[0].sample_dims
        self.n_features_ = [mat.p for mat in mats]
        self.n_samples_ = mats[0].n
        self._mats = mats
        try:
            return self._fit_algorithm(mats)
        except Exception:
            self._free()
            raise

    def _free(self):
        """drop the fitted state and the resident views of an earlier fit"""
        for mat in getattr(self, "_mats", None) or []:
            mat.free()
        self._mats = None
        self.data, self._stats, self._preprocessors = {}, {}, None

    def _pca_views(self, mats):
        """cca.py:167-215: per view the inner PCA, truncated by its cumulative explained-variance ratio; the scores are the
        projection X V (as pop.py here, and for the same reason: `transform` of the training data then reproduces them)
        -> (V32 per view, S32 per view, explained variance per view)"""
        prm, ctx = self._params, self.ctx
        n_pca = process_init_pca_modes(self.init_pca_modes, self.n_samples_, self.n_features_)
        Vs, Ss, evs = [], [], []
        for i, (mat, pre) in enumerate(zip(mats, self._preprocessors)):
            dec = Decomposer.for_model(dict(prm, solver_kwargs=self._solver_kwargs), n_pca[i], ctx)
            dec.fit(mat, total_variance=pre.total_variance)
            ev = dec.s_.astype(np.float64) ** 2 / (mat.n - 1)
            keep, warning = pca_modes_to_keep(ev / pre.total_variance, prm["variance_fraction"])
            if warning:
                print(warning)
            keep = min(keep, ev.size)
            if keep > engine.PCMUL_AMAX:
                raise ValueError(f"the PCA of view {i} kept {keep} modes; CCA takes at most {engine.PCMUL_AMAX} per view: lower "
                                 f"variance_fraction (variance_fraction={prm['variance_fraction']}) or init_pca_modes "
                                 f"(init_pca_modes={self.init_pca_modes[i]})")
            V32, S32 = dec.projected_scores(mat, keep)
            Vs.append(V32)
            Ss.append(S32)
            evs.append(ev[:keep])
        p = sum(V.shape[1] for V in Vs)
        if p > engine.VIEWCOV_PMAX:
            raise ValueError(f"the PCAs of the views kept {p} modes in all; CCA takes at most {engine.VIEWCOV_PMAX}: lower "
                             f"variance_fraction (variance_fraction={prm['variance_fraction']}) or init_pca_modes")
        return Vs, Ss, evs

    def _solve(self, Cd, d, k):
        """the k largest eigenpairs of C x = lam diag(d) x from the device matrix C: host or device by size"""
        p = Cd.shape[0]
        if p <= CCA_HOST_EIG_PMAX:
            lam, x = gevp_diagonal(Cd.cpu().numpy(), d, k)
            return lam, x, "host"
        torch = engine._torch()
        dinv = torch.from_numpy(1.0 / np.sqrt(d)).to(Cd.device)
        lam, Y = torch.linalg.eigh(Cd * dinv[:, None] * dinv[None, :])             # ascending; reads one triangle
        lam, Y = lam[p - k:].flip(0), Y[:, p - k:].flip(1)
        return lam.cpu().numpy(), fix_signs((Y * dinv[:, None]).cpu().numpy()), "device"

    def _xtz(self, mat, R):
        """X^T R for R [n x k] through the X^T Z pass over the resident view"""
        ctx = self.ctx
        k = R.shape[1]
        Rp = engine.panel_import(ctx, np.ascontiguousarray(R, dtype=np.float32), mat.n_pad, engine.panel_width(k))
        out = engine.panel_tmul(ctx, mat, Rp, prec=ctx.precision[1])
        return mat.compact_rows(engine.panel_export(ctx, out, mat.p_phys, k))

    def _fit_algorithm(self, mats):
        """cca.py:307-384 on the resident, preprocessed views"""
        prm, ctx = self._params, self.ctx
        torch = engine._torch()
        m, n, k = self.n_views_, self.n_samples_, int(self.n_modes)
        t0 = time.perf_counter()
        if prm["pca"]:
            Vs, Ss, evs = self._pca_views(mats)
        else:
            if sum(self.n_features_) > engine.VIEWCOV_PMAX:
                raise NotImplementedError(f"CCA without the PCA reduction (pca=False) runs while the views have at most "
                                          f"{engine.VIEWCOV_PMAX} features in all, got {sum(self.n_features_)}; use pca=True")
            Vs, evs = None, None
            Ss = [mat.download() for mat in mats]
        widths = [S.shape[1] for S in Ss]
        off = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
        p = int(off[-1])
        if k > p:
            raise ValueError(f"n_modes = {k} exceeds the {p} columns of the concatenated views")
        Zd = torch.cat([engine.device_panel(ctx, S) for S in Ss], dim=1)          # n x p float32
        t1 = time.perf_counter()
        # 4. C and D
        cov = engine.viewcov(ctx, Zd, off)                                         # m C: the statistics below want it too
        Cd = cov / m
        if prm["pca"]:
            d = shift_diagonal(np.concatenate([(1.0 - c) * ev + c for c, ev in zip(self.c, evs)]), prm["eps"], m)
            t2 = time.perf_counter()
            lam, x, route = self._solve(Cd, d, k)
        else:
            full = engine.viewcov(ctx, Zd, off, keep_diag=True).cpu().numpy()
            D = np.zeros((p, p))
            for i in range(m):
                a, b = off[i], off[i + 1]
                D[a:b, a:b] = (1.0 - self.c[i]) * full[a:b, a:b] + self.c[i] * np.eye(b - a)
            t2 = time.perf_counter()
            lam, x = gevp_dense(Cd.cpu().numpy(), shift_matrix(D, prm["eps"], m), k)
            route = "host"
        t3 = time.perf_counter()
        # 6. weights (feature space, rounded once to float32), loadings, variates, canonical loadings
        xs = [np.ascontiguousarray(x[off[i]:off[i + 1]]) for i in range(m)]
        if prm["pca"]:
            weights = [engine.pcmul(ctx, V, xi, torch.float32).cpu().numpy() for V, xi in zip(Vs, xs)]
        else:
            weights = [xi.astype(np.float32) for xi in xs]
        loadings = [(w.astype(np.float64) / np.linalg.norm(w.astype(np.float64), axis=0)).astype(np.float32) for w in weights]
        variates = [engine.project(ctx, mat, w) for mat, w in zip(mats, weights)]
        can_loadings = [self._xtz(mat, v) for mat, v in zip(mats, variates)]
        # 7. statistics
        transformed = [engine.project(ctx, mat, l) for mat, l in zip(mats, loadings)]
        explained_variance = [t.astype(np.float64).var(axis=0) for t in transformed]
        var1 = Zd.to(torch.float64).var(dim=0, unbiased=True).cpu().numpy()
        total_variance = [float(var1[off[i]:off[i + 1]].sum()) for i in range(m)]
        Td = torch.cat([engine.device_panel(ctx, t) for t in transformed], dim=1)
        covT = engine.viewcov(ctx, Td, np.arange(m + 1) * k).cpu().numpy()         # column i of view v at v k + i
        explained_covariance = np.array([np.linalg.svd(covT[i::k, i::k], compute_uv=False)[0] for i in range(k)])
        if p <= CCA_HOST_EIG_PMAX:
            ev_cov = np.linalg.eigvalsh(cov.cpu().numpy())
        else:
            ev_cov = torch.linalg.eigvalsh(cov).cpu().numpy()
        tec = total_explained_covariance(ev_cov, min(widths))
        t4 = time.perf_counter()
        self.eigvals, self.eigvecs, self.splits = lam, x, off[1:]
        self.data = dict(input_data=mats, pca_data=Ss, weights=weights, loadings=loadings, variates=variates,
                         canonical_loadings=can_loadings, explained_variance=explained_variance,
                         total_variance=total_variance,
                         explained_variance_ratio=[ev / tv for ev, tv in zip(explained_variance, total_variance)],
                         explained_covariance=explained_covariance, total_explained_covariance=tec,
                         explained_covariance_ratio=explained_covariance / tec)
        self._pca_components, self._pca_explained_variance = Vs, evs
        self._stats = dict(eig_route=route, n_pca_modes=widths if prm["pca"] else None, p=p, ms_pca=1e3 * (t1 - t0),
                          ms_viewcov=1e3 * (t2 - t1), ms_eigen=1e3 * (t3 - t2), ms_project=1e3 * (t4 - t3))
        return self

    # ------------------------------------------------------------------ transform
    def transform(self, views):
        """every view through its fitted preprocessing and its weights -> one labelled array of variates per view"""
        self.compute()
        views = list(views)
        if len(views) != self.n_views_:
            raise ValueError(f"the model was fitted on {self.n_views_} views, got {len(views)}")
        out = []
        for pre, w, v in zip(self.preprocessors, self.data["weights"], views):
            mat, fields, vs = pre.transform(v)
            try:
                proj = engine.project(self.ctx, mat, w)
            finally:
                mat.free()
            out.append(pre.inverse_transform_scores(proj, "scores", self.attrs, fields, vs))
        return out

    # ------------------------------------------------------------------ accessors
    def weights(self):
        self.compute()
        return [pre.inverse_transform_components(w, "weights", self.attrs)
                for pre, w in zip(self.preprocessors, self.data["weights"])]

    def components(self, normalize: bool = True):
        """the canonical loadings of every view; `normalize`: as correlations, clipped to [-1, 1] (cca.py:658-682)"""
        self.compute()
        out = []
        for pre, mat, loads, vari in zip(self.preprocessors, self.data["input_data"], self.data["canonical_loadings"],
                                         self.data["variates"]):
            L = loads.astype(np.float64)
            if normalize:
                n = mat.n
                std_x = engine.feature_norms(self.ctx, mat) / np.sqrt(n)           # (the view is centred)
                with np.errstate(divide="ignore", invalid="ignore"):
                    L = np.clip(L / n / std_x[:, None] / vari.astype(np.float64).std(axis=0)[None, :], -1.0, 1.0)
            out.append(pre.inverse_transform_components(L, "components", self.attrs))
        return out

    def scores(self):
        self.compute()
        return [pre.inverse_transform_scores(v, "scores", self.attrs) for pre, v in zip(self.preprocessors, self.data["variates"])]

    def _mode_array(self, values, name, i=0):
        self.compute()
        return labelled.mode_array(values, name, self.attrs, self.preprocessors[i].fields[0].like)

    def explained_variance(self):
        return [self._mode_array(v, "explained_variance", i) for i, v in enumerate(self.data["explained_variance"])]

    def explained_variance_ratio(self):
        return [self._mode_array(v, "explained_variance_ratio", i) for i, v in enumerate(self.data["explained_variance_ratio"])]

    def explained_covariance(self):
        return self._mode_array(self.data["explained_covariance"], "explained_covariance")

    def explained_covariance_ratio(self):
        return self._mode_array(self.data["explained_covariance_ratio"], "explained_covariance_ratio")
