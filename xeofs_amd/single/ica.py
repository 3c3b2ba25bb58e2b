"""xeofs_amd.single.ICA -- independent component analysis of a field [Hyvarinen & Oja 2000, Neural Networks 13, 411-430;
Aires, Chedin & Nadal 2000, J. Geophys. Res. 105, 17437; Hannachi, Unkel, Trendafilov & Jolliffe 2009, J. Climate 22, 2797]: the
leading principal components are rotated towards statistical INDEPENDENCE of their time series, where varimax / promax
(EOFRotator) rotate towards simplicity of the patterns.  The reference has no such model; the definition is
stated here in full.

With X [n x P] the engine's preprocessed, centred float32 matrix of the fit (EOF._preprocess), V [P x q] its q = n_modes leading
PCA patterns, S = X V [n x q] the scores (Decomposer.for_model / projected_scores, float32) and sigma_j the norm of score j:

    1. whiten   Z = S diag(sqrt(n) / sigma_j) in float32 (both factors rounded to float32 first), so that Z^T Z / n = I up to
                the correlation the projection leaves.  A score of norm 0, or scores that are rank deficient by the rule of
                _pcspace.whitened_modes, raise LinAlgError.
    2. starts   R = n_init restarts, each normal(size=(q, q)) from ONE RandomState(random_state) in restart order (with
                n_init = 1 scikit-learn's own draw), decorrelated on the host in float64: (W W^T)^-1/2 W by engine.host_eigh
                (`ica_starts`).  `w_init` ([q x q] or [R x q x q]) replaces the draw.
    3. solve    engine.fastica (csrc/eofx_ica.hpp): the parallel fixed-point iteration of all restarts on the device,
                    W1 = E[g(W z) z^T] - diag(E[g'(W z)]) W,   W <- (W1 W1^T)^-1/2 W1,
                projection and contrast in float32, moments and decorrelation in float64, every sum in an order fixed by the
                shape; a restart stops when lim = max_j | |w_j^new . w_j| - 1 | < tol (scikit-learn's rule) or is degenerate
                (W1 not of full rank).  One call per ICA_ITER_MAX = 64 iterations until no restart is running or `max_iter`
                iterations are done.  fun = "logcosh" (g = tanh(alpha s), 1 <= alpha <= 2), "exp" (g = s exp(-s^2 / 2)) or
                "cube" (g = s^3).
    4. contrast one more moment pass gives E[G(s_j)] at the final W; the contrast of a restart is sum_j (E[G(s_j)] - gamma)^2
                with gamma = E[G(nu)], nu standard normal: 3/4 (cube), -1/sqrt(2) (exp), 64-point Gauss-Hermite (logcosh)
                (`ica_gamma`).  Its terms are the negentropy approximation of Hyvarinen (1998) up to a constant.
    5. pick     the restart of the highest contrast among those not degenerate, the lowest index among equals
                (`best_restart`); LinAlgError if all are degenerate; a warning if the chosen one has not converged.
    6. carry    with D = diag(sigma_j / sqrt(n)): Vq = D^-1 W^T, Wq = D W^T through _pcspace.signed_projection: components
                V Wq (the mixing patterns), filter patterns V Vq, sources S Vq of unit variance; one sign per mode by the
                project's rule on the component.  The modes by descending explained variance sum_i lambda_i w_ji^2, lambda_i the
                PCA mode's explained variance as EOF reports it, the lowest index among equals (`mode_order`).

    components()                 the mixing patterns [P x q], preprocessed units:  X ~ scores . components^T
    filter_patterns()            scores = X . filter_patterns
    scores()                     the independent sources, unit variance, zero mean
    explained_variance(), explained_variance_ratio()
    mixing_matrix()              Wq [q PCs x q modes];  negentropy() per mode;  restart_contrasts();  whitened()  Z
    transform(X')                _pcspace.project_modes with Vq;  inverse_transform(scores)  _pcspace.reconstruct
    singular_values() and the other SVD-only accessors raise NotImplementedError

Out of scope: spatial ICA (independent MAPS: it needs a re-centred, re-whitened V and discards a uniform term), the sharded
path, the bootstrapper, complex data, and the deflation variant of FastICA.  Limits: n_modes <= 32, n <= 4194304,
n_init <= 1024.

The host steps are module-level functions that need no GPU: check_args, check_w_init, ica_starts, ica_gamma, restart_contrast,
best_restart, mode_order.
"""

from __future__ import annotations

import time
import warnings

import numpy as np

from .. import engine, labelled, spca
from ..linalg.decomposer import Decomposer
from ..preprocessing import parse_scores
from . import _pcspace
from .eof import EOF

Q_MAX = engine.ICA_QMAX
N_MAX = engine.ICA_NMAX
R_MAX = engine.ICA_RMAX
CALL_ITERS = engine.ICA_ITER_MAX
FUNS = engine.ICA_FUNS


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_args(n_modes, fun, alpha, tol, max_iter, n_init):
    """-> (n_modes, fun, alpha, tol, max_iter, n_init), checked"""
    if not _is_int(n_modes) or n_modes < 1:
        raise ValueError(f"ICA takes a positive integer n_modes, got {n_modes!r}")
    if n_modes > Q_MAX:
        raise NotImplementedError(f"ICA takes at most {Q_MAX} modes (a row of scores in the registers of a thread), got n_modes = {n_modes}")
    if fun not in FUNS:
        raise ValueError(f"fun must be one of {FUNS}, got {fun!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 1.0 <= alpha <= 2.0:
        raise ValueError(f"alpha must lie in [1, 2], got {alpha!r}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not 0.0 < tol <= 1.0:
        raise ValueError(f"tol must lie in (0, 1], got {tol!r}")
    if not _is_int(max_iter) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not _is_int(n_init) or n_init < 1:
        raise ValueError(f"n_init must be a positive integer, got {n_init!r}")
    if n_init > R_MAX:
        raise NotImplementedError(f"ICA takes at most {R_MAX} restarts, got n_init = {n_init}")
    return int(n_modes), fun, float(alpha), float(tol), int(max_iter), int(n_init)


def check_w_init(w_init, q: int, n_init: int):
    """None, or the starts as a float64 array [R x q x q] (a single [q x q] is R = 1); R must equal n_init"""
    if w_init is None:
        return None
    W = np.asarray(w_init, dtype=np.float64)
    if W.ndim == 2:
        W = W[None]
    if W.ndim != 3 or W.shape[1:] != (q, q):
        raise ValueError(f"w_init must be [q x q] or [R x q x q] with q = n_modes = {q}, got shape {np.shape(w_init)}")
    if W.shape[0] != n_init:
        raise ValueError(f"w_init holds {W.shape[0]} starts, n_init = {n_init}")
    if not np.isfinite(W).all():
        raise ValueError("w_init holds a NaN or an infinity")
    return np.ascontiguousarray(W)


def _decorrelate(W: np.ndarray) -> np.ndarray:
    """(W W^T)^-1/2 W in float64 on the host (engine.host_eigh)"""
    d, E = engine.host_eigh(W @ W.T)
    if not d[-1] > 0.0:
        raise np.linalg.LinAlgError("a start of ICA is singular")
    return np.linalg.multi_dot([E / np.sqrt(d), E.T, W])


def ica_starts(q: int, R: int, random_state=None, w_init=None) -> np.ndarray:
    """[R x q x q] orthogonal starts: normal(size=(q, q)) per restart from one RandomState(random_state) in restart order, or
    `w_init`, each decorrelated"""
    if w_init is None:
        rs = np.random.RandomState(random_state)
        w_init = np.stack([rs.normal(size=(q, q)) for _ in range(R)])
    return np.ascontiguousarray(np.stack([_decorrelate(W) for W in w_init]))


def ica_gamma(fun: str, alpha: float = 1.0) -> float:
    """E[G(nu)] for a standard normal nu"""
    if fun == "cube":
        return 0.75
    if fun == "exp":
        return -1.0 / np.sqrt(2.0)
    x, w = np.polynomial.hermite.hermgauss(64)
    u = np.abs(alpha * np.sqrt(2.0) * x)
    return float((w * (u + np.log1p(np.exp(-2.0 * u)) - np.log(2.0)) / alpha).sum() / np.sqrt(np.pi))


def restart_contrast(gmean, fun: str, alpha: float = 1.0) -> np.ndarray:
    """sum_j (gmean_rj - gamma)^2 per restart, gmean [R x q]"""
    return ((np.asarray(gmean, dtype=np.float64) - ica_gamma(fun, alpha)) ** 2).sum(axis=-1)


def best_restart(contrasts, status) -> int:
    """the restart of the highest contrast among those whose status is not 2, the lowest index among equals"""
    c = np.array(contrasts, dtype=np.float64)
    status = np.asarray(status)
    if c.ndim != 1 or c.shape != status.shape or c.size < 1:
        raise ValueError("one contrast and one status per restart")
    live = status != 2
    if not live.any():
        raise np.linalg.LinAlgError("every restart of ICA is degenerate: the update W1 lost rank")
    if np.isnan(c[live]).any():
        raise ValueError(f"a contrast is NaN: {c!r}")
    c[~live] = -np.inf
    return int(np.argmax(c))                           # (argmax: the first of equals)


def mode_order(ev) -> np.ndarray:
    """the modes by descending explained variance, the lowest index among equals"""
    return np.argsort(-np.asarray(ev, dtype=np.float64), kind="stable")


def _svd_only(what: str):
    def accessor(self, *args, **kwargs):
        raise NotImplementedError(f"ICA has no {what}: independent components are not singular vectors")

    return accessor


class ICA(EOF):
    """Independent component analysis (temporal ICA by parallel FastICA in the space of the leading PCs): scores() are the
    independent sources of unit variance, components() their mixing patterns, filter_patterns() the maps that extract them."""

    def __init__(self, n_modes: int = 2, fun: str = "logcosh", alpha: float = 1.0, tol: float = 1e-4, max_iter: int = 200,
                 n_init: int = 1, w_init=None, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 check_nans=True, sample_name: str = "sample", feature_name: str = "feature", solver: str = "auto",
                 random_state: int | None = None, solver_kwargs: dict = {}):
        q, fun, alpha, tol, T, R = check_args(n_modes, fun, alpha, tol, max_iter, n_init)
        if not center:
            raise ValueError("ICA needs center=True: the sources of FastICA are centred")
        w_init = check_w_init(w_init, q, R)
        super().__init__(n_modes=q, center=True, standardize=standardize, use_coslat=use_coslat, check_nans=check_nans,
                         sample_name=sample_name, feature_name=feature_name, compute=True, random_state=random_state, solver=solver,
                         solver_kwargs=solver_kwargs)
        own = dict(fun=fun, alpha=alpha, tol=tol, max_iter=T, n_init=R)
        self.attrs.update({"model": "ICA", **own, "w_init": "None" if w_init is None else "given"})
        self._params.update({**own, "w_init": w_init})
        self._params["solver_kwargs"] = dict(solver_kwargs)

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        mat = self._preprocess(X, dim, weights)
        try:
            return self._fit_algorithm(mat)
        finally:
            mat.free()

    def _solve(self, Zd, W0):
        """engine.fastica in calls of at most CALL_ITERS iterations until no restart is running or `max_iter` iterations are
        done, then the moment pass alone at the final W -> (W, status, iters, gmean, lim as host arrays, calls)"""
        torch = engine._torch()
        prm, ctx = self._params, self.ctx
        R = W0.shape[0]
        W = torch.from_numpy(W0).to(Zd.device)
        status = torch.zeros(R, dtype=torch.int32, device=Zd.device)
        iters = torch.zeros(R, dtype=torch.int32, device=Zd.device)
        lim = torch.full((R,), float("nan"), dtype=torch.float64, device=Zd.device)
        kw = dict(fun=prm["fun"], alpha=prm["alpha"], tol=prm["tol"])
        done = calls = 0
        while done < prm["max_iter"]:
            T = min(CALL_ITERS, prm["max_iter"] - done)
            engine.fastica(ctx, Zd, W, status, iters, max_iter=T, out=dict(lim=lim), want=(), **kw)
            calls, done = calls + 1, done + T
            if bool((status != 0).all()):
                break
        res = engine.fastica(ctx, Zd, W, status, iters, max_iter=0, want=("gmean",), **kw)
        return (W.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy(), res["gmean"].cpu().numpy(), lim.cpu().numpy(), calls + 1)

    def _fit_algorithm(self, mat, dec=None):
        """the module's algorithm on the resident, centred, preprocessed field `mat`"""
        torch = engine._torch()
        prm, ctx = self._params, self.ctx
        n, q = mat.n, int(self.n_modes)
        if n > N_MAX:
            raise NotImplementedError(f"ICA takes at most {N_MAX} samples, got n_samples = {n}")
        # 1. the inner PCA; the scores are the projection X V
        t0 = time.perf_counter()
        pca = Decomposer.for_model(prm, q, ctx)
        pca.fit(mat, total_variance=self.preprocessor.total_variance)
        V32, S32 = pca.projected_scores(mat)
        if S32.shape[1] != q:
            raise ValueError(f"the PCA kept {S32.shape[1]} modes, ICA needs n_modes = {q}")
        lam = pca.s_.astype(np.float64)[:q] ** 2 / (n - 1)
        Sd = engine.device_panel(ctx, S32, "the scores", (torch.float32,))
        S64 = Sd.to(torch.float64)
        C = engine.lagcov(ctx, Sd, np.array([1.0])).cpu().numpy()                     # S^T S in float64
        if not np.isfinite(C).all():
            raise ValueError("ICA needs finite PCA scores")
        sigma = np.sqrt(np.diag(C))
        d, _ = engine.host_eigh(0.5 * (C + C.T))                                    # descending
        if not sigma.min() > 0.0 or not d[-1] > 0.0 or np.sqrt(d[-1]) <= max(n, q) * np.finfo(np.float32).eps * np.sqrt(d[0]):
            raise np.linalg.LinAlgError(f"the PCA scores are rank deficient: fewer independent modes than n_modes={q}")
        # 2. whiten
        scale = (np.sqrt(n) / sigma).astype(np.float32)
        Zd = (Sd * torch.from_numpy(scale).to(Sd.device)).contiguous()
        ctx.synchronize()
        t1 = time.perf_counter()
        # 3. the starts; 4. all restarts; 5. contrast and pick
        W0 = ica_starts(q, prm["n_init"], prm["random_state"], prm["w_init"])
        W, status, iters, gmean, lim, calls = self._solve(Zd, W0)
        cons = restart_contrast(gmean, prm["fun"], prm["alpha"])
        best = best_restart(cons, status)
        converged = bool(status[best] == 1)
        if not converged:
            warnings.warn(f"FastICA did not converge in {int(iters[best])} iterations (lim = {lim[best]:.3g}, tol = {prm['tol']:g}): "
                          "consider increasing tol or max_iter")
        t2 = time.perf_counter()
        # 6. carry back, ordered by explained variance
        Wb = W[best]
        ev = (Wb * Wb) @ lam
        order = mode_order(ev)
        dd = sigma / np.sqrt(n)
        Vq = np.ascontiguousarray((Wb.T / dd[:, None])[:, order])
        Wq = np.ascontiguousarray((Wb.T * dd[:, None])[:, order])
        proj, sg = _pcspace.signed_projection(lambda X, B: spca.spca_rowmul(ctx, X, B), spca._dev64(ctx, V32), S64, Vq, Wq)
        ctx.synchronize()
        t3 = time.perf_counter()
        neg = (gmean[best] - ica_gamma(prm["fun"], prm["alpha"])) ** 2
        self.data = dict(input_data=S32, **proj, explained_variance=ev[order], total_variance=self.preprocessor.total_variance,
                         mixing_matrix=Wq * sg, negentropy=neg[order], restart_contrasts=cons.copy(),
                         starts=W0, unmixing=Wb.copy(), restart_unmixing=W, sigma=sigma, pca_explained_variance=lam, best=best,
                         mode_order=order)
        self._Vq = Vq * sg
        self._whitened = Zd                             # (stays on the device: whitened() copies it on demand)
        self._pca_scores, self._pca_components = S32, V32
        self.stats = dict(route=pca.route_, ms_pca=1e3 * (t1 - t0), ms_ica=1e3 * (t2 - t1), ms_project=1e3 * (t3 - t2), iterations=iters,
                          status=status, lim=lim, converged=converged, calls=calls, best=best)
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X):
        """new data -> the fitted preprocessing -> PC space (engine.project onto V) -> the product with Vq -> sources"""
        self.compute()
        Zs, fields, vs = _pcspace.project_modes(self, X, self._Vq, engine._torch().float32)
        return self.preprocessor.inverse_transform_scores(Zs, "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores):
        """scores [.., mode] -> scores . components^T (_pcspace.reconstruct) through the inverse preprocessing"""
        self.compute()
        S, modes, vs, fields = parse_scores(scores, self.preprocessor.fields, np.float64, scalar_mode=True)
        C = self.data["components"][:, modes - 1]
        Z = engine.device_panel(self.ctx, np.ascontiguousarray(S, dtype=np.float64))
        return self.preprocessor.inverse_transform_data(_pcspace.reconstruct(self.ctx, Z, C), "reconstructed_data", fields, vs)

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the mixing patterns: X ~ scores . components^T, as (mode, features) in preprocessed units"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def filter_patterns(self):
        """scores = X . filter_patterns"""
        return self.preprocessor.inverse_transform_components(self.data["filter_patterns"], "filter_patterns", self.attrs)

    def scores(self):
        """the independent sources: unit variance (1 / n), zero mean"""
        self.compute()
        return self.preprocessor.inverse_transform_scores(self.data["scores"], "scores", self.attrs)

    def mixing_matrix(self) -> np.ndarray:
        """Wq [q PCA modes x q modes]: components = V Wq"""
        self.compute()
        return self.data["mixing_matrix"].copy()

    def negentropy(self):
        """(E[G(s_j)] - gamma)^2 per mode"""
        self.compute()
        return self._mode_array(self.data["negentropy"], "negentropy")

    def whitened(self) -> np.ndarray:
        """the white float32 panel Z [n x q] the solver ran on, copied from the device on demand"""
        self.compute()
        return self._whitened.cpu().numpy()

    def restart_contrasts(self) -> np.ndarray:
        self.compute()
        return self.data["restart_contrasts"].copy()

    singular_values = _svd_only("singular values")
