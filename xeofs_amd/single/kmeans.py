"""xeofs_amd.single.KMeans -- weather regimes [Michelangeli, Vautard & Legras 1995, J. Atmos. Sci. 52, 1237-1256]: the samples
of a field are partitioned into k recurrent states by k-means in the space of its leading principal components, from many
random starts, of which the best partition is kept; the classifiability index says how well the starts agree.  Where
ArchetypalAnalysis gives the corners of the data cloud, this gives its centres.  The reference has no such model
(INTEGRATION.md); the definition is stated here in full.

With X [n x P] the engine's preprocessed float32 matrix of the fit (EOF._preprocess: masks, centring, standardising and weights
as in EOF), V [P x q] its q = n_pca_modes leading PCA patterns and S = X V [n x q] the scores that carry the variance
(Decomposer.for_model / projected_scores, float32), Euclidean distance between rows of S is the field's distance, truncated.

    1. seed    R = n_init restarts, each k distinct rows of S by plain k-means++ (Arthur & Vassilvitskii 2007; `kmeanspp_seeds`,
               float64 on the host): all restarts draw from ONE RandomState(random_state) in restart order; the first centre is
               randint(n); each further centre is drawn with probability proportional to D^2 (the squared distance to the
               nearest centre so far) by one random_sample() u and a cumulative search -- the first i whose cumulative D^2
               exceeds u times the total.  `init=` (k distinct sample indices) replaces the seeding and means R = 1.
    2. solve   engine.kmeans_lloyd (csrc/eofx_kmeans.hpp): Lloyd's iteration of all R restarts in ONE launch, every reduction in
               an order fixed by the shape -- assign (float32 fmaf chain of (s - c)^2, the lowest index among equals), stop
               when no label changed, otherwise update (float64 means, an EMPTY CLUSTER KEEPS ITS CENTROID).  One call per
               1000 iterations (a chain of calls equals one long call bit for bit) until every restart has converged or
               `max_iter` updates are done.
    3. pick    the restart of the lowest inertia (the sum of squared distances to the own centroid), the lowest index among
               equals (`best_restart`).
    4. order   the modes by descending population, the lowest index among equals (`mode_order`).

    components()                    V c^T as [P x k] in the input's coordinates and PREPROCESSED units (one engine.pcmul)
    centroids()                     the same through the inverse preprocessing: the field's own units, the mean added back
    labels()                        the mode number 1 .. k of every sample (NaN for a dropped sample)
    scores()                        the one-hot membership [n x k]
    distances()                     the Euclidean PC-space distance of every sample to every centroid (float64, host)
    frequencies()                   counts / n
    inertia()                       of the best restart
    explained_variance_fraction()   1 - inertia / sum S^2
    restart_inertias()              of every restart
    classifiability()               the mean over all ordered pairs of distinct restarts P, Q of min_i max_j cos(p_i, q_j), the
                                    centroids taken in PC space in float64 on the host; NaN for a single restart
    transform(X')                   the fitted preprocessing, engine.project onto V, kmeans_lloyd(max_iter = 0) -> one-hot scores
    inverse_transform(scores)       _pcspace.reconstruct: scores . components^T through the inverse preprocessing -- one-hot
                                    scores return every sample's centroid
    singular_values() and the other SVD-only accessors raise NotImplementedError

Deliberate choices: an empty cluster keeps its centroid (no re-seeding: the run stays a function of its
seeds); plain k-means++ without the greedy trials of scikit-learn; the order of the modes; components() in preprocessed units
against centroids() in the field's own.  Out of scope: the sharded path, the bootstrapper, rotation, complex data, and
clustering without the PCA reduction.  Limits: k <= 32, n_pca_modes <= 32, n <= 262144, n_init <= 4096.

The host steps are module-level functions that need no GPU: check_modes, check_counts, check_init, check_problem,
kmeanspp_seeds, best_restart, mode_order, classifiability.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled
from ..linalg.decomposer import Decomposer
from ..preprocessing import parse_scores
from . import _pcspace
from .eof import EOF

K_MAX = engine.KMEANS_KMAX
Q_MAX = engine.KMEANS_QMAX
N_MAX = engine.KMEANS_NMAX
R_MAX = engine.KMEANS_RMAX
LAUNCH_ITERS = engine.KMEANS_ITER_MAX


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_modes(n_modes) -> int:
    if not _is_int(n_modes) or n_modes < 1:
        raise ValueError(f"KMeans takes a positive integer n_modes, got {n_modes!r}")
    if n_modes > K_MAX:
        raise NotImplementedError(f"KMeans takes at most {K_MAX} modes (the centroids the kernel holds in LDS), got n_modes = {n_modes}")
    return int(n_modes)


def check_counts(n_pca_modes, n_init, max_iter):
    """-> (n_pca_modes, n_init, max_iter) as ints"""
    if not _is_int(n_pca_modes) or n_pca_modes < 1:
        raise ValueError(f"n_pca_modes must be a positive integer, got {n_pca_modes!r}")
    if n_pca_modes > Q_MAX:
        raise NotImplementedError(f"KMeans takes at most {Q_MAX} PCA modes (a row of scores in the registers of a thread), got "
                                  f"n_pca_modes = {n_pca_modes}")
    if not _is_int(n_init) or n_init < 1:
        raise ValueError(f"n_init must be a positive integer, got {n_init!r}")
    if n_init > R_MAX:
        raise NotImplementedError(f"KMeans takes at most {R_MAX} restarts, got n_init = {n_init}")
    if not _is_int(max_iter) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    return int(n_pca_modes), int(n_init), int(max_iter)


def check_init(init, k: int):
    """None, or k distinct non-negative sample indices as an int64 array"""
    if init is None:
        return None
    idx = np.asarray(init)
    if idx.ndim != 1 or idx.size != k or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"init must hold n_modes = {k} integer sample indices, got {init!r}")
    idx = idx.astype(np.int64)
    if np.unique(idx).size != k:
        raise ValueError(f"init must hold distinct sample indices, got {idx.tolist()}")
    if idx.min() < 0:
        raise ValueError(f"init must hold sample indices >= 0, got {idx.tolist()}")
    return idx


def check_problem(n: int, k: int, init=None):
    """the refusals that need the number of samples"""
    if k > n:
        raise ValueError(f"n_modes must be at most the number of samples: n_modes = {k}, n_samples = {n}")
    if n > N_MAX:
        raise NotImplementedError(f"KMeans takes at most {N_MAX} samples (1024 rows per thread of a restart's workgroup), got n_samples = {n}")
    if init is not None and np.max(init) >= n:
        raise ValueError(f"init names sample {int(np.max(init))}, the field has n_samples = {n}")


def kmeanspp_seeds(S, k: int, R: int, random_state=None) -> np.ndarray:
    """[R x k] int64 sample indices: plain k-means++ on the rows of S [n x q] in float64, the R restarts drawing from one
    RandomState(random_state) in restart order.  Per restart: randint(n); then k - 1 times one u = random_sample() and the
    first i with cumsum(D^2)_i > u sum(D^2) (such a row has D^2 > 0: it is none of the centres so far, nor equal to one).
    Where sum(D^2) = 0 -- every row equals a centre -- the lowest index not yet taken."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    rs = np.random.RandomState(random_state)
    idx = np.empty((R, k), dtype=np.int64)
    for r in range(R):
        i = int(rs.randint(n))
        D2 = ((S - S[i]) ** 2).sum(axis=1)
        taken = np.zeros(n, dtype=bool)
        for t in range(k):
            if t:
                u = rs.random_sample()
                cum = np.cumsum(D2)
                if cum[-1] > 0.0:
                    i = min(int(np.searchsorted(cum, u * cum[-1], side="right")), n - 1)
                else:
                    i = int(np.argmin(taken))
                D2 = np.minimum(D2, ((S - S[i]) ** 2).sum(axis=1))
            idx[r, t] = i
            taken[i] = True
    return idx


def best_restart(inertias) -> int:
    """the restart of the lowest inertia, the lowest index among equals"""
    inertias = np.asarray(inertias, dtype=np.float64)
    if inertias.ndim != 1 or inertias.size < 1 or np.isnan(inertias).any():
        raise ValueError(f"one inertia per restart and none of them NaN, got {inertias!r}")
    return int(np.argmin(inertias))                # (argmin: the first of equals)


def mode_order(counts) -> np.ndarray:
    """the modes by descending population, the lowest index among equals"""
    return np.argsort(-np.asarray(counts, dtype=np.int64), kind="stable")


def classifiability(C) -> float:
    """Michelangeli et al. (1995), eq. 6-7, for the centroids C [R x k x q] of R restarts: the mean over all ordered pairs of
    distinct restarts P, Q of c(P, Q) = min_i max_j cos(p_i, q_j) -- 1 where all restarts found the same centroids, in any
    order.  float64; a centroid of norm 0 has cosine 0 with everything; NaN for R < 2."""
    C = np.asarray(C, dtype=np.float64)
    if C.ndim != 3:
        raise ValueError(f"C must be [R x k x q], got shape {C.shape}")
    R = C.shape[0]
    if R < 2:
        return float("nan")
    nrm = np.sqrt((C * C).sum(axis=2, keepdims=True))
    U = np.divide(C, nrm, out=np.zeros_like(C), where=nrm > 0.0)
    cos = np.einsum("aiq,bjq->abij", U, U)          # [R x R x k x k]
    c = cos.max(axis=3).min(axis=2)                 # [R x R]
    return float((c.sum() - np.trace(c)) / (R * (R - 1)))


def _svd_only(what: str):
    def accessor(self, *args, **kwargs):
        raise NotImplementedError(f"KMeans has no {what}: centroids are not singular vectors, "
                                  "explained_variance_fraction() gives the share of the variance the partition holds")

    return accessor


class KMeans(EOF):
    """Weather regimes: k-means of the samples in the space of the leading PCs.  centroids() are the regime states in the
    field's units, components() the same in preprocessed units, labels() the regime of every sample, scores() the one-hot
    membership, frequencies() the share of the samples in every regime, classifiability() the agreement of the restarts."""

    def __init__(self, n_modes: int = 4, n_pca_modes: int = 14, n_init: int = 50, max_iter: int = 300, center: bool = True,
                 standardize: bool = False, use_coslat: bool = False, check_nans=True, sample_name: str = "sample",
                 feature_name: str = "feature", random_state: int | None = None, init=None):
        k = check_modes(n_modes)
        q, R, T = check_counts(n_pca_modes, n_init, max_iter)
        init = check_init(init, k)
        super().__init__(n_modes=k, center=center, standardize=standardize, use_coslat=use_coslat, check_nans=check_nans,
                         sample_name=sample_name, feature_name=feature_name, compute=True, random_state=random_state)
        own = dict(n_pca_modes=q, n_init=R, max_iter=T)
        self.attrs.update({"model": "KMeans weather regimes", **own, "init": "None" if init is None else str(init.tolist())})
        self._params.update({**own, "init": init})
        self._params["solver_kwargs"] = {}

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

    def _solve(self, Sd, C0, max_iter: int):
        """engine.kmeans_lloyd in launches of at most LAUNCH_ITERS updates until every restart has converged or `max_iter`
        updates are done -> (the last launch's result, iterations per restart, converged per restart, launches).  A restart
        that has converged stays where it is in every later launch (its state is a fixed point): only the others count."""
        ctx = self.ctx
        R = C0.shape[0]
        iters, conv = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=bool)
        done = launches = 0
        while True:
            T = min(LAUNCH_ITERS, max_iter - done)
            res = engine.kmeans_lloyd(ctx, Sd, C0, T)
            launches += 1
            iters[~conv] += res["iters"].cpu().numpy()[~conv]
            conv |= res["converged"].cpu().numpy() != 0
            done += T
            if conv.all() or done >= max_iter:
                return res, iters, conv, launches
            C0 = res["centroids"]

    def _fit_algorithm(self, mat, pmat=None, dec=None):
        """the module's algorithm on the resident, preprocessed field `mat`; the inner PCA decomposes its centred twin"""
        torch = engine._torch()
        prm, ctx = self._params, self.ctx
        pmat = mat if pmat is None else pmat
        n, k, init = mat.n, int(self.n_modes), prm["init"]
        check_problem(n, k, init)
        # 1. the inner PCA; the scores are the projection X V
        t0 = time.perf_counter()
        pca = Decomposer.for_model(prm, prm["n_pca_modes"], ctx)
        pca.fit(pmat, total_variance=self.preprocessor.total_variance)
        V32, S32 = pca.projected_scores(mat)
        q = S32.shape[1]
        Sd = engine.device_panel(ctx, S32, "the scores", (torch.float32,))
        ctx.synchronize()
        t1 = time.perf_counter()
        # 2. the seeds
        S64 = np.asarray(S32, dtype=np.float64)
        if not np.isfinite(S64).all():
            raise ValueError("KMeans needs finite PCA scores")
        idx = kmeanspp_seeds(S64, k, prm["n_init"], prm["random_state"]) if init is None else init[None, :]
        C0 = torch.from_numpy(np.ascontiguousarray(np.asarray(S32, dtype=np.float32)[idx])).to(Sd.device)      # R x k x q
        t2 = time.perf_counter()
        # 3. all restarts, all iterations; 4. the best restart; 5. the modes by population
        res, iters, conv, launches = self._solve(Sd, C0, prm["max_iter"])
        inertias = res["inertia"].cpu().numpy()
        best = best_restart(inertias)
        counts = res["counts"][best].cpu().numpy().astype(np.int64)
        order = mode_order(counts)
        Call = res["centroids"].cpu().numpy()                                    # R x k x q float32, PC space
        Cq = np.ascontiguousarray(Call[best][order])
        rank = np.empty(k, dtype=np.int64)
        rank[order] = np.arange(k)
        lab = rank[res["labels"][best].cpu().numpy().astype(np.int64)]           # 0 .. k - 1 in the fitted order
        comps = engine.pcmul(ctx, V32, Cq.T.astype(np.float64), torch.float32).cpu().numpy()      # P x k
        ctx.synchronize()
        t3 = time.perf_counter()
        self.data = dict(input_data=S32, components=np.ascontiguousarray(comps), centroids_pc=Cq, labels=lab, counts=counts[order],
                         inertia=float(inertias[best]), restart_inertias=inertias.copy(), restart_centroids=Call,
                         restart_labels=res["labels"].cpu().numpy(),
                         total_ss=float((S64 * S64).sum()), best=best, mode_order=order)
        self._pca_scores, self._pca_components = S32, V32
        self.stats = dict(route=pca.route_, n_pca_modes=q, ms_pca=1e3 * (t1 - t0), ms_seed=1e3 * (t2 - t1), ms_lloyd=1e3 * (t3 - t2),
                          iterations=iters, converged=conv, launches=launches, n_empty=int((counts == 0).sum()), best=best,
                          seeds=np.asarray(idx, dtype=np.int64))
        return self

    # ------------------------------------------------------------------ transform / inverse
    def _one_hot(self, lab) -> np.ndarray:
        k = int(self.n_modes)
        out = np.zeros((lab.size, k), dtype=np.float32)
        ok = lab >= 0
        out[np.nonzero(ok)[0], lab[ok]] = 1.0
        return out

    def transform(self, X):
        """new data -> the fitted preprocessing -> PC space (engine.project onto V) -> the assignment alone
        (kmeans_lloyd with max_iter = 0) against the fitted centroids -> one-hot scores"""
        self.compute()
        mat, fields, vs = self.preprocessor.transform(X)
        try:
            proj = engine.project(self.ctx, mat, self._pca_components)             # n' x q float32
        finally:
            mat.free()
        res = engine.kmeans_lloyd(self.ctx, proj, self.data["centroids_pc"][None], 0)
        lab = res["labels"][0].cpu().numpy().astype(np.int64)
        return self.preprocessor.inverse_transform_scores(self._one_hot(lab), "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores):
        """scores [.., mode] -> scores . components^T (_pcspace.reconstruct) through the inverse preprocessing: one-hot scores
        return every sample's centroid"""
        self.compute()
        S, modes, vs, fields = parse_scores(scores, self.preprocessor.fields, np.float64, scalar_mode=True)
        C = self.data["components"][:, modes - 1]
        Z = engine.device_panel(self.ctx, np.ascontiguousarray(S, dtype=np.float64))
        return self.preprocessor.inverse_transform_data(_pcspace.reconstruct(self.ctx, Z, C), "reconstructed_data", fields, vs)

    # ------------------------------------------------------------------ accessors
    def components(self):
        """V c^T: the centroids in feature space and preprocessed units, as (mode, features)"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def centroids(self):
        """the centroids in the field's own units: components() through the inverse preprocessing (weights, deviation, mean)"""
        pre = self.preprocessor
        vf = pre.valid_feature
        Z = self.data["components"].astype(np.float64).T          # [k x p]
        if pre.feature_weights is not None:
            Z = Z / pre.feature_weights[vf]
        if pre.std_ is not None:
            Z = Z * pre.std_[vf]
        if pre.mean_ is not None:
            Z = Z + pre.mean_[vf]
        return pre.inverse_transform_components(np.ascontiguousarray(Z.T), "centroids", self.attrs)

    def labels(self):
        """the mode number 1 .. k of every sample over the sample dimensions (float64: NaN for a dropped sample)"""
        self.compute()
        pre = self.preprocessor
        f, vs = pre.fields[0], pre.valid_sample
        full = np.full(vs.size, np.nan)
        full[vs] = self.data["labels"] + 1.0
        coords = {d: f.coords[d] for d in f.sample_dims}
        return labelled.pack(full.reshape(f.sample_shape), tuple(f.sample_dims), coords, "labels", dict(self.attrs), f.like)

    def scores(self):
        """the one-hot membership of every sample"""
        self.compute()
        return self.preprocessor.inverse_transform_scores(self._one_hot(self.data["labels"]), "scores", self.attrs)

    def distances(self):
        """the Euclidean PC-space distance of every sample to every centroid (float64 on the host)"""
        self.compute()
        S = np.asarray(self._pca_scores, dtype=np.float64)
        C = self.data["centroids_pc"].astype(np.float64)
        D = np.sqrt(((S[:, None, :] - C[None, :, :]) ** 2).sum(axis=2))
        return self.preprocessor.inverse_transform_scores(D, "distances", self.attrs)

    def frequencies(self):
        self.compute()
        return self._mode_array(self.data["counts"] / float(self.data["labels"].size), "frequencies")

    def inertia(self) -> float:
        self.compute()
        return self.data["inertia"]

    def explained_variance_fraction(self) -> float:
        """1 - inertia / sum S^2"""
        self.compute()
        return 1.0 - self.data["inertia"] / self.data["total_ss"]

    def restart_inertias(self) -> np.ndarray:
        self.compute()
        return self.data["restart_inertias"].copy()

    def classifiability(self) -> float:
        self.compute()
        return classifiability(self.data["restart_centroids"])

    singular_values = _svd_only("singular values")
    explained_variance = _svd_only("explained variance per mode")
    explained_variance_ratio = _svd_only("explained variance ratio per mode")
