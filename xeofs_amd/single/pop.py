"""xeofs_amd.single.POP -- drop-in for xeofs.single.POP (xeofs/single/pop.py:14-498): principal oscillation pattern analysis
[Hasselmann 1988; von Storch et al. 1995], the eigenmodes of the feedback matrix of a field in the space of its leading PCs.

With V [P x q] the PCA patterns of the preprocessed field X and S = X V [n x q] its PCA scores (U s, not rescaled; taken
as the projection, as the reference's PCA does and as `transform` does for new data),

    C0 = S[:-1]^T S[:-1],   C1 = S[1:]^T S[:-1],   A = C1 C0^-1,   A Pq = Pq diag(lam),
    damping_times = -1 / log|lam|,   periods = 2 pi / arg(lam)   (inf for a positive real lam),

the POP coefficients of mode j are the least-squares coordinates of every sample in the plane spanned by Re p_j and Im p_j
(von Storch et al. 1995, eq. 19; pop.py:185-198): with G_j the 2 x 2 Gram matrix of (Re p_j, Im p_j),
[Re z_j; Im z_j] = G_j^+ [Re p_j, Im p_j]^T s_t.  The reference loops over the modes; here the q pseudo-inverses fold into one
real matrix W [q x 2q] (`pop_coefficient_matrix`), so Z = S W is one product with the output [Re | Im].

C0 and C1 are two calls of the lag-covariance kernel (engine.lagcov, csrc/eofx_lagcov.hpp); the q x q algebra and the
nonsymmetric eigenproblem run in float64 on the host (numpy.linalg.eig); Z = S W and the patterns V [Re Pq | Im Pq] are
products of a tall panel with a small matrix of inner length q on the fp64 matrix cores (engine.pcmul,
csrc/eofx_pcmul.hpp): the scores stay float64, the patterns are rounded once to float32.

Deliberate deviations from the reference:
  1. `n_modes` does not truncate, as in the reference: the model returns the q modes the PCA kept (q <= 1024);
  2. every eigenvector has unit 2-norm in PC space and is rotated so that its entry of largest modulus is real and positive
     (the lowest index on ties); LAPACK fixes the norm and leaves that phase open.  The two members of a conjugate pair are
     exact conjugates;
  3. the modes are ordered by `norms` descending; a conjugate pair has equal norms, and its member with Im lam > 0 comes
     first.  The reference's argsort leaves that tie to chance;
  4. feature-space POP (`use_pca=False`, a P x P inverse) is not built: NotImplementedError.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled
from ..linalg.decomposer import Decomposer
from ..preprocessing import parse_scores
from . import _pcspace
from .eof import EOF, NO_EXPLAINED_VARIANCE, NO_SINGULAR_VALUES, ComplexEOF

POP_QMAX = engine.PCMUL_AMAX          # PCA modes the PC-space product takes


# ---------------------------------------------------------------------------------------------------- host algebra
def pop_normalize(Pq: np.ndarray) -> np.ndarray:
    """every column scaled to unit 2-norm and rotated so that its entry of largest modulus (lowest index on ties) is real
    and positive"""
    Pq = np.array(Pq, dtype=np.complex128)
    Pq /= np.linalg.norm(Pq, axis=0)
    top = np.argmax(np.abs(Pq), axis=0)                       # (the first of equal maxima)
    pivot = Pq[top, np.arange(Pq.shape[1])]
    Pq *= np.conj(pivot) / np.abs(pivot)
    Pq[top, np.arange(Pq.shape[1])] = np.abs(pivot)           # exactly real
    return Pq


def pop_pair_conjugates(lam: np.ndarray, Pq: np.ndarray):
    """-> (lam, Pq, partner): the eigenvalues of a real matrix come in conjugate pairs, which LAPACK returns next to each
    other; the second member of every pair is overwritten with the exact conjugate of the first.  partner[j] = the index of
    the other member, j itself for a real mode."""
    lam, Pq = np.array(lam, dtype=np.complex128), np.array(Pq, dtype=np.complex128)
    q = lam.size
    partner = np.arange(q)
    j = 0
    while j < q:
        if lam[j].imag != 0.0 and j + 1 < q and lam[j + 1].imag != 0.0 and partner[j] == j:
            if abs(lam[j + 1] - np.conj(lam[j])) <= 1e-12 * abs(lam[j]):
                lam[j + 1], Pq[:, j + 1] = np.conj(lam[j]), np.conj(Pq[:, j])
                partner[j], partner[j + 1] = j + 1, j
                j += 2
                continue
        j += 1
    return lam, Pq, partner


def pop_coefficient_matrix(Pq: np.ndarray) -> np.ndarray:
    """W [q x 2q] with S W = [Re Z | Im Z], Z the POP coefficients of pop.py:185-198: per mode, with pr = Re p, pi = Im p and
    G = [[pr.pr, pr.pi], [pr.pi, pi.pi]], columns j and q + j of W are the two rows of G^+ [pr, pi]^T.  G^+ in closed form:
    the inverse where G has rank two; G / trace(G)^2 where it has rank one (a real or a purely rotated-real eigenvector;
    numpy's pinv drops a singular value below 1e-15 of the largest, which is det(G) <= 1e-15 trace(G)^2 here)."""
    Pq = np.asarray(Pq, dtype=np.complex128)
    q = Pq.shape[1]
    pr, pi = Pq.real, Pq.imag
    a, b, c = (pr * pr).sum(axis=0), (pr * pi).sum(axis=0), (pi * pi).sum(axis=0)
    det, tr = a * c - b * b, a + c
    full = det > 1e-15 * tr * tr
    d = np.where(full, det, 1.0)
    t2 = tr * tr
    g00 = np.where(full, c / d, a / t2)
    g01 = np.where(full, -b / d, b / t2)
    g11 = np.where(full, a / d, c / t2)
    W = np.empty((Pq.shape[0], 2 * q))
    W[:, :q] = pr * g00 + pi * g01
    W[:, q:] = pr * g01 + pi * g11
    return W


def pop_order(norms: np.ndarray, lam: np.ndarray, partner: np.ndarray | None = None) -> np.ndarray:
    """the order of the modes: `norms` descending; the two members of a conjugate pair (equal norms) stay together, the one
    with Im lam > 0 first; other ties keep the order they came in"""
    norms, lam = np.asarray(norms, dtype=np.float64), np.asarray(lam, dtype=np.complex128)
    q = norms.size
    if partner is None:
        partner = np.arange(q)
        for j in range(q):
            if lam[j].imag != 0.0 and partner[j] == j:
                hit = [i for i in range(q) if i != j and partner[i] == i and lam[i] == np.conj(lam[j])]
                if hit:
                    partner[j], partner[hit[0]] = hit[0], j
    shared = np.maximum(norms, norms[partner])
    first = np.minimum(np.arange(q), partner)
    return np.array(sorted(range(q), key=lambda j: (-shared[j], first[j], -lam[j].imag)), dtype=np.int64)


def pop_times(lam: np.ndarray):
    """-> (damping_times, periods) = (-1 / log|lam|, 2 pi / arg(lam)); the period of a positive real eigenvalue is inf"""
    lam = np.asarray(lam, dtype=np.complex128)
    with np.errstate(divide="ignore"):
        return -1.0 / np.log(np.abs(lam)), 2.0 * np.pi / np.angle(lam)


def pop_solve(C0: np.ndarray, C1: np.ndarray):
    """the feedback matrix A = C1 C0^-1 (a solve with the Cholesky-checked, symmetrised C0) and its normalised eigenpairs
    -> (lam, Pq, partner)"""
    C0 = 0.5 * (C0 + C0.T)
    try:
        np.linalg.cholesky(C0)
    except np.linalg.LinAlgError:
        raise np.linalg.LinAlgError("the covariance of the PCA scores is not positive definite: fewer independent modes than "
                                    f"the {C0.shape[0]} PCA modes kept") from None
    A = np.linalg.solve(C0, C1.T).T
    lam, Pq = np.linalg.eig(A)
    lam, Pq, partner = pop_pair_conjugates(lam, pop_normalize(Pq))
    return lam, Pq, partner


class POP(EOF):
    """Drop-in for xeofs.single.POP (xeofs/single/pop.py:14-498).  components() are the POPs (complex patterns), scores() the
    POP coefficients (complex time series), eigenvalues() / damping_times() / periods() describe the feedback matrix."""

    def __init__(self, n_modes: int = 2, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 use_pca: bool = True, n_pca_modes: float | int | str = 0.999, pca_init_rank_reduction: float = 0.3,
                 check_nans=True, sample_name: str = "sample", feature_name: str = "feature", compute: bool = True,
                 random_state: int | None = None, solver: str = "auto", solver_kwargs: dict = {}, **kwargs):
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs, **kwargs)
        self.attrs.update({"model": "Principal Oscillation Pattern analysis"})
        self._params.update({"use_pca": use_pca, "n_pca_modes": n_pca_modes,
                             "pca_init_rank_reduction": pca_init_rank_reduction})
        self._params["solver_kwargs"] = dict(solver_kwargs)
        self.preprocessor.masked_ok = False

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if not self._params["use_pca"]:
            raise NotImplementedError("POP without the PCA reduction (use_pca=False) needs the inverse of a feature x feature "
                                      "covariance and is not implemented; use use_pca=True")
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        mat = self._preprocess(X, dim, weights)
        try:
            return self._fit_algorithm(mat)
        finally:
            mat.free()

    def _fit_algorithm(self, mat, omega=None, dec=None):
        """pop.py:159-253 on the resident, preprocessed field"""
        prm, ctx = self._params, self.ctx
        torch = engine._torch()
        n = mat.n
        if n < 3:
            raise ValueError(f"POP needs at least 3 samples (two lagged pairs), got n_samples = {n}")
        # 1. inner PCA (pop.py:138-147, 205): scores U s, not rescaled
        t0 = time.perf_counter()
        n_pca = prm["n_pca_modes"]
        if isinstance(n_pca, str):
            if n_pca != "all":
                raise ValueError("`n_pca_modes` must be an integer, float or 'all'")
            n_pca = min(mat.n, mat.p)
        pca = Decomposer.for_model(prm, n_pca, ctx, init_rank_reduction=prm["pca_init_rank_reduction"])
        pca.fit(mat, total_variance=self.preprocessor.total_variance)
        V32, S32 = pca.projected_scores(mat)
        q = S32.shape[1]
        if q > POP_QMAX:
            raise ValueError(f"the PCA kept {q} modes; POP takes at most {POP_QMAX}: lower n_pca_modes "
                             f"(n_pca_modes={prm['n_pca_modes']})")
        t1 = time.perf_counter()
        # 2. C0 = S[:-1]^T S[:-1] and C1 = S[1:]^T S[:-1], one kernel call each
        Sd = engine.device_panel(ctx, S32)
        C0 = engine.lagcov(ctx, Sd[:n - 1], np.array([1.0])).cpu().numpy()
        C1 = engine.lagcov(ctx, Sd, np.array([0.0, 1.0])).cpu().numpy().T          # (sum_t s_t s_{t+1}^T)^T
        t2 = time.perf_counter()
        # 3. feedback matrix and its eigenmodes, 4. the coefficient matrix (host, float64)
        lam, Pq, partner = pop_solve(C0, C1)
        W = pop_coefficient_matrix(Pq)
        t3 = time.perf_counter()
        # 4. Z = S W, 5. norms = sqrt(var Z) (ddof = 0) on the device in float64
        Z = engine.pcmul(ctx, Sd, W)                                               # n x 2q float64, [Re | Im]
        Zc = Z - Z.mean(dim=0)
        sq = (Zc * Zc).mean(dim=0)
        norms = torch.sqrt(sq[:q] + sq[q:]).cpu().numpy()
        order = pop_order(norms, lam, partner)
        # 6. total variance of the PCA scores (linalg/utils.py:4-6)
        Sd64 = Sd.to(torch.float64)
        total_variance = float((Sd64 * Sd64).sum()) / (n - 1)
        # 7. components V [Re Pq | Im Pq], rounded once to float32
        Cd = engine.pcmul(ctx, V32, np.concatenate([Pq.real, Pq.imag], axis=1), torch.float32)
        Zh, Ch = Z.cpu().numpy(), Cd.cpu().numpy()
        scores = (Zh[:, :q] + 1j * Zh[:, q:])[:, order]
        comps = np.empty((Ch.shape[0], q), np.complex64)
        comps.real, comps.imag = Ch[:, :q][:, order], Ch[:, q:][:, order]
        lam, Pq = lam[order], Pq[:, order]
        tau, T = pop_times(lam)
        self.data = dict(input_data=S32, components=comps, scores=scores, norms=norms[order], eigenvalues=lam,
                         damping_times=tau, periods=T, total_variance=total_variance)
        self._Pq, self._W = Pq, pop_coefficient_matrix(Pq)
        self._pca_scores, self._pca_components = S32, V32
        t4 = time.perf_counter()
        self.stats = dict(route=pca.route_, n_pca_modes=q, ms_pca=1e3 * (t1 - t0), ms_lagcov=1e3 * (t2 - t1),
                          ms_eigen=1e3 * (t3 - t2), ms_project=1e3 * (t4 - t3))
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X, normalized: bool = False):
        """pop.py:271-294: new data -> the fitted preprocessing -> PC space (X V) -> the fitted coefficient product"""
        self.compute()
        Z, fields, vs = _pcspace.project_modes(self, X, self._W)
        q = self._W.shape[0]
        Z = Z[:, :q] + 1j * Z[:, q:]
        if normalized:
            Z = Z / self.data["norms"]
        return self.preprocessor.inverse_transform_scores(Z, "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores, normalized: bool = False):
        """pop.py:296-324: Xhat = scores . components^T over the modes the scores name (no conjugation), complex:
        Re = Zr Cr^T - Zi Ci^T and Im = Zi Cr^T + Zr Ci^T, float64 products of inner length k' on the matrix cores
        (engine.pcmul over blocks of 2048 features); the real part is un-scaled with the fitted centring, the imaginary
        part without the mean (the reference's Scaler adds one real mean)"""
        self.compute()
        S, modes, vs, fields = parse_scores(scores, self.preprocessor.fields, np.complex128, scalar_mode=True)
        if normalized:
            S = S * self.data["norms"][modes - 1]
        C = self.data["components"][:, modes - 1]
        ctx = self.ctx
        Zr, Zi = engine.device_panel(ctx, S.real), engine.device_panel(ctx, S.imag)      # float64, staged once for the blocks
        rec_re = _pcspace.reconstruct(ctx, Zr, C.real) - _pcspace.reconstruct(ctx, Zi, C.imag)
        rec_im = _pcspace.reconstruct(ctx, Zi, C.real) + _pcspace.reconstruct(ctx, Zr, C.imag)
        pre = self.preprocessor
        re = pre.inverse_transform_data(rec_re, "reconstructed_data", fields, vs)
        mean, pre.mean_ = pre.mean_, None
        try:
            im = pre.inverse_transform_data(rec_im, "reconstructed_data", fields, vs)
        finally:
            pre.mean_ = mean
        return labelled.complex_join(re, im)

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the POPs: the eigenvectors of the feedback matrix in feature space"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def scores(self, normalized: bool = False):
        """the POP coefficients; `normalized`: divided by `norms`"""
        S = self.data["scores"]
        if normalized:
            S = S / self.data["norms"]
        return self.preprocessor.inverse_transform_scores(S, "scores", self.attrs)

    def eigenvalues(self):
        return self._mode_array(self.data["eigenvalues"], "eigenvalues")

    def damping_times(self):
        return self._mode_array(self.data["damping_times"], "damping_times")

    def periods(self):
        return self._mode_array(self.data["periods"], "periods")

    def components_amplitude(self):
        return ComplexEOF._map(self.components(), np.abs, "components_amplitude")

    def components_phase(self):
        return ComplexEOF._map(self.components(), np.angle, "components_phase")

    def scores_amplitude(self, normalized: bool = True):
        return ComplexEOF._map(self.scores(normalized), np.abs, "scores_amplitude")

    def scores_phase(self):
        return ComplexEOF._map(self.scores(), np.angle, "scores_phase")

    singular_values = NO_SINGULAR_VALUES
    explained_variance = explained_variance_ratio = NO_EXPLAINED_VARIANCE
