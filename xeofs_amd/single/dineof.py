"""xeofs_amd.single.DINEOF -- EOF analysis and gap filling of a field with isolated missing values (Beckers & Rixen 2003,
Alvera-Azcarate et al. 2005).  The reference has no such model: its Sanitizer, like `EOF` here, refuses such a field.

DINEOF is an EM iteration around the truncated SVD: fit rank k, write the rank-k reconstruction into the gaps, repeat until
the filled values stand still; the number of modes is the one that reconstructs a set of withheld valid entries best.  The
SVD is `engine.fit` on the device-resident field, in place and warm-started; the fill is `engine.lrfill`
(csrc/eofx_lrfill.hpp), which writes the masked entries only and returns the change norm.

The sketch of every decomposition has ONE width, n_modes + n_oversamples (at most the smaller side of the field): a stage
with k < n_modes modes oversamples by the difference.  A field whose smaller side is within that width is decomposed
exactly (the engine replaces a full-width sketch by the identity).  The first decomposition draws a Gaussian sketch and
runs scikit-learn's "auto" count of power iterations; every later one starts from the previous small-side factor, padded
with fresh Gaussian columns, and runs `solver_kwargs["n_iter_warm"]` (default 2) power iterations: between two EM steps
only the gaps move, by less and less, so the previous subspace is a start the iteration count of a cold start would be
wasted on.  Two is a choice, not a measured optimum; tests/test_gpu_dineof.py holds the resulting cross-validation error
against an exact-SVD restatement.  The LAST decomposition, whose factors the accessors return, is a cold one again: the
sketch, oversampling and iteration count of `EOF(n_modes=k*, random_state=..., solver_kwargs=...)` on the filled field, so
that on a gap-free field the two models agree mode by mode, noise-bulk modes included.
"""

from __future__ import annotations

import warnings

import numpy as np

from .. import engine
from ..preprocessing import GapPreprocessor
from .eof import EOF

MAX_SKETCH = 256      # EOFX_MAX_SKETCH (include/eofx.h)


# ---------------------------------------------------------------------------- host logic (tests/test_dineof_host.py)
def cv_count(n_valid: int, cv_fraction: float, cv_min: int) -> int:
    """the number of cross-validation points: max(cv_min, round(cv_fraction * #valid))"""
    return max(int(cv_min), int(round(cv_fraction * n_valid)))


def cv_candidates(total: int, m: int, random_state=None) -> np.ndarray:
    """2 m flat indices (int64) into a field of `total` entries, drawn without replacement"""
    rng = np.random.default_rng(random_state)
    return rng.choice(int(total), size=min(2 * int(m), int(total)), replace=False).astype(np.int64)


def cv_keep(candidates, is_gap, m: int) -> np.ndarray:
    """the first m candidates that are no gap, in drawing order"""
    return np.asarray(candidates, dtype=np.int64)[~np.asarray(is_gap, dtype=bool)][: int(m)]


def group_bits(flat_index, p: int, ldw: int):
    """Flat indices i p + j of a field with p columns -> (words, masks): the unique flat word indices i ldw + (j >> 5)
    (int64, ascending) of a gap mask with `ldw` words per row, and per word the OR of the bits j & 31 (int32, bit 31 being
    the sign) -- what one gather / scatter with unique indices updates."""
    idx = np.asarray(flat_index, dtype=np.int64)
    i, j = idx // p, idx % p
    word = i * int(ldw) + (j >> 5)
    bit = np.left_shift(np.uint32(1), (j & 31).astype(np.uint32))
    order = np.argsort(word, kind="stable")
    word, bit = word[order], bit[order]
    if word.size == 0:
        return word, bit.view(np.int32)
    first = np.flatnonzero(np.concatenate([[True], word[1:] != word[:-1]]))
    return word[first], np.bitwise_or.reduceat(bit, first).view(np.int32)


def converged(sum_d2: float, count: int, tol: float, rms: float) -> bool:
    """the stopping rule of the EM iteration: sqrt(sum (new - old)^2 / count) <= tol rms (nothing to fill: converged)"""
    return count == 0 or float(np.sqrt(sum_d2 / count)) <= tol * rms


def stop_raising(cv_error) -> bool:
    """whether the last mode count made the cross-validation error worse"""
    return len(cv_error) >= 2 and cv_error[-1] > cv_error[-2]


def optimal_modes(cv_error) -> int:
    """k* = the (first) mode count of the smallest cross-validation error; the counts run from 1"""
    return int(np.argmin(np.asarray(cv_error, dtype=np.float64))) + 1


class DINEOF(EOF):
    """EOF analysis of a field with isolated NaNs, and the field with its gaps filled (`filled()`).

    `fit(X, dim, weights=None)`: features and samples that are entirely NaN are dropped as everywhere else; every other
    NaN is a gap.  `cv_fraction` of the valid entries (at least `cv_min`) are withheld to choose the number of modes --
    m points from 2 m candidates, so a field with more gaps than valid entries yields fewer than m (about 0.6 m at a gap
    fraction of 0.7), with a warning; `data["cv_index"]` holds those in use --
    k* <= n_modes (`n_modes_optimal`, `cv_error()`); an EM iteration stops when the RMS change of the filled values is
    below `tol` times the RMS of the valid ones, or after `max_iter` steps.  The `EOF` accessors then give the k* modes of
    the filled field; `transform` of new data raises on isolated NaNs as `EOF` does."""

    def __init__(self, n_modes: int = 10, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 cv_fraction: float = 0.01, cv_min: int = 30, tol: float = 1e-3, max_iter: int = 50,
                 random_state: int | None = None, sample_name: str = "sample", feature_name: str = "feature",
                 solver_kwargs: dict = {}):
        if not isinstance(n_modes, (int, np.integer)) or isinstance(n_modes, bool) or not 1 <= n_modes <= engine.LRFILL_KMAX:
            raise ValueError(f"n_modes must be an integer in [1, {engine.LRFILL_KMAX}], got {n_modes!r}")
        if not 0.0 < float(cv_fraction) < 1.0:
            raise ValueError(f"cv_fraction must lie in (0, 1), got {cv_fraction!r}")
        if not isinstance(cv_min, (int, np.integer)) or cv_min < 1:
            raise ValueError(f"cv_min must be a positive integer, got {cv_min!r}")
        if not float(tol) > 0.0:
            raise ValueError(f"tol must be positive, got {tol!r}")
        if not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
            raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
        n_over = int(dict(solver_kwargs).get("n_oversamples", 10))
        if n_over < 0 or int(n_modes) + n_over > MAX_SKETCH:
            raise ValueError(f"n_modes + n_oversamples must be at most {MAX_SKETCH}, got {int(n_modes) + n_over}")
        kw = {k: v for k, v in dict(solver_kwargs).items() if k != "n_iter_warm"}
        super().__init__(n_modes=int(n_modes), center=center, standardize=standardize, use_coslat=use_coslat,
                         sample_name=sample_name, feature_name=feature_name, random_state=random_state, solver="randomized",
                         solver_kwargs=kw)
        self._solver_kwargs = dict(solver_kwargs)
        self._width = int(n_modes) + n_over
        self._params.update(cv_fraction=float(cv_fraction), cv_min=int(cv_min), tol=float(tol), max_iter=int(max_iter))
        for k in ("check_nans", "compute", "solver"):
            self._params.pop(k)
        self.attrs = {k: v for k, v in self.attrs.items() if k not in ("check_nans", "compute", "solver")}
        self.attrs.update(model="DINEOF", cv_fraction=float(cv_fraction), cv_min=int(cv_min), tol=float(tol),
                          max_iter=int(max_iter))
        self.preprocessor = GapPreprocessor(center, standardize, use_coslat)
        self.n_modes_optimal = None

    # ------------------------------------------------------------------ the decomposition and one EM stage
    def _svd(self, F, k, final=False):
        """rank-k SVD of the device field F -> (U [n x k], s [k] host, V [p x k]), device tensors; the resident matrix of the
        call aliases F and is freed before anything writes F.  final: -> (the matrix, U, s, V) with host factors instead."""
        n, p = F.shape
        small = min(n, p)
        L = min(self._width, small)
        kw = self._solver_kwargs
        if L == small:                       # the engine takes the identity: exact, nothing to start from
            omega, n_iter = np.eye(small, L, dtype=np.float32), kw.get("n_iter", "auto")
        elif self._warm is None:
            omega, n_iter = engine.sketch_matrix(small, L, self._rs), kw.get("n_iter", "auto")
        else:
            fresh = self._rs.normal(size=(small, L - self._warm.shape[1])).astype(np.float32)
            omega, n_iter = np.ascontiguousarray(np.concatenate([self._warm, fresh], axis=1)), kw.get("n_iter_warm", 2)
        n_over, rs = L - k, None
        if final and L < small:
            # the last decomposition is the one `EOF(n_modes=k*, random_state=..., solver_kwargs=...)` makes of the filled
            # field: its sketch, its oversampling, its iteration count -- a mode inside the noise bulk is not converged by
            # either count, and only the same recipe gives the same vector (0.9989 against EOF's with the warm start)
            omega, n_iter = None, kw.get("n_iter", "auto")
            n_over, rs = self._width - int(self.n_modes), self._params["random_state"]
        # (check_nans stays on: it is the engine's ordinary statistics pass, and F holds no NaN for it to find)
        mat, _, U, s, V = engine.fit(self.ctx, F, k, center=False, standardize=False, feature_weights=None, check_nans=True,
                                     n_oversamples=n_over, n_iter=n_iter, random_state=rs, omega=omega, want_stats=False,
                                     device_out=not final)
        if final:
            return mat, U, s, V
        mat.free()
        # The engine takes its start matrix from the host, so the small-side factor (min(n, p) x k floats: 2 MB at
        # 10000 x 50) crosses PCIe twice per EM step, and the download waits for the decomposition -- which the stopping
        # rule, read on the host after every fill, does anyway.
        self._warm = (U if n < p else V).cpu().numpy()
        return U, s, V

    def _stage(self, F, bits, k, rms):
        """EM at k modes until the stopping rule or max_iter -> (iterations, sum new^2 of the last fill)"""
        import torch

        prm = self._params
        new2 = 0.0
        for it in range(1, prm["max_iter"] + 1):
            U, s, V = self._svd(F, k)
            A = U * torch.as_tensor(s, device=U.device)
            count, d2, new2 = engine.lrfill(self.ctx, F, bits, A, V)
            if converged(d2, count, prm["tol"], rms):
                break
        return it, new2

    # ------------------------------------------------------------------ fit
    def fit(self, X, dim, weights=None):
        return self._fit_now(X, dim, weights)

    def _fit_now(self, X, dim, weights=None):
        import torch

        ctx = self._bind_context()
        pre, prm = self.preprocessor, self._params
        F, bits, gaps = pre.fit_transform(X, dim, weights)
        self.sample_dims = pre.sample_dims
        n, p = F.shape
        K = int(self.n_modes)
        if K > min(n, p):
            raise ValueError(f"n_modes must be less than or equal to the rank of the dataset (rank = {min(n, p)}).")
        if n < 2:
            raise ValueError("DINEOF needs at least two valid samples")
        self._rs = np.random.RandomState(prm["random_state"])
        self._warm = None
        flatF, flatB = F.view(-1), bits.view(-1)
        # cross-validation points: withheld valid entries
        n_valid = n * p - gaps
        m = cv_count(n_valid, prm["cv_fraction"], prm["cv_min"])
        cand = cv_candidates(n * p, m, prm["random_state"])
        cw = torch.as_tensor((cand // p) * bits.shape[1] + ((cand % p) >> 5), device=F.device)
        is_gap = (flatB[cw].cpu().numpy().view(np.uint32) >> (cand % p & 31).astype(np.uint32)) & 1
        cv_index = cv_keep(cand, is_gap, m)
        if cv_index.size == 0 or cv_index.size >= n_valid:
            raise ValueError(f"no cross-validation points can be withheld from {n_valid} valid entries and {gaps} gaps")
        if cv_index.size < m:                            # more than half of the candidates were gaps
            warnings.warn(f"DINEOF: {cv_index.size} cross-validation points instead of {m}: of the {cand.size} candidates drawn, "
                          f"{cand.size - cv_index.size} are gaps (gap fraction {gaps / (n * p):.2f})", stacklevel=3)
        cv_dev = torch.as_tensor(cv_index, device=F.device)
        cv_truth = flatF[cv_dev].clone()
        words, masks = (torch.as_tensor(a, device=F.device) for a in group_bits(cv_index, p, bits.shape[1]))
        flatF[cv_dev] = 0.0
        flatB[words] = flatB[words] | masks
        truth64 = cv_truth.to(torch.float64)
        rest = n_valid - cv_index.size                   # entries that are neither gap nor withheld
        rms = float(np.sqrt(max(pre.sumsq_valid - float((truth64 ** 2).sum()), 0.0) / rest))
        # the number of modes
        cv_error, n_iterations = [], []
        for k in range(1, K + 1):
            it, _ = self._stage(F, bits, k, rms)
            n_iterations.append(it)
            cv_error.append(float(torch.sqrt(((flatF[cv_dev].to(torch.float64) - truth64) ** 2).mean())))
            if stop_raising(cv_error):
                break
        kopt = optimal_modes(cv_error)
        # the final stage: the withheld entries are data again
        flatB[words] = flatB[words] & ~masks
        flatF[cv_dev] = cv_truth
        rms = float(np.sqrt(pre.sumsq_valid / n_valid))
        it, new2 = self._stage(F, bits, kopt, rms)
        n_iterations.append(it)
        # one more decomposition, of the field as it now stands; its in-place matrix stays (and keeps F alive)
        mat, U, s, V = self._svd(F, kopt, final=True)
        s64 = s.astype(np.float64)
        total_variance = (pre.sumsq_valid + new2) / (n - 1)
        pre.total_variance = total_variance
        self.n_modes_optimal = kopt
        self.data = dict(input_data=mat, components=V, scores=U * s, norms=s64, explained_variance=s64 ** 2 / (n - 1),
                         total_variance=total_variance, cv_index=cv_index, cv_truth=cv_truth.cpu().numpy(),
                         cv_error=np.asarray(cv_error), n_iterations=np.asarray(n_iterations), n_gaps=int(gaps),
                         filled_anomalies=F, gap_bits=bits)
        del self._warm, self._rs
        return self

    # ------------------------------------------------------------------ accessors
    def cv_error(self):
        """the RMSE at the withheld entries after the stage of 1 .. K_tried modes, in preprocessed units"""
        return self._mode_array(self.data["cv_error"], "cv_error")

    def filled(self):
        """the field in the caller's units and labels: every valid entry as it came, the gaps reconstructed from the
        n_modes_optimal modes; features and samples that were entirely NaN stay NaN"""
        self.compute()
        return self.preprocessor.filled_data(self.data["filled_anomalies"].cpu().numpy(), "filled")
