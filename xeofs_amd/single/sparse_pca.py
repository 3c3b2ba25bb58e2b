"""xeofs_amd.single.SparsePCA -- drop-in for xeofs.single.SparsePCA (xeofs/single/sparse_pca.py:15-352): sparse PCA by
variable projection [Erichson et al. 2020], minimising 1/2 |X - X B A^T|^2 + alpha |B|_1 + beta/2 |B|^2.

The randomized route compresses the preprocessed field to C = Q^T X (compute_rqb) with the engine's panel products; the
exact route decomposes X itself.  Either way the iteration runs on the device in float64 from the thin SVD of C
(spca.spca_solve, csrc/eofx_spca.hpp): for k <= 64 modes and at most 128 singular vectors each iteration is one streaming
pass over V and B plus a single-workgroup step, and the host reads a finished flag once per 16 iterations.

Deliberate deviations from the reference:
  1. the right singular vectors V of C carry the engine's deterministic sign rule (the reference keeps LAPACK's); the
     iteration is sign-equivariant, so B, A and the scores equal the reference's up to one sign per mode;
  2. when Z = X^T X B is rank-deficient (e.g. a mode whose B column is entirely zero) A's completion is deterministic
     (the first unit vectors outside the span), not LAPACK's;
  3. shapes beyond the loop kernels (k > 64 or more than 128 singular vectors, mostly the exact route) take the general
     route: the same iteration as fixed-order device products with the small polar factor on the host.
"""

from __future__ import annotations

import numpy as np

from .. import engine, labelled, spca
from .eof import EOF, NO_SINGULAR_VALUES

VALID_SOLVERS = ("auto", "full", "randomized")


class SparsePCA(EOF):
    """Drop-in for xeofs.single.SparsePCA (xeofs/single/sparse_pca.py:15-352).  components() is the sparse weight matrix
    B, data["components_normal"] the orthonormal A, scores() = X B, inverse_transform(scores) = A scores."""

    def __init__(self, n_modes: int = 2, alpha: float = 1e-3, beta: float = 1e-3, robust: bool = False,
                 regularizer: str = "l1", max_iter: int = 500, tol: float = 1e-6, oversample: int = 10,
                 n_subspace: int = 1, n_blocks: int = 1, center: bool = True, standardize: bool = False,
                 use_coslat: bool = False, sample_name: str = "sample", feature_name: str = "feature", check_nans=True,
                 compute: bool = True, random_state: int | None = None, solver: str = "auto", solver_kwargs: dict = {},
                 **kwargs):
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs, **kwargs)
        self.attrs.update({"model": "Sparse PCA"})
        self._params.update({"alpha": alpha, "beta": beta, "robust": robust, "regularizer": regularizer,
                             "max_iter": max_iter, "tol": tol, "oversample": oversample, "n_subspace": n_subspace,
                             "n_blocks": n_blocks})
        self._params["solver_kwargs"] = dict(solver_kwargs)

    # ------------------------------------------------------------------ fit
    def _check_arguments(self, X):
        prm = self._params
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        if prm["solver"] not in VALID_SOLVERS:
            raise ValueError(f"Unrecognized solver '{prm['solver']}'. Valid options are 'auto', 'full', and 'randomized'.")
        if prm["regularizer"] not in spca.SPCA_REGULARIZERS:
            raise ValueError(f'regularizer must be one of ("l1", "l0"), not {prm["regularizer"]}.')
        if prm["robust"] and prm["regularizer"] == "l0":
            raise NotImplementedError("l0 regularization is not supported for robust sparse pca")

    def _fit_now(self, X, dim, weights=None):
        self._check_arguments(X)
        return self._fit_algorithm(self._preprocess(X, dim, weights))

    def use_exact(self, n: int, p: int) -> bool:
        """sparse_pca.py:161-178: "auto" takes the exact route iff max(n, p) < 500 and n_modes > int(0.8 min(n, p))"""
        solver = self._params["solver"]
        if solver == "auto":
            return max(n, p) < 500 and self.n_modes > int(0.8 * min(n, p))
        return solver == "full"

    def _fit_algorithm(self, mat, omega=None, dec=None):
        prm = self._params
        k = int(self.n_modes)
        n, p = mat.n, mat.p
        if k > p:
            mat.free()
            raise ValueError(f"n_components must be less than the number of columns of X ({p})")
        exact = self.use_exact(n, p)
        if exact:
            Ct = spca._dev64(self.ctx, mat.download()).T.contiguous()        # X^T [p x n]
        else:
            Ct = spca.spca_compress(self.ctx, mat, k, prm["oversample"], prm["n_subspace"], prm["n_blocks"],
                                    prm["random_state"])
        m_c = Ct.shape[1]
        res = spca.spca_solve(self.ctx, Ct, k, prm["alpha"], prm["beta"], prm["regularizer"], prm["max_iter"], prm["tol"],
                              check=bool(prm["compute"]), robust=bool(prm["robust"]))
        del Ct
        ev = explained_variance(res["dtilde"], n, m_c, k, prm["oversample"], exact)
        B = res["B"].to(dtype=engine._torch().float32).cpu().numpy()
        A = res["A"].to(dtype=engine._torch().float32).cpu().numpy()
        scores = engine.project(self.ctx, mat, B)
        norms = np.linalg.norm(scores.astype(np.float64), axis=0)
        self.data = dict(input_data=mat, components=B, components_normal=A, scores=scores, norms=norms,
                         explained_variance=ev, total_variance=self.preprocessor.total_variance)
        self.stats = dict(route="exact" if exact else "randomized", solver_route=res["route"], n_iter=res["n_iter"],
                          objective=res["objective"], ms=res["ms"], rows_compressed=m_c)
        return self

    # ------------------------------------------------------------------ transform / inverse
    def inverse_transform(self, scores, normalized: bool = False):
        """sparse_pca.py:277-284: A . scores over the selected modes, then un-scaled by the Preprocessor"""
        self.compute()
        S, modes, vs, fields = self._parse_scores(scores, normalized, np.float32)
        A = np.ascontiguousarray(self.data["components_normal"][:, modes - 1])
        rec = engine.reconstruct(self.ctx, S, A)
        return self.preprocessor.inverse_transform_data(rec, "reconstructed_data", fields, vs)

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the sparse weight matrix B (not renormalised, as in the reference)"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    singular_values = NO_SINGULAR_VALUES


def explained_variance(dtilde, n: int, m_c: int, k: int, oversample: int, exact: bool) -> np.ndarray:
    """compute_spca's Dtilde / (m_c - 1), rescaled on the randomized route by (k + oversample - 1) / (n - 1)
    (_sparse_pca.py:561, 692); m_c = the rows of the decomposed matrix (n on the exact route, min(n, l) otherwise)"""
    ev = np.asarray(dtilde, dtype=np.float64) / (m_c - 1)
    if not exact:
        ev = ev * (k + oversample - 1) / (n - 1)
    return ev
