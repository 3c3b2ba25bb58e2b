"""What the real and complex cross models and their rotators share: the labelled accessors of a fitted pair of fields
(base_model_cross_set.py:465-523) and the diagnostics of Swenson (2015) in rank-one algebra (cpcca.py:330-640), written
once in the conjugate-aware form -- `conj()` and `.real` are the identity on real arrays.

A class that mixes `PairSurface` in keeps its fitted arrays in `self.data` (`components1/2`, `scores1/2`, `norm1/2`, ...)
and names its two preprocessors through `_pres()`; `ModelSurface` also reads the analysis-space singular vectors
(`_analysis_vectors`) and the two analysis sides (`_sides`): objects with `A_mul(B)`, `A_tmul(R)`, `A_sumsq()` and
`Tinv`, A the UNwhitened analysis matrix -- `cpcca._Side` (resident or host) and `HostSide` (a host matrix)."""

from __future__ import annotations

import warnings

import numpy as np

from .. import labelled


def _pair(v):
    return list(v) if isinstance(v, (list, tuple)) else [v, v]


def _wide(a):
    """float32 -> float64, complex -> complex128: the precision of the host diagnostics"""
    return np.asarray(a, dtype=np.result_type(a.dtype, np.float64))


def warn_ill_conditioned(n, m):
    if n < m:                                               # whitener.py:101-104
        warnings.warn(f"The number of samples ({n}) is smaller than the number of features ({m}), leading to "
                      "an ill-conditioned problem. This may cause unstable results. Consider using PCA to "
                      "reduce dimensionality and stabilize the problem by setting `use_pca=True`.")


class HostSide:
    """An analysis side whose unwhitened matrix A (n x m, real or complex) lies on the host."""

    def __init__(self, A, Tinv=None):
        self.A, self.Tinv = A, Tinv

    def A_mul(self, B):
        return self.A @ B

    def A_tmul(self, R):
        return self.A.conj().T @ R

    def A_sumsq(self):
        return (np.abs(self.A) ** 2).sum()


def _deflated_norms(sx, sy, R1, R2, B1, B2, M2):
    """||(A1 - r1 b1^H)^H (A2 - r2 b2^H)||_F^2 per mode without forming A1^H A2 (A_i the matrices of the sides sx, sy): with
    M = A1^H A2 the product is D = M - g1 b2^H - b1 g2^H + c b1 b2^H (g1 = A1^H r2, g2 = A2^H r1, c = r1^H r2) and ||D||^2
    expands into inner products of n-vectors A_i x (M2 = ||M||_F^2), all modes batched into panel products."""
    dot = lambda a, b: (a.conj() * b).sum(axis=0)            # column-wise <a, b>
    G1, G2 = sx.A_tmul(R2), sy.A_tmul(R1)                    # (m1 x k), (m2 x k)
    a1, a2b = sx.A_mul(B1), sy.A_mul(B2)
    a1g, a2g = sx.A_mul(G1), sy.A_mul(G2)
    c = dot(R1, R2)
    nb1, nb2, ng1, ng2 = dot(B1, B1).real, dot(B2, B2).real, dot(G1, G1).real, dot(G2, G2).real
    return (M2 + nb1 * ng2 + ng1 * nb2 + np.abs(c) ** 2 * nb1 * nb2
            - 2 * dot(a2g, a1).real - 2 * dot(a2b, a1g).real + 2 * (c * dot(a2b, a1)).real
            + 2 * (dot(B1, G1) * dot(B2, G2)).real - 2 * (c * nb1 * dot(B2, G2)).real - 2 * (c * dot(G1, B1) * nb2).real)


def covariance_fraction_CD95(self):
    """mca.py:127-189 (Cheng & Dunkerton 1995): CF_i = sigma_i / sum_j sigma_j over the retained modes, with the
    reference's warning when the estimate still moves by more than 1e-3 with the last mode."""
    s = np.asarray(self.data["singular_values"], dtype=np.float64)
    cf = s[0] / np.cumsum(s)
    if len(s) > 1 and (cf[-2] - cf[-1]) > 0.001:
        warnings.warn("The curent estimate of CF is sensitive to the number of modes retained. Please increase "
                      "`n_modes` for a better estimate.")
    return self._mode_array(s / s.sum(), "covariance_fraction")


class PairSurface:
    """components / scores of the two fields and the per-mode arrays: models and rotators alike."""

    _suffix = ("1", "2")          # of the output names: components1 / components2

    def _pres(self):
        """the two preprocessors that label the outputs"""
        raise NotImplementedError

    def _mode_array(self, values, name):
        return labelled.mode_array(values, name, self.attrs, self._pres()[0].fields[0].like)

    def _mode_matrix(self, M, name):
        return labelled.mode_matrix(M, name, self.attrs, self._pres()[0].fields[0].like)

    def _components(self, normalized):
        c = [self.data["components1"], self.data["components2"]]
        if not normalized:                                       # cpcca.py:308-316
            c = [x * self.data[f"norm{i + 1}"].astype(x.real.dtype) for i, x in enumerate(c)]
        return c

    def _scores(self, normalized):
        s = [self.data["scores1"], self.data["scores2"]]
        if normalized:                                           # cpcca.py:318-329
            s = [x / self.data[f"norm{i + 1}"].astype(x.real.dtype) for i, x in enumerate(s)]
        return s

    def _wrap(self, kind, arrays, name):
        return tuple(getattr(pre, "inverse_transform_" + kind)(a, name + sfx, self.attrs)
                     for pre, a, sfx in zip(self._pres(), arrays, self._suffix))

    def components(self, normalized: bool = True):
        return self._wrap("components", self._components(normalized), "components")

    def scores(self, normalized: bool = False):
        return self._wrap("scores", self._scores(normalized), "scores")

    def squared_covariance(self):
        return self._mode_array(self.data["squared_covariance"], "squared_covariance")


class ComplexPairSurface:
    """amplitude and phase of complex components / scores (next to `PairSurface`)"""

    def components_amplitude(self, normalized: bool = True):
        return self._wrap("components", [np.abs(c) for c in self._components(normalized)], "components_amplitude")

    def components_phase(self, normalized: bool = True):
        return self._wrap("components", [np.angle(c) for c in self._components(normalized)], "components_phase")

    def scores_amplitude(self, normalized: bool = False):
        return self._wrap("scores", [np.abs(s) for s in self._scores(normalized)], "scores_amplitude")

    def scores_phase(self, normalized: bool = False):
        return self._wrap("scores", [np.angle(s) for s in self._scores(normalized)], "scores_phase")


class ModelSurface(PairSurface):
    """the fitted models: spectrum and diagnostics, in the n x m analysis space (a PCA basis has orthonormal columns, so
    Frobenius norms of feature-space residuals equal those of their PC-space coordinates)"""

    def _sides(self):
        """the two analysis sides (see the module docstring)"""
        raise NotImplementedError

    def _analysis_vectors(self, i):
        """singular vectors of side i in the (whitened) analysis space, m x k"""
        raise NotImplementedError

    def singular_values(self):
        return self._mode_array(self.data["singular_values"], "singular_values")

    def total_squared_covariance(self):
        return self.data["total_squared_covariance"]

    def _rank_one_terms(self):
        """mode j: the whitened reconstruction r_j q_j^H un-whitened (whitener.inverse_transform_data: . @ T^-1) is
        r_j b_j^H with b_j = T^-H q_j"""
        R1, R2 = _wide(self.data["scores1"]), _wide(self.data["scores2"])      # (reading `data` runs a deferred fit)
        B = []
        for i, sd in enumerate(self._sides()):
            Q = self._analysis_vectors(i)
            B.append(Q if sd.Tinv is None else sd.Tinv.conj().T @ Q)
        return R1, R2, B[0], B[1]

    def squared_covariance_fraction(self):
        """cpcca.py:418-512: SCF_i = 1 - ||d_X,i^H d_Y,i||_F^2 / ||X^H Y||_F^2 with d the residual of the un-whitened data
        after its reconstruction by mode i (clipped at 0) -- for every alpha; with alpha = 1 it equals sigma_i^2 / TSC.
        Neither X^H Y nor any per-mode reconstruction of the fields is formed (`_deflated_norms`)."""
        R1, R2, B1, B2 = self._rank_one_terms()
        sx, sy = self._sides()
        M2 = self.data["total_squared_covariance"] * (R1.shape[0] - 1) ** 2
        scf = 1 - _deflated_norms(sx, sy, R1, R2, B1, B2, M2) / M2
        return self._mode_array(np.where(scf < 0, 0, scf), "squared_covariance_fraction")

    def _fve_self(self, i):
        """cpcca.py:514-639: 1 - ||A - r b^H||_F^2 / ||A||_F^2 per mode"""
        terms = self._rank_one_terms()
        sd, R, B = self._sides()[i], terms[i], terms[2 + i]
        tot = sd.A_sumsq()
        res = tot - 2 * (sd.A_mul(B).conj() * R).sum(axis=0).real + (np.abs(R) ** 2).sum(0) * (np.abs(B) ** 2).sum(0)
        return 1 - res / tot

    def fraction_variance_X_explained_by_X(self):
        return self._mode_array(self._fve_self(0), "fraction_variance_X_explained_by_X")

    def fraction_variance_Y_explained_by_Y(self):
        return self._mode_array(self._fve_self(1), "fraction_variance_Y_explained_by_Y")

    @staticmethod
    def _corr(A, B):
        """cpcca.py:910-1022 method='correlation': columns divided by numpy's (real, population) std, then A^H B / (n - 1)"""
        A, B = _wide(A), _wide(B)
        return (A / A.std(axis=0)).conj().T @ (B / B.std(axis=0)) / (A.shape[0] - 1)

    def cross_correlation_coefficients(self):
        return self._mode_array(np.diag(self._corr(self.data["scores1"], self.data["scores2"])),
                                "cross_correlation_coefficients")

    def correlation_coefficients_X(self):
        return self._mode_matrix(self._corr(self.data["scores1"], self.data["scores1"]), "correlation_coefficients_X")

    def correlation_coefficients_Y(self):
        return self._mode_matrix(self._corr(self.data["scores2"], self.data["scores2"]), "correlation_coefficients_Y")
