"""The complex and Hilbert cross models: ComplexCPCCA / HilbertCPCCA (xeofs/cross/cpcca.py:1023-1500) and their fixed-alpha
children ComplexMCA / HilbertMCA (cross/mca.py:224-489, alpha = 1), ComplexCCA / HilbertCCA (cross/cca.py:123-355,
alpha = 0), ComplexRDA / HilbertRDA (cross/rda.py:123-355, alpha = [0, 1]), plus their rotators.

The `Complex*` classes take complex fields Z_x = U_x + i V_x, Z_y = U_y + i V_y; the `Hilbert*` classes take real fields and
augment them with their Hilbert transform.  Order of the stages as in base_model_cross_set.py:300-315:

    preprocess -> PCA pre-reduction (default) -> [Hilbert transform of the PC scores: `_augment_data`] -> fractional
    whitening T = (S^H S / n)^((alpha - 1) / 2) (identity for alpha = 1) -> cross-covariance C = S_x^H S_y / (n - 1) ->
    SVD of C -> scores, norms, total squared covariance of the UNwhitened matrices.

What runs on the GPU: the preprocessor, the PCA pre-reductions -- `ResidentPCA` on the real fields of the Hilbert model
(its analytic signal is taken of the n x m PC scores, through the same `eofx_hilbert_f32`), `ComplexResidentPCA`
(Hermitian Gram route) on complex fields -- and every product with a resident field (back-projection of the singular
vectors, projection of new data).  After the pre-reduction the analysis matrices are n x m with m of the order of tens to
hundreds, and the m_x x m_y complex cross-covariance matrix is decomposed exactly on the host (the reference hands it to
scipy's svds(lobpcg): same singular values / subspaces to its tolerance, vectors up to a unit phase per mode).
Without PCA (`use_pca=False`) the fields themselves are the analysis matrices: supported while they are small enough to
decompose densely (n * p <= MAX_DENSE); beyond that use the default PCA route.
Accessors and diagnostics are those of `cross/_surface.py` on the host analysis matrices (`HostSide`); the rotator shares
`cpcca_rotator.CrossRotator` with the real one.
"""

from __future__ import annotations

import datetime
import os
import warnings

import numpy as np

from .. import __version__, cpanel, engine, labelled, rotation
from .._deferred import Deferred
from ..cpca import ComplexResidentPCA
from ..linalg.decomposer import sanity_check_n_modes
from ..pca import ResidentPCA
from ..preprocessing import Preprocessor, parse_scores
from ._surface import ComplexPairSurface, HostSide, ModelSurface, _pair, covariance_fraction_CD95, warn_ill_conditioned
from .cpcca_rotator import CrossRotator

MAX_DENSE = 50_000_000      # elements of a field decomposed without PCA pre-reduction


def _hermitian_power(C, power):
    """linalg/_numpy/_utils.py:6-33 for a Hermitian PSD matrix: V s^power V^H, s <= eps dropped"""
    w, V = np.linalg.eigh(0.5 * (C + C.conj().T))
    keep = w > np.finfo(w.dtype).eps
    return (V[:, keep] * w[keep] ** power) @ V[:, keep].conj().T


def _part32(vals, imag):
    """real / imaginary part of the input as a contiguous float32 array in ONE pass over it (the engine's working
    precision; a float64 copy of a 10 GB complex128 field first would double the host time of a fit), row blocks on a
    few threads (numpy's casting copy releases the GIL; one thread moves about 8 GB/s of a strided complex source)"""
    if not np.iscomplexobj(vals):
        return np.zeros(vals.shape, np.float32) if imag else np.ascontiguousarray(vals, dtype=np.float32)
    src = vals.imag if imag else vals.real
    if vals.ndim == 0 or vals.size < (1 << 24) or vals.shape[0] < 16:
        return np.ascontiguousarray(src, dtype=np.float32)
    from concurrent.futures import ThreadPoolExecutor
    out = np.empty(vals.shape, np.float32)
    nt = min(16, os.cpu_count() or 1, vals.shape[0])
    edges = np.linspace(0, vals.shape[0], nt + 1).astype(int)

    def block(j):
        out[edges[j]:edges[j + 1]] = src[edges[j]:edges[j + 1]]

    with ThreadPoolExecutor(nt) as ex:
        list(ex.map(block, range(nt)))
    return out


def _re_im(Z):
    """Re and Im of a labelled (complex) array as two labelled float32 arrays"""
    vals, dims, coords, name, attrs = labelled.unpack(Z)
    vals = np.asarray(vals)
    return [labelled.pack(_part32(vals, imag), dims, coords, name, attrs, Z) for imag in (False, True)]


def _leading_svd_device(C, k, device, block=24, max_iter=80, tol=1e-10):
    """k leading singular triplets of a dense complex matrix (hundreds x hundreds, float64) by block power iteration on
    the device: each step is two complex GEMMs and a QR of a (k + block)-column panel, iterated until the residuals
    ||C v - s u|| of the k wanted triplets are below tol * s_1 -- to the accuracy of the dense SVD it replaces
    (0.6 s through rocSOLVER at 1500 x 1500), which remains the fallback if the iteration has not converged.
    (The OTHER residual, ||C^H u - s v||, vanishes by construction -- V and s come from the factorisation of C^H Y
    itself -- and says nothing about convergence: ADVICE r02.)"""
    torch = engine._torch()
    dev = f"cuda:{device}"
    Cd = torch.as_tensor(C, device=dev)
    m1, m2 = Cd.shape
    l = min(k + block, m1, m2)
    g = torch.Generator().manual_seed(12345)
    Q = torch.randn((m2, l, 2), generator=g, dtype=torch.float64)
    Q = torch.view_as_complex(Q).to(dev)
    Q, _ = torch.linalg.qr(Q)
    CH = Cd.conj().T.contiguous()
    for it in range(max_iter):
        Y, _ = torch.linalg.qr(Cd @ Q)                 # m1 x l
        B = CH @ Y                                     # m2 x l   (= C^H Y)
        Q, R = torch.linalg.qr(B)
        if it >= 2 and it % 2 == 0:
            Ub, sb, Vbh = torch.linalg.svd(R.conj().T, full_matrices=False)    # Y^H C = R^H Q^H
            U = Y @ Ub[:, :k]
            V = Q @ Vbh.conj().T[:, :k]
            res = torch.linalg.norm(Cd @ V - U * sb[:k], dim=0).max()
            if float(res) <= tol * float(sb[0]):
                return U.cpu().numpy(), sb[:k].cpu().numpy(), V.conj().T.cpu().numpy()
    out = torch.linalg.svd(Cd, full_matrices=False)
    return tuple(a.cpu().numpy() for a in out)


def _sign_rule(VT):
    """utils/xarray_utils.py:273-301: +1 where |max| >= |min| per mode, numpy's lexicographic complex max / min"""
    mx, mn = VT.max(axis=1), VT.min(axis=1)
    return np.where(np.abs(mx) >= np.abs(mn), 1.0, -1.0)


class _Field:
    """one side after preprocessing and pre-reduction: analysis matrix S (n x m complex, host), maps back to features"""

    def __init__(self, S, back, project, parts, pca):
        self.S, self.back, self.project, self.parts, self.pca = S, back, project, parts, pca

    def free(self):
        for m in self.parts:
            if m is not None:
                m.free()
        self.parts = ()


class ComplexCPCCA(ComplexPairSurface, ModelSurface, Deferred):
    """Drop-in for xeofs.cross.ComplexCPCCA (cross/cpcca.py:1023-1326)."""

    _model_name = "Complex CPCCA"
    _hilbert = False
    _suffix = ("_X", "_Y")
    covariance_fraction_CD95 = covariance_fraction_CD95

    def __init__(self, n_modes: int = 2, alpha=0.2, standardize=False, use_coslat=False, check_nans=True, use_pca=True,
                 n_pca_modes=0.999, pca_init_rank_reduction=0.3, compute: bool = True, sample_name: str = "sample",
                 feature_name="feature", solver: str = "auto", random_state=None, solver_kwargs: dict = {}, **kwargs):
        sanity_check_n_modes(n_modes)
        self.alpha = [float(a) for a in _pair(alpha)]
        if any(a < 0 for a in self.alpha):       # preprocessing/whitener.py:63-66
            raise ValueError("`alpha` must be greater than or equal to 0")
        if solver not in ("auto", "full", "randomized"):
            raise ValueError(f"Unrecognized solver '{solver}'. Valid options are 'auto', 'full', and 'randomized'.")
        self.n_modes = n_modes
        std, cos, chk = _pair(standardize), _pair(use_coslat), _pair(check_nans)
        self._params = dict(n_modes=n_modes, standardize=std, use_coslat=cos, check_nans=chk, use_pca=_pair(use_pca),
                            n_pca_modes=_pair(n_pca_modes), pca_init_rank_reduction=_pair(pca_init_rank_reduction),
                            sample_name=sample_name, feature_name=_pair(feature_name), random_state=random_state,
                            compute=compute, solver=solver, alpha=list(self.alpha))
        self.sample_name = sample_name
        self.solver_kwargs = dict(solver_kwargs)
        # CPCCA always centres (cpcca.py:145); real and imaginary parts share centring, scaling and weights
        self.pre_re = [Preprocessor(True, std[i], cos[i], chk[i]) for i in range(2)]
        self.pre_im = [Preprocessor(True, False, cos[i], chk[i]) for i in range(2)]
        self.attrs = {"model": self._model_name, "software": "xeofs_amd", "version": __version__,
                      "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")}
        self.ctx = None
        self.data = {}
        self.field = [None, None]

    def get_params(self):
        return dict(self._params)

    # ------------------------------------------------------------------ fit
    def fit(self, X, Y, dim, weights_X=None, weights_Y=None):
        if labelled.is_lazy(X) or labelled.is_lazy(Y):      # linalg/decomposer.py:172-177
            raise NotImplementedError("Complex data together with dask is currently not implemented. See dask issue 7639 "
                                      "https://github.com/dask/dask/issues/7639")
        return self._fit_now(X, Y, dim, weights_X, weights_Y)

    def _complex_parts(self, i, Z, dim, weights):
        """preprocess Re and Im of a complex input with the same centring / weights (as `ComplexEOF`)"""
        if not np.iscomplexobj(labelled.unpack(Z)[0]):
            warnings.warn("Expected complex-valued data but found real-valued data. For Hilbert model, use corresponding "
                          "`Hilbert` class.")
        re, im = _re_im(Z)
        pr, pi = self.pre_re[i], self.pre_im[i]
        std_c = None
        if self._params["standardize"][i]:
            # scaler.py:105-108 on complex data: numpy's std of a complex array is the real sqrt(var Re + var Im)
            pr.standardize = False
            eps = np.finfo(np.float32).eps       # peek_std clips each part at eps: undo that, combine, clip ONCE
            s_re, s_im = (np.where(v <= eps, 0.0, v) for v in (pr.peek_std(re, dim), pi.peek_std(im, dim)))
            std_c = np.maximum(np.sqrt(s_re ** 2 + s_im ** 2), eps)
        A = pr.fit_transform(re, dim, weights, std_override=std_c)
        B = pi.fit_transform(im, dim, weights, std_override=std_c)
        return A, B, pr.total_variance + pi.total_variance

    def _dense(self, A, B):
        if A.n * A.p > MAX_DENSE:
            raise NotImplementedError(f"use_pca=False on a {A.n} x {A.p} field: the complex cross models decompose without "
                                      "PCA pre-reduction only up to n * p = %d elements; use use_pca=True" % MAX_DENSE)
        S = A.download().astype(np.float64) + 1j * B.download().astype(np.float64)

        def back(Q):
            return np.asarray(Q, dtype=np.complex64)

        def project(An, Bn):
            return An.download().astype(np.float64) + 1j * Bn.download().astype(np.float64)

        return _Field(S, back, project, (A, B), None)

    def _make_field(self, i, Z, dim, weights):
        ctx = self.ctx
        A, B, tv = self._complex_parts(i, Z, dim, weights)
        if not self._params["use_pca"][i]:
            return self._dense(A, B)
        pca = ComplexResidentPCA(ctx, self._params["n_pca_modes"][i], self._params["pca_init_rank_reduction"][i])
        pca.fit(A, B, tv)
        return _Field(pca.scores(), pca.back_project, pca.transform, (A, B), pca)

    def _fit_now(self, X, Y, dim, weights_X=None, weights_Y=None):
        self.ctx = self.ctx or engine.default_context()
        for p in self.pre_re + self.pre_im:
            p.ctx = self.ctx
        fx = self._make_field(0, X, dim, weights_X)
        fy = self._make_field(1, Y, dim, weights_Y)
        self.field = [fx, fy]
        self.sample_dims = self.pre_re[0].sample_dims
        if fx.S.shape[0] != fy.S.shape[0]:
            raise ValueError("Both data matrices must have the same number of samples but found "
                             f"{fx.S.shape[0]} in the first and {fy.S.shape[0]} in the second.")
        # fractional whitening in the analysis space (preprocessing/whitener.py:86-141; identity when alpha == 1, :46-60)
        self.T, self.Tinv, Sw = [None, None], [None, None], []
        for i, fld in enumerate((fx, fy)):
            S = fld.S
            if not (1.0 - self.alpha[i]) < np.finfo(np.float64).eps:     # whitener.py:46-60: alpha >= 1 is the identity
                n_, m_ = S.shape
                warn_ill_conditioned(n_, m_)
                T = _hermitian_power(np.ascontiguousarray(S.conj().T) @ S / n_, (self.alpha[i] - 1) / 2)
                try:
                    Tinv = np.linalg.inv(T)
                except np.linalg.LinAlgError:
                    Tinv = np.linalg.pinv(T)
                self.T[i], self.Tinv[i] = T, Tinv
                S = S @ T
            Sw.append(S)
        Sx, Sy = Sw
        n = Sx.shape[0]
        k = int(self.n_modes)
        C = np.ascontiguousarray(Sx.conj().T) @ Sy / (n - 1)     # cpcca.py:1008-1016
        rank = min(C.shape)
        if k > rank:
            raise ValueError(f"n_modes must be less than or equal to the rank of the dataset (rank = {rank}).")
        if rank >= 512:      # PC-space matrices of hundreds of modes: the leading triplets on the device
            U, s, VT = _leading_svd_device(C, k, self.ctx.device)
        else:
            U, s, VT = np.linalg.svd(C, full_matrices=False)
        U, s, VT = np.ascontiguousarray(U[:, :k]), s[:k], np.ascontiguousarray(VT[:k])
        sgn = _sign_rule(VT)
        Q1, Q2 = U * sgn[None, :], (VT * sgn[:, None]).conj().T   # decomposer.py:226: V = conj(VT).T
        scores1, scores2 = Sx @ Q1, Sy @ Q2
        norm1 = np.sqrt((scores1.conj() * scores1).sum(axis=0).real)
        norm2 = np.sqrt((scores2.conj() * scores2).sum(axis=0).real)
        Cu = C if self.Tinv[1] is None else C @ self.Tinv[1]        # cpcca.py:991-1000: of the unwhitened matrices
        Cu = Cu.conj().T if self.Tinv[0] is None else Cu.conj().T @ self.Tinv[0]

        def back(fld, Q, i):      # whitener.inverse_transform_components, then pca.inverse_transform_components
            return fld.back(Q if self.Tinv[i] is None else self.Tinv[i].conj().T @ Q)

        for fld in (fx, fy):             # the resident parts are not read again (transform preprocesses new data and
            fld.free()                   # projects through the PCA's own panel): give their HBM back
        self._Su = (fx.S, fy.S)          # unwhitened analysis matrices (host): the diagnostics below work on them
        self._back = lambda i, Q: back(self.field[i], Q, i)
        self.data = dict(Q1=Q1, Q2=Q2, components1=back(fx, Q1, 0), components2=back(fy, Q2, 1), scores1=scores1,
                         scores2=scores2, singular_values=s, squared_covariance=s ** 2,
                         total_squared_covariance=float((np.abs(Cu) ** 2).sum()), norm1=norm1, norm2=norm2)
        return self

    # ------------------------------------------------------------------ the shared surface (cross/_surface.py) reads these
    def _pres(self):
        return self.pre_re

    def _sides(self):
        return [HostSide(self._Su[i], self.Tinv[i]) for i in (0, 1)]

    def _analysis_vectors(self, i):
        return self.data[f"Q{i + 1}"]

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X=None, Y=None, normalized: bool = False):
        """base_model_cross_set.py:323-374 + cpcca.py:227-252"""
        if X is None and Y is None:
            raise ValueError("Either X or Y must be given.")
        out = []
        for i, Z in enumerate((X, Y)):
            if Z is None:
                continue
            re, im = _re_im(Z)
            An, fields, vs = self.pre_re[i].transform(re)
            Bn, _, _ = self.pre_im[i].transform(im)
            S = self.field[i].project(An, Bn)
            if self.T[i] is not None:
                S = S @ self.T[i]
            S = S @ self.data[f"Q{i + 1}"]
            An.free()
            Bn.free()
            if normalized:
                S = S / self.data[f"norm{i + 1}"]
            out.append(self.pre_re[i].inverse_transform_scores(S, "scores_" + "XY"[i], self.attrs, fields, vs))
        return out[0] if len(out) == 1 else out

    def inverse_transform(self, X=None, Y=None):
        """base_model_cross_set.py:376-425 + cpcca.py:254-271: scores (with a 'mode' dimension) back to the fields --
        S conj(Q)^T in the analysis space, un-whitened, out of the PCA basis, then every part un-scaled by its own
        Scaler (the imaginary part of a Hilbert model carries no mean)."""
        if X is None and Y is None:
            raise ValueError("Either X or Y must be provided.")
        outs = []
        for i, S in enumerate((X, Y)):
            if S is None:
                continue
            pre = self.pre_re[i]
            Sm, modes, vs, fields = parse_scores(S, pre.fields, np.complex128)                   # (n', k')
            Za = Sm @ self.data[f"Q{i + 1}"][:, modes - 1].conj().T                              # analysis space (n' x m)
            rec = np.asarray(self._back(i, np.ascontiguousarray(Za.conj().T))).conj().T         # (V T^-H Za^H)^H = Za T^-1 V^H
            re = pre.inverse_transform_data(rec.real, "reconstructed_data", fields, vs)
            if self._hilbert:      # un-scale only: inverse(Im) - inverse(0)
                im = pre.inverse_transform_data(rec.imag, "reconstructed_data", fields, vs)
                zero = pre.inverse_transform_data(np.zeros_like(rec.imag), "reconstructed_data", fields, vs)
            else:
                im = self.pre_im[i].inverse_transform_data(rec.imag, "reconstructed_data", fields, vs)
                zero = None
            outs.append(labelled.complex_join(re, im, zero))
        return outs[0] if len(outs) == 1 else outs


class HilbertCPCCA(ComplexCPCCA):
    """Drop-in for xeofs.cross.HilbertCPCCA (cpcca.py:1328-1500): real fields, analytic signal of the (PCA-reduced) data
    along the sample axis, optional exponential padding against spectral leakage."""

    _model_name = "Hilbert CPCCA"
    _hilbert = True

    def __init__(self, n_modes: int = 2, alpha=0.2, padding="exp", decay_factor=0.2, **kwargs):
        super().__init__(n_modes=n_modes, alpha=alpha, **kwargs)
        self._params["padding"] = _pair(padding)
        self._params["decay_factor"] = _pair(decay_factor)

    def _analytic(self, S, i):
        """utils/hilbert_transform.py:40-72 of an n x m real matrix along the samples, through the engine"""
        mat = engine.from_dense(self.ctx, np.ascontiguousarray(S, dtype=np.float32))
        im, _ = engine.hilbert(self.ctx, mat, self._params["padding"][i], float(self._params["decay_factor"][i]))
        out = S.astype(np.float64) + 1j * im.download().astype(np.float64)
        im.free()
        mat.free()
        return out

    def _make_field(self, i, Z, dim, weights):
        ctx = self.ctx
        pre = self.pre_re[i]
        pre.standardize = self._params["standardize"][i]
        mat = pre.fit_transform(Z, dim, weights)
        if not self._params["use_pca"][i]:
            im, _ = engine.hilbert(ctx, mat, self._params["padding"][i], float(self._params["decay_factor"][i]))
            return self._dense(mat, im)
        pca = ResidentPCA(ctx, self._params["n_pca_modes"][i], self._params["pca_init_rank_reduction"][i])
        pca.fit(mat, pre.total_variance)

        def back(Q):          # V Q with a real V: the two parts separately
            Q = np.asarray(Q)
            return pca.back_project(Q.real).astype(np.complex64) + 1j * pca.back_project(Q.imag)

        return _Field(self._analytic(pca.scores(), i), back, None, (mat,), pca)

    def transform(self, X=None, Y=None, normalized: bool = False):
        raise NotImplementedError("Hilbert models do not support the transform method.")


class ComplexCPCCARotator(ComplexPairSurface, CrossRotator):
    """Drop-in for xeofs.cross.ComplexCPCCARotator (cross/cpcca_rotator.py:472-534 over :20-420): Varimax
    (power = 1) / Promax rotation of a fitted complex cross model.  The stacked complex feature-space loadings [Qx; Qy] sqrt(s)
    are rotated on the device as one [Re | Im] panel (`rotation.cpromax_panel`); their images in the
    analysis space are Q sqrt(s) rotation_matrix -- k x k algebra (as in `CPCCARotator`)."""

    _model_name = "Rotated Complex CPCCA"
    _hilbert = False
    _score_dtype = np.complex64

    _rotate = staticmethod(rotation.cpromax_panel)

    def _adopt(self, model):
        self.pre = model.pre_re
        return {}

    def _pres(self):
        return self.pre

    @staticmethod
    def _model_vectors(model, i):
        return model.data[f"Q{i + 1}"]

    def _panel_sign(self, Xrot, ptot, k):
        """numpy's lexicographic complex max / min on the [Re | Im] panel"""
        amax, amin = engine.panel_colargminmax(self.ctx, Xrot, ptot)
        return cpanel.lex_sign(*cpanel.lex_extrema(Xrot, amax, amin, k, Xrot.shape[1] // 2))

    def _export(self, Xrot, lo, hi, idx, w):
        return cpanel.permute_export(self.ctx, Xrot[lo:], hi - lo, idx, w, Xrot.shape[1] // 2)

    def _unrotated_scores(self, which, Z, k):
        un = self.model.transform(**{"XY"[which - 1]: Z})          # unrotated scores: data . back-projected components
        vals, dims, coords, _, _ = labelled.unpack(un)
        S = np.asarray(vals).reshape(vals.shape[0], -1).T[:, :k]
        ok = ~np.isnan(S).all(axis=1)

        def label(proj, name):
            full = np.full(S.shape, np.nan, dtype=complex)
            full[ok] = proj
            return labelled.pack(full.T.reshape((k,) + vals.shape[1:]), dims, dict(coords, mode=np.arange(1, k + 1)), name,
                                 dict(self.attrs), un)

        return S[ok], label

    def transform(self, X=None, Y=None, normalized: bool = False):
        if self._hilbert:
            raise NotImplementedError("Hilbert models do not support the transform method.")
        return super().transform(X, Y, normalized)


class HilbertCPCCARotator(ComplexCPCCARotator):
    """Drop-in for xeofs.cross.HilbertCPCCARotator (cpcca_rotator.py:536-600); `transform` is not implemented there either."""

    _model_name = "Rotated Hilbert CPCCA"
    _hilbert = True


class ComplexMCARotator(ComplexCPCCARotator):
    """Drop-in for xeofs.cross.ComplexMCARotator (cross/mca_rotator.py:77-150)."""

    _model_name = "Rotated Complex MCA"


class HilbertMCARotator(HilbertCPCCARotator):
    """Drop-in for xeofs.cross.HilbertMCARotator (cross/mca_rotator.py:153-230)."""

    _model_name = "Rotated Hilbert MCA"


# --------------------------------------------------------------------------------------------------------------------
# the fixed-alpha children (cross/mca.py, cca.py, rda.py) and the rotator names of cross/cpcca_rotator.py, mca_rotator.py
# --------------------------------------------------------------------------------------------------------------------
def _fixed_alpha(base, alpha, name, doc):
    def __init__(self, n_modes: int = 2, **kwargs):
        kwargs.pop("alpha", None)
        base.__init__(self, n_modes=n_modes, alpha=alpha, **kwargs)
        self._params.pop("alpha", None)          # hard-coded for these classes (mca.py:120-123)
        self.attrs["model"] = name

    return type(name.replace(" ", ""), (base,), {"__init__": __init__, "__doc__": doc, "_model_name": name})


ComplexMCA = _fixed_alpha(ComplexCPCCA, [1.0, 1.0], "Complex MCA", "Drop-in for xeofs.cross.ComplexMCA (cross/mca.py:224-338).")
ComplexCCA = _fixed_alpha(ComplexCPCCA, [0.0, 0.0], "Complex CCA", "Drop-in for xeofs.cross.ComplexCCA (cross/cca.py:123-237).")
ComplexRDA = _fixed_alpha(ComplexCPCCA, [0.0, 1.0], "Complex RDA", "Drop-in for xeofs.cross.ComplexRDA (cross/rda.py:123-237).")
HilbertMCA = _fixed_alpha(HilbertCPCCA, [1.0, 1.0], "Hilbert MCA", "Drop-in for xeofs.cross.HilbertMCA (cross/mca.py:340-489).")
HilbertCCA = _fixed_alpha(HilbertCPCCA, [0.0, 0.0], "Hilbert CCA", "Drop-in for xeofs.cross.HilbertCCA (cross/cca.py:239-355).")
HilbertRDA = _fixed_alpha(HilbertCPCCA, [0.0, 1.0], "Hilbert RDA", "Drop-in for xeofs.cross.HilbertRDA (cross/rda.py:239-355).")
