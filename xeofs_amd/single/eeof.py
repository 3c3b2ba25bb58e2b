"""xeofs_amd.single.ExtendedEOF -- drop-in for xeofs.single.ExtendedEOF (xeofs/single/eeof.py:10-179): Extended EOF
analysis (multichannel singular spectrum analysis), an EOF of the delay-embedded field

    X_ext[t, (e, j)] = X[t + e tau, j],      t < n' = n - (embedding - 1) tau,  e < embedding,

centred per embedded column over its own window (the reference's inner `EOF(center=True)`, eeof.py:138-150).

The reference concatenates the `embedding` shifted copies of the field (eeof.py:124-134), E times its memory.  Here the
randomized decomposition runs on the embedding as an OPERATOR (`LagOps`, csrc/eofx_lag.hpp): both products read the
resident field once per group of lags, the lags live on the small sample-side panel and the window means ride along as a
rank-one correction.  Only the exact / wide branches of the solver ladder and the PCA route, where the embedded matrix is
small, write it (`eofx_lag_embed_f32`).
"""

from __future__ import annotations

import numpy as np

from .. import engine, labelled
from ..linalg.decomposer import Decomposer
from ..sharded import Comm, HipPanelOps, sharded_rsvd
from .eof import EOF


class LagOps(HipPanelOps):
    """Panel products of the centred embedded matrix X_ext - 1 mu^T (n' x E p) on the resident preprocessed field.
    Feature-side panels are lag-major, (E p_pad) x L: row e p_pad + j, zero padding rows j >= p in every lag block;
    sample-side panels are n'_pad x L.  The matrix-independent steps (Gram, Cholesky-QR, matmul) are the base class's."""

    def __init__(self, ctx, mat, tau, embedding, mean):
        super().__init__(ctx, mat)
        self.tau, self.E, self.mean = int(tau), int(embedding), mean
        self.p_field, self.p_pad_field = mat.p, mat.p_pad
        self.n = engine.lag_samples(mat, tau, embedding)
        self._n_pad_engine = (self.n + 511) // 512 * 512
        self.p, self.p_pad = self.E * mat.p, self.E * mat.p_pad
        # the two sides must differ in their panel row counts (the driver tells them apart by shape): where they would
        # coincide, the sample side gets one more 512-row block of zeros
        self.n_pad = self._n_pad_engine + (512 if self._n_pad_engine == self.p_pad else 0)
        self.p_rows = self.p_pad        # feature-side rows that may carry data (padding rows interleave the lag blocks)

    def _feature_panel(self, P, rows):
        return P.shape[0] == self.p_pad and rows == self.p

    def import_panel(self, src, side):
        if side == "n":
            return super().import_panel(src, side)
        l = src.shape[1]
        src = np.asarray(src.detach().cpu().numpy() if hasattr(src, "detach") else src, dtype=np.float32)
        padded = np.zeros((self.E, self.p_pad_field, l), np.float32)
        padded[:, :self.p_field] = src.reshape(self.E, self.p_field, l)
        return self.e.panel_import(self.ctx, padded.reshape(self.p_pad, l), self.p_pad, self.e.panel_width(l))

    def tmul(self, Zn, final=False):
        return self.e.lag_tmul(self.ctx, self.mat, self.tau, self.E, self.mean, Zn, prec=self.ctx.precision[1 if final else 0])

    def mul(self, Yp, final=False):
        out = None
        if self.n_pad != self._n_pad_engine:
            torch = self.e._torch()
            out = torch.zeros((self.n_pad, Yp.shape[1]), dtype=torch.float32, device=Yp.device)
        return self.e.lag_mul(self.ctx, self.mat, self.tau, self.E, self.mean, Yp, out=out,
                              prec=self.ctx.precision[1 if final else 0])

    def colminmax(self, P, rows):
        if self._feature_panel(P, rows):
            rows = self.p_pad            # zero padding rows cannot change which of |max|, |min| is larger
        return self.e.panel_colminmax(self.ctx, P, rows)

    def export(self, P, rows, k, sign=None, device_out=False):
        if not self._feature_panel(P, rows):
            return self.e.panel_export(self.ctx, P, rows, k, sign, device_out)
        out = self.e.panel_export(self.ctx, P, self.p_pad, k, sign, device_out)      # drop the padding rows of every lag block
        out = out.reshape(self.E, self.p_pad_field, k)[:, :self.p_field].reshape(self.p, k)
        return out.contiguous() if device_out else np.ascontiguousarray(out)


def _positive_int(name, v, allow_none=False):
    if v is None and allow_none:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


class ExtendedEOF(EOF):
    """Drop-in for xeofs.single.ExtendedEOF (xeofs/single/eeof.py:10-179): Extended EOF analysis [Weare & Nasstrom 1982;
    Broomhead & King 1986].  `tau` is the delay between the embedded copies, `embedding` their number; with `n_pca_modes`
    the field is first reduced to that many PCA scores and the embedding is built on those.

    The shift is positional along the stacked, sanitised sample axis.  `scores()` is NaN on the last (embedding - 1) tau
    valid samples; `components()` has dims (mode, embedding, *feature_dims) with embedding = arange(embedding) tau.
    `transform` is not supported (as in the reference).

    Two deliberate deviations from the reference:
      1. `random_state` is forwarded to the inner PCA and EOF (the reference leaves both unseeded, so its EEOF is not
         reproducible);
      2. `embedding=1` is the plain EOF of the field (n' = n; the reference's `slice(None, -0)` empties the sample axis).
    """

    def __init__(self, n_modes: int, tau: int, embedding: int, n_pca_modes: int | None = None, center: bool = True,
                 standardize: bool = False, use_coslat: bool = False, check_nans: bool = True, sample_name: str = "sample",
                 feature_name: str = "feature", compute: bool = True, solver: str = "auto", random_state: int | None = None,
                 solver_kwargs: dict = {}, **kwargs):
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs, **kwargs)
        self.tau = _positive_int("tau", tau)
        self.embedding = _positive_int("embedding", embedding)
        self.n_pca_modes = _positive_int("n_pca_modes", n_pca_modes, allow_none=True)
        self.attrs.update({"model": "Extended EOF Analysis"})
        self._params.update({"tau": tau, "embedding": embedding, "n_pca_modes": n_pca_modes})

    # ------------------------------------------------------------------ fit
    def _check_length(self, n):
        n_emb = n - (self.embedding - 1) * self.tau
        if n_emb < 2:
            raise ValueError(f"embedding={self.embedding} with tau={self.tau} needs more than {(self.embedding - 1) * self.tau + 1} "
                             f"samples; the data have {n} (the embedded series would have {n_emb})")
        return n_emb

    @staticmethod
    def _n_samples(X, dim):
        vals, dims, _, _, _ = labelled.unpack(labelled.first_array(X))
        sd = (dim,) if isinstance(dim, str) else tuple(dim)
        return int(np.prod([vals.shape[dims.index(d)] for d in sd if d in dims], dtype=np.int64))

    def _fit_now(self, X, dim, weights=None):
        self._check_length(self._n_samples(X, dim))
        self._decomposer_kwargs["lazy_input"] = labelled.is_lazy(X)
        mat = self._preprocess(X, dim, weights)
        n_emb = self._check_length(mat.n)           # (samples dropped by the Sanitizer shorten the series)
        if self.n_pca_modes:
            return self._fit_pca(mat, X, dim, weights, n_emb)
        return self._fit_direct(mat, n_emb)

    def _inner_decomposer(self):
        return Decomposer(ctx=self.ctx, **self._decomposer_kwargs)

    def _fit_direct(self, mat, n_emb):
        ctx, E, tau = self.ctx, self.embedding, self.tau
        dec = self._inner_decomposer()
        k, n_over, n_iter, wide = dec.policy(n_emb, E * mat.p)
        if wide or n_iter == 0:       # exact / wide branch: the embedded matrix is small enough to write
            inner, tv = self._embedded_matrix(mat, E * mat.p)
            dec.fit(inner, total_variance=tv)
            inner.free()
        else:                         # randomized branch: the embedding stays an operator on the resident field
            mean, tv = engine.lag_stats(ctx, mat, tau, E)
            ops = LagOps(ctx, mat, tau, E, mean)
            U, s, V = sharded_rsvd(ops, Comm(), k, E * mat.p, 0, n_over, n_iter, random_state=dec.random_state,
                                   flip=bool(dec.flip_signs))
            dec.n_modes_precompute = k
            dec._finish(U, s, V, n_emb, k, tv)
        return self._store(mat, dec.U_, dec.s_, dec.V_, tv, n_emb)

    def _embedded_matrix(self, mat, width):
        """the centred embedded matrix of `mat` as a resident matrix (eofx_lag_embed_f32 + the engine's centring) and its total
        variance; MemoryError when it does not fit in HBM"""
        torch = engine._torch()
        n_emb = engine.lag_samples(mat, self.tau, self.embedding)
        need = 4 * n_emb * width
        free, _ = torch.cuda.mem_get_info(self.ctx.device)
        if 3 * need + (1 << 30) > free:      # the embedded matrix and the two layouts of its centred copy
            raise MemoryError(f"the embedded matrix ({n_emb} x {width}, {need / 1e9:.1f} GB) does not fit in device memory for "
                              "the exact decomposition; solver=\"randomized\" decomposes the embedding as an operator without "
                              "writing it")
        emb = engine.lag_embed(self.ctx, mat, self.tau, self.embedding)
        inner, st = engine.preprocess(self.ctx, emb, center=True, check_nans=False)
        del emb
        return inner, st["total_variance"]

    def _fit_pca(self, mat, X, dim, weights, n_emb):
        """eeof.py:99-122, 157-162: PCA scores of the (centred) preprocessed field, their embedding, a small EOF on it;
        components = V_pca V_eeof on the device."""
        ctx, E, tau, m = self.ctx, self.embedding, self.tau, self.n_pca_modes
        pmat = self._centred_twin(mat, X, dim, weights)
        # exactly these arguments, not Decomposer.for_model: the model's `solver` and `compute` do not reach the inner PCA.
        # Honouring `solver` would change results and belongs to an issue of its own.
        pca = Decomposer(n_modes=m, ctx=ctx, random_state=self._params["random_state"],
                         solver_kwargs=self._decomposer_kwargs.get("solver_kwargs", {}))
        pca.fit(pmat)
        if pmat is not mat:
            pmat.free()
        Vp = np.asarray(pca.V_, dtype=np.float32)                         # p x m
        m = Vp.shape[1]
        scores = np.ascontiguousarray(pca.U_ * pca.s_, dtype=np.float32)  # n x m
        smat = engine.from_dense(ctx, scores)
        inner, tv = self._embedded_matrix(smat, E * m)
        smat.free()
        dec = self._inner_decomposer()
        dec.fit(inner, total_variance=tv)
        inner.free()
        # components: V_pca (p x m) times the lag blocks of V_eeof (E m x k) as ONE panel product (p x E k), lag-major after
        torch = engine._torch()
        Ve = np.asarray(dec.V_, dtype=np.float64)
        k = Ve.shape[1]
        L = engine.panel_width(m)
        P = engine.panel_import(ctx, Vp, (Vp.shape[0] + 511) // 512 * 512, L)
        M = np.zeros((L, engine.panel_width(E * k)))
        M[:m, :E * k] = Ve.reshape(E, m, k).transpose(1, 0, 2).reshape(m, E * k)
        C = engine.panel_matmul(ctx, P, torch.as_tensor(M, device=P.device))
        p = Vp.shape[0]
        V = C[:p, :E * k].reshape(p, E, k).permute(1, 0, 2).reshape(E * p, k).cpu().numpy()
        return self._store(mat, dec.U_, dec.s_, np.ascontiguousarray(V), tv, n_emb)

    def _store(self, mat, U, s, V, total_variance, n_emb):
        s64 = np.asarray(s, dtype=np.float64)
        scores = np.full((mat.n, len(s64)), np.nan, np.float32)        # the last (E - 1) tau samples have no embedded row
        scores[:n_emb] = np.asarray(U) * np.asarray(s, dtype=np.float32)
        self.data = dict(input_data=mat, components=np.asarray(V, dtype=np.float32), scores=scores, norms=s64,
                         explained_variance=s64 ** 2 / (n_emb - 1), total_variance=total_variance)
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X, normalized: bool = False):
        raise NotImplementedError("EEOF does currently not support transform")

    def inverse_transform(self, scores, normalized: bool = False):
        """eeof.py:171-179: scores times the lag-0 slice of the components (the inner window means are not added back),
        then the outer Preprocessor un-scales."""
        self.compute()
        S, modes, vs, fields = self._parse_scores(scores, normalized, np.float32)
        p = self.data["components"].shape[0] // self.embedding
        V = np.ascontiguousarray(self.data["components"][:p, modes - 1])
        rec = engine.reconstruct(self.ctx, S, V)
        return self.preprocessor.inverse_transform_data(rec, "reconstructed_data", fields, vs)

    # ------------------------------------------------------------------ accessors
    def components(self, normalized: bool = True):
        V = self.data["components"]
        if not normalized:
            V = V * self.data["norms"].astype(V.dtype)
        p = V.shape[0] // self.embedding
        per = [self.preprocessor.inverse_transform_components(np.ascontiguousarray(V[e * p:(e + 1) * p]), "components",
                                                              self.attrs) for e in range(self.embedding)]
        coord = np.arange(self.embedding) * self.tau

        def stack(objs):      # (mode, *feature_dims) per lag -> (mode, embedding, *feature_dims)
            vals, dims, coords, name, attrs = labelled.unpack(objs[0])
            out = np.stack([np.asarray(labelled.unpack(o)[0]) for o in objs], axis=1)
            return labelled.pack(out, (dims[0], "embedding") + tuple(dims[1:]), dict(coords, embedding=coord), name, attrs,
                                 objs[0])

        first = per[0]
        if labelled.is_dataset(first):
            return labelled.make_dataset(first, {v: stack([o[v] for o in per]) for v in first.data_vars})
        if isinstance(first, list):
            return [stack([o[i] for o in per]) for i in range(len(first))]
        return stack(per)
