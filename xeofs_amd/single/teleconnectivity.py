"""xeofs_amd.single.Teleconnectivity -- the teleconnectivity map [Wallace & Gutzler 1981, Mon. Wea. Rev. 109, 784-812,
"Teleconnections in the geopotential height field during the Northern Hemisphere winter"]: for every grid point, the strongest
NEGATIVE correlation it has with any other grid point, and the point it has it with.  The seesaws of the atmosphere (NAO, PNA,
...) were first read off this map.  The reference has no such model; the definition is stated here in full.

With Xc [n x p] the engine's preprocessed float32 matrix of the fit (centred, weights applied; with center=False its centred
twin stands in for it, `EOF._centred_twin`, as in EOT), x_j its column j,

    c_j   = |x_j|^2                                           (engine.feature_norms, squared)
    w_j   = 1 / sqrt(c_j), 0 where c_j = 0                    (float64, rounded once to float32: scale_vector)
    rmin_j, partner_j = min / argmin over i != j, w_i > 0 of (x_j . x_i w_j) w_i
                                                              (engine.mat_pairmin, csrc/eofx_pairmin.hpp: float32, int32;
                                                               the p x p correlation matrix never exists)
    teleconnectivity()    = -rmin_j                           as a map in the input's own coordinates (NaN for masked or
                                                               constant points)
    data["partner_index"] = partner_j                         (int64, valid-feature order, -1 where there is none)

The modes are the n_modes strongest seesaws that are mutually separated.  The candidates are the points with rmin_j < 0,
sorted by ascending rmin, the lowest index among equals (candidate_order); the blocked set starts empty; for k = 0, 1, ...:

    b, a    = the first candidate b such that neither b nor a = partner_b is blocked
    u_j     = x_j / |x_j|                                     (float64 on the host; x_b, x_a through engine.project with a
                                                               one-hot V)
    s_k     = sqrt(n - 1) (u_b - u_a) / 2                     (the half difference of the two standardised series)
    sh_k    = s_k / |s_k|
    R_b, R_a, comp_k = w * Xc^T [u_b, u_a, sh_k]              (ONE engine.panel_tmul of three columns at ctx.precision[1]: the
                                                               correlation of every point with the two poles and with the
                                                               index)
    block every j with max(|R_b[j]|, |R_a[j]|) > max_corr     (the poles themselves among them)

If the candidates run out before n_modes modes are found: ValueError.

    scores()             = s_k [n x k]
    components()         = comp_k [p x k]: the correlation of every point with the index, near +1 at b_k and -1 at a_k
    centre_mask()        = [p x k]: +1 at b_k, -1 at a_k, 0 elsewhere, in the input's own coordinates;
                           data["centre_index"] = [[b_k, a_k]] (int64, valid-feature order)
    singular_values()    = |Xc^T sh_k|,  explained_variance() = that^2 / (n - 1),  total_variance = sum_j c_j / (n - 1)
    transform(X')        = the fitted preprocessing, its 2K pole columns (engine.project with the one-hot matrix), each scaled
                           by the FIT's sqrt(n - 1) / |x_j|, half differences (half_differences)
    inverse_transform    raises NotImplementedError: the indices are not an expansion of the field

Deliberate choices: the feature weights (use_coslat, weights) do not change a correlation -- they only exclude
the points whose weight is 0; the lowest index wins every tie; the map is -rmin, so it is negative where a point has no
negatively correlated partner; the index is the two-pole form of Wallace & Gutzler's pattern indices; separation is by
correlation with the chosen poles, not by distance, so no coordinates are needed.  Out of scope: the sharded path, the
bootstrapper, rotation, complex data.

The host steps are module-level functions that need no GPU: scale_vector, candidate_order, select_pairs, half_differences.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled
from .eof import EOF
from .eot import one_hot


def scale_vector(c) -> np.ndarray:
    """w_j = 1 / sqrt(c_j) in float64, rounded once to float32; 0 where c_j > 0 fails"""
    c = np.asarray(c, dtype=np.float64)
    w = np.zeros(c.shape, dtype=np.float64)
    np.divide(1.0, np.sqrt(c, where=c > 0.0, out=np.ones_like(c)), out=w, where=c > 0.0)
    return w.astype(np.float32)


def candidate_order(rmin) -> np.ndarray:
    """the points with rmin_j < 0 by ascending rmin, the lowest index among equals (int64; NaN is never a candidate)"""
    rmin = np.asarray(rmin, dtype=np.float64)
    idx = np.flatnonzero(rmin < 0.0)
    return idx[np.argsort(rmin[idx], kind="stable")].astype(np.int64)


def select_pairs(rmin, partner, n_modes: int, max_corr: float, maps):
    """The greedy selection: -> the list of (b_k, a_k).  `maps`: a callable (k, b, a) -> (R_b, R_a), the correlation of every
    point with the two poles, or a precomputed [p x p] correlation matrix whose columns are read.  ValueError when the
    candidates run out before n_modes pairs are found."""
    partner = np.asarray(partner)
    p = partner.shape[0]
    blocked = np.zeros(p, dtype=bool)
    pairs = []
    cand = candidate_order(rmin)
    pos = 0
    for k in range(int(n_modes)):
        while pos < cand.size and (blocked[cand[pos]] or partner[cand[pos]] < 0 or blocked[partner[cand[pos]]]):
            pos += 1
        if pos == cand.size:
            raise ValueError(f"n_modes must be less than or equal to the number of separated seesaws: the field is exhausted "
                             f"after {k} modes (every remaining point with a negatively correlated partner correlates above "
                             f"max_corr = {max_corr} with a pole already chosen).")
        b, a = int(cand[pos]), int(partner[cand[pos]])
        if callable(maps):
            Rb, Ra = maps(k, b, a)
        else:
            Rb, Ra = np.asarray(maps)[:, b], np.asarray(maps)[:, a]
        pairs.append((b, a))
        blocked |= np.maximum(np.abs(np.asarray(Rb, dtype=np.float64)), np.abs(np.asarray(Ra, dtype=np.float64))) > max_corr
        blocked[[b, a]] = True                         # (their own correlation is 1 up to rounding: said, not relied on)
    return pairs


def half_differences(B, scale) -> np.ndarray:
    """s_k = (B[:, 2k] scale[2k] - B[:, 2k + 1] scale[2k + 1]) / 2: B [n x 2K] the pole columns (b_0, a_0, b_1, a_1, ...) of a
    field, scale [2K] the sqrt(n - 1) / |x_j| of the fit; float64"""
    Z = np.asarray(B, dtype=np.float64) * np.asarray(scale, dtype=np.float64)[None, :]
    return 0.5 * (Z[:, 0::2] - Z[:, 1::2])


def _check_max_corr(max_corr) -> float:
    if not isinstance(max_corr, (int, float, np.integer, np.floating)) or not (0.0 < max_corr < 1.0):
        raise ValueError(f"max_corr must lie strictly between 0 and 1, got {max_corr!r}")
    return float(max_corr)


class Teleconnectivity(EOF):
    """The teleconnectivity map and its strongest separated seesaws.  teleconnectivity() is the map, scores() the two-pole
    indices, components() the correlation of every point with them, centre_mask() marks the poles."""

    def __init__(self, n_modes: int = 2, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 check_nans=True, sample_name: str = "sample", feature_name: str = "feature", compute: bool = True,
                 random_state: int | None = None, solver: str = "auto", solver_kwargs: dict = {},
                 max_corr: float = 0.5, **kwargs):
        max_corr = _check_max_corr(max_corr)
        if not isinstance(n_modes, (int, np.integer)) or n_modes < 1:
            raise ValueError(f"Teleconnectivity takes a positive integer n_modes, got {n_modes!r}")
        super().__init__(n_modes=n_modes, center=center, standardize=standardize, use_coslat=use_coslat,
                         check_nans=check_nans, sample_name=sample_name, feature_name=feature_name, compute=compute,
                         random_state=random_state, solver=solver, solver_kwargs=solver_kwargs, **kwargs)
        self.attrs.update({"model": "Teleconnectivity", "max_corr": max_corr})
        self._params.update({"max_corr": max_corr, "solver_kwargs": dict(solver_kwargs)})

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
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

    def _fit_algorithm(self, mat, omega=None, dec=None):
        """the module's equations on the resident, centred, preprocessed field `mat`"""
        ctx = self.ctx
        n, p = mat.shape
        K, max_corr = int(self.n_modes), self._params["max_corr"]
        if n < 2:
            raise ValueError(f"Teleconnectivity needs at least two samples, got n_samples = {n}")
        ms = dict(pairmin=0.0, series=0.0, tmul=0.0)
        tick = time.perf_counter
        c = engine.feature_norms(ctx, mat) ** 2
        w = scale_vector(c)
        t0 = tick()
        had_layout = mat.has_sample_layout()
        try:
            rmin, partner = engine.mat_pairmin(ctx, mat, w)
            rmin, partner = rmin.cpu().numpy(), partner.cpu().numpy().astype(np.int64)
        finally:
            if not had_layout:
                mat.release_sample_layout()
        ms["pairmin"] = 1e3 * (tick() - t0)
        w64 = w.astype(np.float64)
        S, comps, norms, scale = [], [], [], []

        def maps(k, b, a):
            t1 = tick()
            x = engine.project(ctx, mat, one_hot(p, [b, a])).astype(np.float64)
            xn = np.sqrt(np.sum(x * x, axis=0))
            u = x / xn
            s = np.sqrt(n - 1.0) * (u[:, 0] - u[:, 1]) / 2.0
            sh = s / np.sqrt(s @ s)
            t2 = tick()
            Zn = engine.panel_import(ctx, np.ascontiguousarray(np.column_stack([u, sh]), dtype=np.float32), mat.n_pad,
                                     engine.panel_width(3))
            out = engine.panel_tmul(ctx, mat, Zn, prec=ctx.precision[1])
            W = mat.compact_rows(engine.panel_export(ctx, out, mat.p_phys, 3)).astype(np.float64)
            t3 = tick()
            ms["series"] += 1e3 * (t2 - t1)
            ms["tmul"] += 1e3 * (t3 - t2)
            S.append(s)
            comps.append(w64 * W[:, 2])
            norms.append(float(np.sqrt(W[:, 2] @ W[:, 2])))
            scale.extend((np.sqrt(n - 1.0) / xn).tolist())
            return w64 * W[:, 0], w64 * W[:, 1]

        pairs = select_pairs(rmin, partner, K, max_corr, maps)
        norms = np.asarray(norms)
        Sc = np.ascontiguousarray(np.stack(S, axis=1), dtype=np.float32)
        self._pole_scale = np.asarray(scale, dtype=np.float64)
        self.data = dict(input_data=Sc, components=np.ascontiguousarray(np.stack(comps, axis=1), dtype=np.float32), scores=Sc,
                         teleconnectivity=-rmin, partner_index=partner, centre_index=np.asarray(pairs, dtype=np.int64),
                         norms=norms, explained_variance=norms ** 2 / (n - 1.0), total_variance=float(c.sum()) / (n - 1.0))
        self.stats = {f"ms_{name}": v for name, v in ms.items()}
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X):
        """new data -> the fitted preprocessing -> its 2K pole columns -> the half differences at the fit's scales"""
        self.compute()
        mat, fields, vs = self.preprocessor.transform(X)
        try:
            B = engine.project(self.ctx, mat, one_hot(mat.p, self.data["centre_index"].reshape(-1)))
        finally:
            mat.free()
        S = half_differences(B, self._pole_scale).astype(np.float32)
        return self.preprocessor.inverse_transform_scores(S, "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores):
        raise NotImplementedError("Teleconnectivity has no inverse_transform: the indices are not an expansion of the field")

    # ------------------------------------------------------------------ accessors
    def components(self):
        """the correlation of every point with the index of each mode"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def scores(self):
        """the two-pole indices s_k"""
        return self.preprocessor.inverse_transform_scores(self.data["scores"], "scores", self.attrs)

    def centre_mask(self):
        """+1 at b_k, -1 at a_k, 0 elsewhere, in the input's own coordinates (NaN where the input is masked)"""
        p = self.data["components"].shape[0]
        ci = self.data["centre_index"]
        return self.preprocessor.inverse_transform_components(one_hot(p, ci[:, 0]) - one_hot(p, ci[:, 1]), "centre_mask",
                                                              self.attrs)

    def teleconnectivity(self):
        """-rmin_j as a map in the input's own coordinates: NaN for masked or constant points"""
        self.compute()
        pre = self.preprocessor
        full = np.full(pre.valid_feature.size, np.nan, dtype=np.float32)
        full[pre.valid_feature] = self.data["teleconnectivity"]
        outs, off = [], 0
        for f in pre.fields:
            blk = full[off:off + f.P].reshape(f.feature_shape)
            off += f.P
            outs.append(labelled.pack(blk, f.feature_dims, {d: f.coords[d] for d in f.feature_dims}, "teleconnectivity",
                                      dict(self.attrs), f.like))
        return pre._wrap(outs)
