"""GPU tests of empirical orthogonal teleconnections (xeofs_amd.single.EOT).

The checker is the float64 restatement of tests/eot_reference.py, which shares no code with the model.

  * Base points.  On the designed field the runner-up of every mode scores below 0.95 of the winner (asserted with the
    restatement first), so the model must name exactly the designated columns.  On random fields a near-tie may fall either
    way: every base point the model chose must have a float64 score within

        4 (bound_b / den_b + bound_m / den_m)

    of the float64 maximum at that step (m the float64 winner), where bound_j = 1.01 (n + 8) 2^-24 sum |x_j| |A_k| |x_j| is the
    bound of the quadratic-form kernel (tests/test_gpu_colquad.py) and den_j the squared residual norm: the model prefers b to
    m only if its own scores say so, and each of the two is off by its kernel error over den; the factor 4 covers the float32
    rounding of A_k and of the products behind den.
  * Values.  The restatement FED THE MODEL'S OWN BASE POINTS must match scores(), components(), explained_variance() and
    inverse_transform().  The tolerance is derived, not chosen, and never from EOT's own output: the same float64 comparison is
    run on the two engine products EOT is made of -- engine.project (X V) and engine.panel_tmul (X^T Z) of the EOF model, on
    the same resident field with random orthonormal V and Z rounded to float32, and the squared column norms of X^T Z -- and
    the tolerance is four times the largest relative error seen there (`calibration`), because the EOT outputs are those
    products divided by O(1) norms.  Measured on an MI355X: see DESIGN.md section 22 and the comment at `calibration`.
"""

import numpy as np
import pytest

import eot_reference as er

pytestmark = pytest.mark.gpu

K = 4
LATS = {7: np.linspace(-60.0, 60.0, 7), 3: np.array([10.0, 35.0, 70.0]), 5: np.linspace(-80.0, 40.0, 5)}


def random_field(n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 6)) @ (rng.standard_normal((6, p)) * np.linspace(3.0, 0.5, 6)[:, None])
    return (X + 0.3 * rng.standard_normal((n, p)) + 2.0).astype(np.float32)


def grid(X, nlat):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X.reshape(n, nlat, p // nlat), ("time", "lat", "lon"),
                        {"time": np.arange(n), "lat": LATS[nlat], "lon": np.arange(p // nlat) * 2.5})


CASES = {
    "plain_33x70": dict(n=33, p=70, nlat=7),
    "coslat_weights_64x129": dict(n=64, p=129, nlat=3, use_coslat=True, weights=True),
    "standardize_130x65": dict(n=130, p=65, nlat=5, standardize=True),
    "uncentred_33x70": dict(n=33, p=70, nlat=7, center=False),
    "dataset_64x129": dict(n=64, p=129, nlat=3, dataset=True),
    "land_mask_130x65": dict(n=130, p=65, nlat=5, mask=True),
}
_cache = {}


def flat(obj, k):
    """components-like output (array, or dataset of arrays) -> [k x P] in stacked feature order"""
    if hasattr(obj, "data_vars"):
        return np.concatenate([np.asarray(obj[v].values).reshape(k, -1) for v in obj.data_vars], axis=1)
    return np.asarray(obj.values).reshape(k, -1)


def rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def calibration(ctx, mat, Xt):
    """the largest relative error of the EOF model's two products on this resident field against float64.
    Measured on an MI355X over the six cases: between 1.10e-7 (uncentred_33x70) and 2.84e-7 (plain_33x70), so the derived
    tolerances lie between 4.4e-7 and 1.14e-6; the largest error of an EOT output seen against them was 2.9e-7 (the
    explained variance of plain_33x70), 1.6e-7 on scores and components."""
    from xeofs_amd import engine

    n, p = Xt.shape
    rng = np.random.default_rng(11)
    X64 = Xt.astype(np.float64)
    V64 = np.linalg.qr(rng.standard_normal((p, K)))[0]
    Z64 = np.linalg.qr(rng.standard_normal((n, K)))[0]
    S = engine.project(ctx, mat, V64.astype(np.float32))
    Zp = engine.panel_import(ctx, np.ascontiguousarray(Z64, dtype=np.float32), mat.n_pad, engine.panel_width(K))
    W = engine.panel_export(ctx, engine.panel_tmul(ctx, mat, Zp, prec=ctx.precision[1]), mat.p_phys, K)
    Wref = X64.T @ Z64
    sq, sqref = np.sum(W.astype(np.float64) ** 2, axis=0), np.sum(Wref ** 2, axis=0)
    return max(rel(S, X64 @ V64), rel(W, Wref), float(np.max(np.abs(sq - sqref) / sqref)))


def fitted(ctx, name):
    """the fitted model of a case, its input, the preprocessed float32 field the fit saw, the restatement fed the model's own
    base points, and the derived tolerance: computed once and shared (nothing changes them)"""
    import xeofs_amd as xe
    from xeofs_amd import engine

    if name not in _cache:
        c = CASES[name]
        n, p, nlat = c["n"], c["p"], c["nlat"]
        X = random_field(n, p, seed=len(name) + n)
        if c.get("mask"):
            X[:, np.arange(p) % 4 == 1] = np.nan
        weights = None
        if c.get("dataset"):
            pa = nlat * 30
            inp = xe.Dataset({"a": grid(X[:, :pa], nlat),
                              "b": xe.DataArray(X[:, pa:], ("time", "x"), {"time": np.arange(n), "x": np.arange(p - pa)})})
        else:
            inp = grid(X, nlat)
            if c.get("weights"):
                wv = np.random.default_rng(3).random((nlat, p // nlat)) * 1.5 + 0.25
                weights = xe.DataArray(wv, ("lat", "lon"), {"lat": LATS[nlat], "lon": np.arange(p // nlat) * 2.5})
        m = xe.single.EOT(n_modes=K, standardize=bool(c.get("standardize")), use_coslat=bool(c.get("use_coslat")),
                          center=c.get("center", True))
        m.ctx = ctx
        m.fit(inp, dim="time", weights=weights)
        pre = m.preprocessor
        mat, st = engine.preprocess(ctx, X, True, bool(c.get("standardize")), pre.feature_weights, in_place=True)
        try:
            assert np.array_equal(st["valid_feature"], pre.valid_feature) and not mat.masked
            Xt = mat.download()
            tol = 4.0 * calibration(ctx, mat, Xt)
        finally:
            mat.free()
        ref = er.gram_form(Xt, K, base=m.data["base_index"])
        print(f"{name}: derived tolerance {tol:.3e}")
        _cache[name] = (m, inp, X, Xt, ref, tol)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ (i) the designed field
def test_designed_field_names_its_base_points(ctx):
    import xeofs_amd as xe

    X = er.designed_field()
    ref = er.textbook(X, 3)
    for k in range(3):
        s = np.sort(ref["all_scores"][k])[::-1]
        assert s[1] < 0.95 * s[0]                                      # the margin first: 0.882, 0.869, 0.797
    assert tuple(ref["base"]) == er.DESIGNED_BASE
    m = xe.single.EOT(n_modes=3)
    m.ctx = ctx
    m.fit(xe.DataArray(X.astype(np.float32), ("time", "x"), {"time": np.arange(X.shape[0]), "x": np.arange(36)}), dim="time")
    assert tuple(m.data["base_index"]) == er.DESIGNED_BASE
    mask = m.base_point_mask()
    assert mask.dims == ("mode", "x") and np.array_equal(np.argmax(mask.values, axis=1), er.DESIGNED_BASE)
    assert np.array_equal(mask.values.sum(axis=1), np.ones(3))


# ------------------------------------------------------------------------------------------------ (ii) random fields
@pytest.mark.parametrize("name", list(CASES))
def test_base_points_are_float64_maxima_up_to_the_kernel_bound(ctx, name):
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    n, p = Xt.shape
    base = m.data["base_index"]
    assert base.dtype == np.int64 and base.shape == (K,) and len(set(base.tolist())) == K
    X64 = Xt.astype(np.float64)
    G = X64 @ X64.T
    for k in range(K):
        T = ref["series"][:, :k] / np.sqrt(np.sum(ref["series"][:, :k] ** 2, axis=0))
        P = np.eye(n) - T @ T.T
        A = P @ G @ P
        bound = 1.01 * (n + 8) * 2.0 ** -24 * np.einsum("sj,st,tj->j", np.abs(X64), np.abs(A), np.abs(X64))
        score, den = ref["all_scores"][k], ref["den"][k]
        b, w = int(base[k]), int(np.argmax(score))
        slack = 4.0 * (bound[b] / den[b] + bound[w] / den[w])
        print(f"{name} mode {k}: base {b}, float64 winner {w}, gap {score[w] - score[b]:.3e}, allowed {slack:.3e}")
        assert score[b] > 0.0 and score[w] - score[b] <= slack


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_against_the_restatement_fed_the_models_base_points(ctx, name):
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    n, p = Xt.shape
    pre = m.preprocessor
    vf = pre.valid_feature
    assert sorted(m.data) == sorted(["input_data", "components", "scores", "base_index", "norms", "explained_variance",
                                     "total_variance"])
    assert set(m.stats) == {"ms_gram", "ms_colquad", "ms_select", "ms_series", "ms_tmul", "ms_deflate"}
    S = np.asarray(m.scores().values)
    assert S.shape == (K, n) and S.dtype == np.float32
    C = flat(m.components(), K)[:, vf]
    errs = dict(scores=rel(S.T, ref["series"]), components=rel(C.T, ref["patterns"]))
    ev, evo = m.data["explained_variance"], ref["score"] / (n - 1.0)
    errs["explained_variance"] = float(np.max(np.abs(ev - evo) / evo))
    tv = np.sum(Xt.astype(np.float64) ** 2) / (n - 1.0)
    errs["total_variance"] = abs(m.data["total_variance"] - tv) / tv
    # inverse_transform of the model's scores: R beta^T through the inverse preprocessing, in float64
    rec = ref["series"] @ ref["patterns"].T
    if pre.feature_weights is not None:
        rec = rec / pre.feature_weights[vf]
    if pre.std_ is not None:
        rec = rec * pre.std_[vf]
    scale = np.abs(rec).max()
    if pre.mean_ is not None:
        rec = rec + pre.mean_[vf]
    got = m.inverse_transform(m.scores())
    got = flat_data(got, n)[:, vf]
    errs["inverse_transform"] = float(np.abs(got - rec).max() / scale)
    print(f"{name}: tolerance {tol:.3e}, relative errors {errs}")
    for key, e in errs.items():
        assert e <= tol, (key, e, tol)
    np.testing.assert_array_equal(np.asarray(m.explained_variance().values), ev)
    np.testing.assert_allclose(np.asarray(m.singular_values().values), np.sqrt(ev * (n - 1.0)), rtol=1e-15)
    np.testing.assert_allclose(np.asarray(m.explained_variance_ratio().values), ev / m.data["total_variance"], rtol=1e-15)
    # beta_k[b_k] = 1 and the series are orthogonal, to the same tolerance
    base = m.data["base_index"]
    assert np.abs(C[np.arange(K), base] - 1.0).max() <= tol * np.abs(ref["patterns"]).max()
    Gm = S.astype(np.float64) @ S.astype(np.float64).T
    assert np.abs(Gm - np.diag(np.diag(Gm))).max() <= 4 * tol * np.diag(Gm).max()
    # the base points carry the input's own coordinates; masked features are NaN
    mask = flat(m.base_point_mask(), K)
    assert np.all(np.isnan(mask[:, ~vf])) and np.array_equal(np.argmax(mask[:, vf], axis=1), base)
    assert np.array_equal(np.nansum(mask, axis=1), np.ones(K))
    assert type(m.base_point_mask()) is type(m.components())


def flat_data(obj, n):
    """reconstructed data (array with time first, or dataset of such) -> [n x P]"""
    if hasattr(obj, "data_vars"):
        return np.concatenate([np.asarray(obj[v].values).reshape(n, -1) for v in obj.data_vars], axis=1)
    return np.asarray(obj.values).reshape(n, -1)


# ------------------------------------------------------------------------------------------------ (iii) identical columns
def test_a_duplicate_of_a_base_point_is_never_chosen(ctx):
    import xeofs_amd as xe

    X = random_field(40, 30, seed=4)
    b0 = int(er.textbook(X - X.mean(axis=0), 1)["base"][0])
    dup = (b0 + 11) % 30
    X[:, dup] = X[:, b0]
    m = xe.single.EOT(n_modes=6)
    m.ctx = ctx
    m.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(40), "x": np.arange(30)}), dim="time")
    base = m.data["base_index"].tolist()
    assert base[0] == min(b0, dup)                                     # identical series, identical arithmetic: the lowest index
    assert max(b0, dup) not in base and len(set(base)) == 6


# ------------------------------------------------------------------------------------------------ (iv) transform
@pytest.mark.parametrize("name", ["plain_33x70", "coslat_weights_64x129", "standardize_130x65", "dataset_64x129",
                                  "land_mask_130x65"])
def test_transform_of_the_training_data_returns_the_scores(ctx, name):
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    got = m.transform(inp)
    S = m.scores()
    assert got.dims == S.dims and got.values.shape == S.values.shape
    assert rel(got.values, S.values) <= tol


# ------------------------------------------------------------------------------------------------ (v) beyond the rank
def test_n_modes_beyond_the_rank_raises(ctx):
    import xeofs_amd as xe

    X = random_field(8, 20, seed=1)
    arr = xe.DataArray(X, ("time", "x"), {"time": np.arange(8), "x": np.arange(20)})
    m = xe.single.EOT(n_modes=7)
    m.ctx = ctx
    m.fit(arr, dim="time")                                             # the rank of a centred field of 8 samples
    for k in (8, 9):
        m = xe.single.EOT(n_modes=k)
        m.ctx = ctx
        with pytest.raises(ValueError, match="less than or equal to the rank"):
            m.fit(arr, dim="time")
