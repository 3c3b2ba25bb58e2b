"""GPU tests of the teleconnectivity model (xeofs_amd.single.Teleconnectivity).

The checker is the float64 restatement of tests/teleconnectivity_reference.py, which shares no code with the model and is FED
THE ENGINE'S float32 preprocessed matrix and THE MODEL'S OWN pairs.

  * The map.  teleconnectivity() = -rmin must lie within B_j of float64, B_j the row maximum of the bound of the
    pairwise-minimum kernel (tests/test_gpu_pairmin.py; teleconnectivity_reference.pair_bound).
  * The pairs.  On the designed field the margins are asserted on the restatement first (0.03 against bounds below 3e-4:
    tests/test_teleconnectivity_reference_cpu.py), so the model must name the planted pairs in order.  On random fields a near
    tie may fall either way: the base b of every step must be open in float64 and have rmin64[b] within 2 max(B_b, B_m) of
    the float64 winner m of that step (the model prefers b to m only if its own float32 minima say so, and each is off by at
    most its B), and its partner a must have r64[b, a] <= rmin64[b] + 2 B_b.
  * Values.  scores(), components(), singular_values() and the variances against the restatement.  The tolerance is derived,
    not chosen, and never from the model's own output: the same float64 comparison is run on the two engine products the
    model is made of -- engine.project (X V) and engine.panel_tmul (X^T Z) of the EOF model, on the same resident field with
    random orthonormal V and Z rounded to float32, and the squared column norms of X^T Z -- and the tolerance is four times
    the largest relative error seen there (`calibration`, as tests/test_gpu_eot.py derives its own).
"""

import numpy as np
import pytest

import teleconnectivity_reference as tr

pytestmark = pytest.mark.gpu

K = 3
MAX_CORR = 0.6
LATS = {6: np.linspace(-50.0, 50.0, 6), 4: np.array([-20.0, 10.0, 35.0, 70.0])}


def random_field(n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 10)) @ (rng.standard_normal((10, p)) * np.linspace(1.5, 0.5, 10)[:, None])
    return (X + 1.5 * rng.standard_normal((n, p)) + 2.0).astype(np.float32)


def grid(X, nlat):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X.reshape(n, nlat, p // nlat), ("time", "lat", "lon"),
                        {"time": np.arange(n), "lat": LATS[nlat], "lon": np.arange(p // nlat) * 2.5})


CASES = {
    "plain_41x300": dict(n=41, p=300, nlat=6),
    "mask_coslat_weights_120x260": dict(n=120, p=260, nlat=4, use_coslat=True, weights=True, mask=True),
    "standardize_uncentred_64x252": dict(n=64, p=252, nlat=6, standardize=True, center=False),
    "dataset_33x330": dict(n=33, p=330, nlat=6, dataset=True),
    "list_200x132": dict(n=200, p=132, nlat=4, as_list=True),
}
_cache = {}


def flat(obj, lead):
    """components-like output (array, list of arrays, or dataset of arrays) -> [lead x P] in stacked feature order"""
    if isinstance(obj, (list, tuple)):
        return np.concatenate([np.asarray(o.values).reshape(lead, -1) for o in obj], axis=1)
    if hasattr(obj, "data_vars"):
        return np.concatenate([np.asarray(obj[v].values).reshape(lead, -1) for v in obj.data_vars], axis=1)
    return np.asarray(obj.values).reshape(lead, -1)


def rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def calibration(ctx, mat, Xt):
    """the largest relative error of the EOF model's two products on this resident field against float64"""
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


def make_input(name):
    import xeofs_amd as xe

    c = CASES[name]
    n, p, nlat = c["n"], c["p"], c["nlat"]
    X = random_field(n, p, seed=len(name) + n)
    if c.get("mask"):
        X[:, np.arange(p) % 5 == 1] = np.nan
    weights = None
    if c.get("dataset") or c.get("as_list"):
        pa = nlat * 12
        parts = [grid(X[:, :pa], nlat), xe.DataArray(X[:, pa:], ("time", "x"), {"time": np.arange(n), "x": np.arange(p - pa)})]
        inp = xe.Dataset({"a": parts[0], "b": parts[1]}) if c.get("dataset") else parts
    else:
        inp = grid(X, nlat)
        if c.get("weights"):
            wv = np.random.default_rng(3).random((nlat, p // nlat)) * 1.5 + 0.25
            weights = xe.DataArray(wv, ("lat", "lon"), {"lat": LATS[nlat], "lon": np.arange(p // nlat) * 2.5})
    return X, inp, weights


def fitted(ctx, name):
    """the fitted model of a case, its input, the preprocessed float32 field the fit saw (centred), the restatement fed the
    model's own pairs, and the derived tolerance: computed once and shared (nothing changes them)"""
    import xeofs_amd as xe
    from xeofs_amd import engine

    if name not in _cache:
        c = CASES[name]
        X, inp, weights = make_input(name)
        m = xe.single.Teleconnectivity(n_modes=K, standardize=bool(c.get("standardize")), use_coslat=bool(c.get("use_coslat")),
                                       center=c.get("center", True), max_corr=MAX_CORR)
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
        ref = tr.model(Xt, K, MAX_CORR, pairs=m.data["centre_index"])
        print(f"{name}: derived tolerance {tol:.3e}")
        _cache[name] = (m, inp, X, Xt, ref, tol)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ (i) the designed field
def test_designed_field_names_its_planted_pairs_in_order(ctx):
    import xeofs_amd as xe

    X = tr.designed_field()
    p = X.shape[1]
    m = xe.single.Teleconnectivity(n_modes=3)
    m.ctx = ctx
    m.fit(xe.DataArray(X.astype(np.float32), ("time", "x"), {"time": np.arange(X.shape[0]), "x": np.arange(p)}), dim="time")
    ci = m.data["centre_index"]
    assert ci.dtype == np.int64 and ci.shape == (3, 2)
    assert [frozenset(q) for q in ci.tolist()] == [frozenset(q) for q in tr.DESIGNED_PAIRS]
    mask = m.centre_mask()
    assert mask.dims == ("mode", "x")
    for k in range(3):
        want = np.zeros(p)
        want[ci[k, 0]], want[ci[k, 1]] = 1.0, -1.0
        assert np.array_equal(mask.values[k], want)
    # the neighbours of a pole correlate with it far above max_corr: never a later pole
    near = {pole + d for q in tr.DESIGNED_PAIRS for pole in q for d in range(1, tr.DESIGNED_NEIGHBOURS + 1)}
    assert not near & set(ci.reshape(-1).tolist())
    m6 = xe.single.Teleconnectivity(n_modes=6, max_corr=0.3)
    m6.ctx = ctx
    m6.fit(xe.DataArray(X.astype(np.float32), ("time", "x"), {"time": np.arange(X.shape[0]), "x": np.arange(p)}), dim="time")
    assert [frozenset(q) for q in m6.data["centre_index"][:3].tolist()] == [frozenset(q) for q in tr.DESIGNED_PAIRS]
    assert not near & set(m6.data["centre_index"].reshape(-1).tolist())
    # the partner of every pole is the other pole, and the map is the strength of the seesaw
    tele = m.teleconnectivity()
    assert tele.dims == ("x",) and tele.values.shape == (p,)
    for (b, a), al in zip(tr.DESIGNED_PAIRS, tr.DESIGNED_ALPHA):
        assert m.data["partner_index"][b] == a and m.data["partner_index"][a] == b
        assert abs(tele.values[b] - al) < 0.08 and tele.values[b] == pytest.approx(tele.values[a], abs=1e-6)


# ------------------------------------------------------------------------------------------------ (ii) random fields
@pytest.mark.parametrize("name", list(CASES))
def test_map_and_partners_against_float64(ctx, name):
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    n, p = Xt.shape
    vf = m.preprocessor.valid_feature
    tele = flat(m.teleconnectivity(), 1)[0]
    assert tele.shape == (vf.size,) and np.all(np.isnan(tele[~vf]))
    assert type(m.teleconnectivity()) is type(inp) or isinstance(inp, list)
    got = -tele[vf].astype(np.float64)
    B, Bj = tr.pair_bound(Xt)
    err = np.abs(got - ref["rmin"])
    print(f"{name}: largest map error / B_j = {np.max(err / Bj):.3f}")
    assert np.all(err <= Bj)
    partner = m.data["partner_index"]
    assert partner.dtype == np.int64 and partner.shape == (p,) and np.all(partner >= 0) and np.all(partner != np.arange(p))
    R = tr.correlation(Xt)
    assert np.all(R[np.arange(p), partner] <= ref["rmin"] + 2 * Bj)
    np.testing.assert_array_equal(m.data["teleconnectivity"], tele[vf])


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_are_the_float64_choice_up_to_the_kernel_bound(ctx, name):
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    B, Bj = tr.pair_bound(Xt)
    R = tr.correlation(Xt)
    ci = m.data["centre_index"]
    assert ci.shape == (K, 2) and len(set(ci.reshape(-1).tolist())) == 2 * K
    for k in range(K):
        b, a = int(ci[k, 0]), int(ci[k, 1])
        w = ref["choice"][k][0]
        slack = 2.0 * max(Bj[b], Bj[w])
        print(f"{name} mode {k}: pair ({b}, {a}), float64 choice {ref['choice'][k]}, gap {ref['rmin'][b] - ref['rmin'][w]:.3e}, "
              f"allowed {slack:.3e}")
        assert ref["open"][k][b] and ref["rmin"][b] < 0.0
        assert ref["rmin"][b] - ref["rmin"][w] <= slack
        assert R[b, a] <= ref["rmin"][b] + 2 * Bj[b]
        for q in range(k):                                             # separated from every earlier pole
            for x in (b, a):
                assert max(abs(R[x, ci[q, 0]]), abs(R[x, ci[q, 1]])) <= MAX_CORR + 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_against_the_restatement_fed_the_models_pairs(ctx, name):
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    n, p = Xt.shape
    vf = m.preprocessor.valid_feature
    assert sorted(m.data) == sorted(["input_data", "components", "scores", "teleconnectivity", "partner_index", "centre_index",
                                     "norms", "explained_variance", "total_variance"])
    assert set(m.stats) == {"ms_pairmin", "ms_series", "ms_tmul"}
    S = np.asarray(m.scores().values)
    assert S.shape == (K, n) and S.dtype == np.float32
    C = flat(m.components(), K)[:, vf]
    errs = dict(scores=rel(S.T, ref["scores"]), components=rel(C.T, ref["components"]))
    errs["singular_values"] = float(np.max(np.abs(np.asarray(m.singular_values().values) - ref["sv"]) / ref["sv"]))
    ev = m.data["explained_variance"]
    errs["explained_variance"] = float(np.max(np.abs(ev - ref["explained_variance"]) / ref["explained_variance"]))
    errs["total_variance"] = abs(m.data["total_variance"] - ref["total_variance"]) / ref["total_variance"]
    print(f"{name}: tolerance {tol:.3e}, relative errors {errs}")
    for key, e in errs.items():
        assert e <= tol, (key, e, tol)
    np.testing.assert_array_equal(np.asarray(m.explained_variance().values), ev)
    np.testing.assert_allclose(np.asarray(m.explained_variance_ratio().values), ev / m.data["total_variance"], rtol=1e-15)
    # the poles: +~1 and -~1, of equal size, and nothing above 1
    ci = m.data["centre_index"]
    for k in range(K):
        b, a = ci[k]
        want = np.sqrt((1.0 - ref["rmin"][b]) / 2.0)
        assert abs(C[k, b] - want) <= 2 * tol + 2 * tr.pair_bound(Xt)[1][b] and abs(C[k, a] + want) <= 2 * tol + 2 * tr.pair_bound(Xt)[1][b]
    assert np.abs(C).max() <= 1.0 + tol
    # the centres carry the input's own coordinates; masked features are NaN
    mask = flat(m.centre_mask(), K)
    assert np.all(np.isnan(mask[:, ~vf]))
    mv = mask[:, vf]
    assert np.array_equal(np.argmax(mv, axis=1), ci[:, 0]) and np.array_equal(np.argmin(mv, axis=1), ci[:, 1])
    assert np.array_equal(np.abs(mv).sum(axis=1), np.full(K, 2.0)) and np.array_equal(mv.sum(axis=1), np.zeros(K))
    assert type(m.centre_mask()) is type(m.components())
    with pytest.raises(NotImplementedError):
        m.inverse_transform(m.scores())


@pytest.mark.parametrize("name", [c for c in CASES if CASES[c].get("center", True)])        # (center=False: transform applies the
def test_transform_of_the_training_data_returns_the_scores(ctx, name):                      #  fitted, uncentred preprocessing)
    m, inp, X, Xt, ref, tol = fitted(ctx, name)
    got = m.transform(inp)
    S = m.scores()
    assert got.dims == S.dims and got.values.shape == S.values.shape
    assert rel(got.values, S.values) <= tol


# ------------------------------------------------------------------------------------------------ (iii) further properties
def test_n_modes_beyond_what_separation_allows_raises(ctx):
    import xeofs_amd as xe

    X = tr.designed_field().astype(np.float32)
    arr = xe.DataArray(X, ("time", "x"), {"time": np.arange(X.shape[0]), "x": np.arange(X.shape[1])})
    m = xe.single.Teleconnectivity(n_modes=30, max_corr=0.05)
    m.ctx = ctx
    with pytest.raises(ValueError, match="less than or equal to the number of separated seesaws.*exhausted after"):
        m.fit(arr, dim="time")


def test_uncentred_fit_equals_the_centred_fits_patterns(ctx):
    import xeofs_amd as xe

    X = random_field(50, 120, seed=6)
    arr = xe.DataArray(X, ("time", "x"), {"time": np.arange(50), "x": np.arange(120)})
    fits = []
    for center in (True, False):
        m = xe.single.Teleconnectivity(n_modes=2, center=center, max_corr=MAX_CORR)
        m.ctx = ctx
        m.fit(arr, dim="time")
        fits.append(m)
    a, b = fits
    np.testing.assert_array_equal(a.data["centre_index"], b.data["centre_index"])
    np.testing.assert_array_equal(a.data["partner_index"], b.data["partner_index"])
    # the centred twin is the same preprocessing of the same input: the same float32 field up to its last bits
    np.testing.assert_allclose(a.teleconnectivity().values, b.teleconnectivity().values, rtol=0, atol=1e-6)
    np.testing.assert_allclose(a.components().values, b.components().values, rtol=0, atol=1e-6)
    np.testing.assert_allclose(a.scores().values, b.scores().values, rtol=0, atol=1e-6 * np.abs(a.scores().values).max())


def test_constant_and_zero_weight_points_are_nan_and_never_poles(ctx):
    import xeofs_amd as xe

    n, p = 60, 96
    X = random_field(n, p, seed=9)
    const, zero_w = [7, 40], [13, 64]
    X[:, const] = 3.25
    arr = xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})
    wv = np.ones(p)
    wv[zero_w] = 0.0
    m = xe.single.Teleconnectivity(n_modes=2, max_corr=MAX_CORR)
    m.ctx = ctx
    m.fit(arr, dim="time", weights=xe.DataArray(wv, ("x",), {"x": np.arange(p)}))
    tele = m.teleconnectivity().values
    out = const + zero_w
    assert np.all(np.isnan(tele[out])) and np.all(np.isfinite(np.delete(tele, out)))
    vf = m.preprocessor.valid_feature
    where = np.flatnonzero(vf)                                         # valid-feature order -> the input's own order
    assert not set(where[m.data["centre_index"].reshape(-1)].tolist()) & set(out)
    partner = m.data["partner_index"]
    assert not set(where[partner[partner >= 0]].tolist()) & set(out)
    # and the rest of the map is that of the field without them
    keep = np.setdiff1d(np.arange(p), out)
    m2 = xe.single.Teleconnectivity(n_modes=2, max_corr=MAX_CORR)
    m2.ctx = ctx
    m2.fit(xe.DataArray(X[:, keep], ("time", "x"), {"time": np.arange(n), "x": np.arange(keep.size)}), dim="time")
    Xc = X[:, keep].astype(np.float64) - X[:, keep].astype(np.float64).mean(axis=0)
    Bj = tr.pair_bound(Xc)[1]
    assert np.all(np.abs(tele[keep] - m2.teleconnectivity().values) <= 2 * Bj + 1e-6)
