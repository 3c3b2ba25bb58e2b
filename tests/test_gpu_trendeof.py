"""GPU tests of trend EOF analysis (xeofs_amd.single.TrendEOF, engine.rank_matrix).

The checker is the float64 restatement of tests/trend_reference.py, which shares no code with the model.

  * The rank matrix is an integer matrix times a weight, rounded once: it is taken back from the engine and compared
    EXACTLY with the restatement of the downloaded preprocessed field.
  * total_variance is a closed form: float64 rounding.
  * Singular values and explained variance against the exact float64 SVD of that Z, with the tolerance
    tests/test_gpu_parity.py applies to the same quantities of EOF (|s - s_ref| <= 1e-5 s_ref[0]; it is the same solver on a
    float32 matrix), copied as SV_TOL.  For s^2 / (n - 1) the same bound gives |s^2 - s_ref^2| <= SV_TOL s_ref[0] (s + s_ref).
    The inverse ranks of anything but a monotone series are scrambled, so past the trend mode the spectrum of Z is a noise
    bulk (here s_4 / s_3 = 0.89): no fixed number of power iterations resolves modes 2 .. k of it to 1e-5, as for EOF on any
    such matrix.  The models of these comparisons therefore take solver="full", the decomposer's exact branch; the default
    (randomized) branch is checked on the separated trend mode.
  * scores(), components() and transform(training data) against the restatement FED THE MODEL'S OWN V, as test_gpu_lfca.py
    feeds the model's own PCA.  The bound is computed, not chosen: the error of a float32 numpy evaluation of the same two
    products (X V, then X^T Sh / (n - 1)) against float64, times 8 for the engine's different summation order.
  * An exactly monotone rank-one field X[t, j] = a_j g(t) is checked by construction, with cos-latitude and user weights.
"""

import numpy as np
import pytest

import trend_reference as tr

pytestmark = pytest.mark.gpu

SV_TOL = 1e-5            # tests/test_gpu_parity.py: np.abs(s - so).max() <= 1e-5 * so[0]
COS_TOL = 1e-5           # tests/test_gpu_parity.py: |cos| >= 1 - 1e-5 for a gap-separated vector
MARGIN = 8.0             # on the float32 numpy evaluation's own error: another summation order
K = 3


def trend_field(n, P, seed=0, noise=0.25):
    """a monotone non-linear trend, two oscillations and white noise, random loadings"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / (n - 1.0)
    G = np.stack([np.exp(2.5 * t), np.sin(2 * np.pi * 3.1 * t), np.cos(2 * np.pi * 7.3 * t) * (1 + t)], axis=1)
    G = (G - G.mean(0)) / G.std(0)
    L = rng.standard_normal((3, P)) * np.array([2.0, 1.3, 0.8])[:, None]
    return (G @ L + noise * rng.standard_normal((n, P)) + 3.0).astype(np.float32)


def da(X):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})


def preprocessed(ctx, model, X2d):
    """the float32 matrix the fit saw: the engine's preprocessing of the stacked field with the model's settings (centred:
    the centred twin stands in for an uncentred model), compacted; and the weights of its columns"""
    from xeofs_amd import engine

    prm, pre = model.get_params(), model.preprocessor
    mat, st = engine.preprocess(ctx, X2d, True, prm["standardize"], pre.feature_weights, in_place=True)
    try:
        Xt = mat.download()
    finally:
        mat.free()
    vf = st["valid_feature"]
    assert np.array_equal(vf, pre.valid_feature)
    w = np.ones(int(vf.sum())) if pre.feature_weights is None else np.asarray(pre.feature_weights)[vf]
    return Xt, w


CASES = {
    "plain": dict(n=200, P=300),                                   # m = 256: 32 threads per series, 8 series per workgroup
    "past_tier_edge": dict(n=257, P=150),                          # m = 512: one past the edge of the 256 tier
    "land_mask": dict(n=200, P=300, mask=True),                    # a third of the features all-NaN
    "weights_standardized": dict(n=200, P=120, weights=True, standardize=True),
    "uncentred": dict(n=130, P=90, center=False),
}
_cache = {}


def fitted(ctx, name):
    """the fitted model of a case, its raw field, its preprocessed field, its weights and its restatement: computed once and
    shared (nothing changes them)"""
    import xeofs_amd as xe

    if name not in _cache:
        c = CASES[name]
        X = trend_field(c["n"], c["P"], seed=len(name))
        if c.get("mask"):
            X[:, np.arange(c["P"]) % 3 == 1] = np.nan
        weights = None
        if c.get("weights"):
            wv = np.random.default_rng(3).random(c["P"]) * 1.5 + 0.25
            wv[5] = 0.0                                            # a feature of weight zero: a zero column of Z
            weights = xe.DataArray(wv, ("x",), {"x": np.arange(c["P"])})
        m = xe.single.TrendEOF(n_modes=K, solver="full", standardize=bool(c.get("standardize")), center=c.get("center", True))
        m.ctx = ctx
        m.fit(da(X), dim="time", weights=weights)
        Xt, w = preprocessed(ctx, m, X)
        ref = tr.restate(Xt, m.data["trend_eofs"], w)
        _cache[name] = (m, X, Xt, w, ref)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ 1. the rank matrix
@pytest.mark.parametrize("n,P,in_place,weighted,mask", [(200, 300, True, False, False), (257, 150, False, True, False),
                                                        (200, 300, True, True, True), (65, 70, True, False, False)])
def test_rank_matrix_is_exact(ctx, n, P, in_place, weighted, mask):
    from xeofs_amd import engine

    X = trend_field(n, P, seed=n + P)
    X[::7, 3] = X[0, 3]                                            # ties
    if mask:
        X[:, np.arange(P) % 3 == 0] = np.nan
    wfull = np.random.default_rng(1).random(P) + 0.5 if weighted else None
    mat, st = engine.preprocess(ctx, X, True, False, wfull, in_place=in_place)
    vf = st["valid_feature"]
    assert mat.p == int(vf.sum()) and not mat.masked
    w = None if wfull is None else wfull[vf]
    had = mat.has_sample_layout()
    zmat = engine.rank_matrix(ctx, mat, w)
    try:
        assert zmat.shape == mat.shape and (zmat.n_pad, zmat.p_pad) == (mat.n_pad, mat.p_pad)
        assert mat.has_sample_layout()                             # built on demand, kept for the caller to release
        if not had:
            mat.release_sample_layout()
            assert not mat.has_sample_layout()
        Xt = mat.download()
        Qref = tr.order_positions(np.ascontiguousarray(Xt.T))
        Zref = tr.rank_values(Qref, w).T
        Z = zmat.download()
        assert Z.dtype == np.float32 and Z.shape == (n, mat.p)
        bad = np.argwhere(Z.view(np.uint32) != np.ascontiguousarray(Zref).view(np.uint32))
        assert bad.size == 0, f"{len(bad)} entries differ, first {bad[0]}"
        # the padding of the new matrix is zero: its sum of squares is that of the n x p block (float32 entries, float64 sum)
        want = float(np.sum(Zref.astype(np.float64) ** 2))
        assert abs(zmat.sumsq() - want) <= 1e-12 * want
        # ... and that is the closed form, up to the one rounding of every entry (2^-24 relative, squared: 2^-23)
        tv = tr.total_variance(n, np.ones(mat.p) if w is None else w)
        assert abs(want / (n - 1) - tv) <= 2.0 ** -22 * tv
    finally:
        zmat.free()
        mat.free()
    with pytest.raises(ValueError, match="one entry per series"):
        m2 = engine.from_dense(ctx, np.zeros((4, 3), np.float32))
        try:
            engine.rank_matrix(ctx, m2, np.ones(4))
        finally:
            m2.free()


def test_rank_matrix_refuses_a_masked_in_place_matrix(ctx):
    from xeofs_amd import engine

    import ctypes as C

    from xeofs_amd import _lib

    X = trend_field(200, 700, seed=2)          # layout mode 3 keeps a mask in place when n < valid features >= 0.6 P, P % 4 == 0
    X[:, ::3] = np.nan
    mat, st = engine.preprocess(ctx, X, True, False, None, in_place=True, allow_masked=True)
    try:
        assert mat.masked, "the engine did not keep the land mask in place: the case needs another shape"
        with pytest.raises(ValueError, match="masked"):
            engine.rank_matrix(ctx, mat)
        h = C.c_void_p()
        assert ctx.lib.eofx_mat_orderpos_f32(ctx.handle, mat.handle, None, C.byref(h)) == _lib.ERR_ARG and not h.value
        assert b"masked" in ctx.lib.eofx_last_error(ctx.handle)
    finally:
        mat.free()


# ------------------------------------------------------------------------------------------------ 2. the model
@pytest.mark.parametrize("name", list(CASES))
def test_spectrum_against_the_exact_svd(ctx, name):
    m, X, Xt, w, ref = fitted(ctx, name)
    n = Xt.shape[0]
    assert sorted(m.data) == sorted(["input_data", "components", "scores", "trend_eofs", "norms", "explained_variance",
                                     "total_variance"])
    assert set(m.stats) == {"route", "ms_rank", "ms_svd", "ms_project"} and m.stats["route"] == "exact"
    tv = m.data["total_variance"]
    assert isinstance(tv, float) and abs(tv - ref["total_variance"]) <= 4 * np.finfo(np.float64).eps * ref["total_variance"]
    assert abs(tv - n * (n + 1) / 12.0 * float(np.sum(w * w))) <= 4 * np.finfo(np.float64).eps * tv
    so = ref["s"][:K]
    s = m.data["norms"]
    assert s.dtype == np.float64 and s.shape == (K,)
    print(f"{name}: s = {s}, exact = {so}, relative to s_1: {np.abs(s - so) / so[0]}")
    assert np.all(np.abs(s - so) <= SV_TOL * so[0]), (s, so)
    ev, evo = m.data["explained_variance"], so ** 2 / (n - 1)
    assert np.all(np.abs(ev - evo) <= SV_TOL * so[0] * (s + so) / (n - 1)), (ev, evo)
    np.testing.assert_array_equal(np.asarray(m.singular_values().values), s)
    np.testing.assert_array_equal(np.asarray(m.explained_variance().values), ev)
    np.testing.assert_allclose(np.asarray(m.explained_variance_ratio().values), ev / tv, rtol=1e-15)
    V = m.data["trend_eofs"]
    assert V.dtype == np.float32 and V.shape == (Xt.shape[1], K)
    np.testing.assert_allclose(V.astype(np.float64).T @ V.astype(np.float64), np.eye(K), atol=1e-5)


def float32_chain(Xt, V):
    """the two products of the model evaluated by numpy in float32: S = X V, then X^T Sh / (n - 1)"""
    n = Xt.shape[0]
    S32 = Xt @ V
    Sh32 = ((S32 - S32.mean(axis=0, dtype=np.float32)) / S32.std(axis=0, ddof=1, dtype=np.float32)).astype(np.float32)
    C32 = (Xt.T @ Sh32) / np.float32(n - 1)
    return S32, C32


@pytest.mark.parametrize("name", list(CASES))
def test_scores_components_and_transform_against_the_restatement(ctx, name):
    m, X, Xt, w, ref = fitted(ctx, name)
    n, p = Xt.shape
    S32, C32 = float32_chain(Xt, m.data["trend_eofs"])
    err_s = np.abs(S32.astype(np.float64) - ref["scores"]).max()
    err_c = np.abs(C32.astype(np.float64) - ref["components"]).max()
    got_s, got_c = m.data["scores"], m.data["components"]
    assert got_s.dtype == np.float32 and got_s.shape == (n, K) and got_c.dtype == np.float32 and got_c.shape == (p, K)
    ds = np.abs(got_s.astype(np.float64) - ref["scores"]).max()
    dc = np.abs(got_c.astype(np.float64) - ref["components"]).max()
    print(f"{name}: scores err {ds:.3e} (float32 numpy {err_s:.3e}), components err {dc:.3e} (float32 numpy {err_c:.3e})")
    assert ds <= MARGIN * err_s, f"scores: {ds:.3e} > {MARGIN} x {err_s:.3e}"
    assert dc <= MARGIN * err_c, f"components: {dc:.3e} > {MARGIN} x {err_c:.3e}"
    if CASES[name].get("center", True):                            # (an uncentred model's transform keeps the mean: module docstring)
        tt = np.asarray(m.transform(da(X)).values).T
        dt = np.abs(tt.astype(np.float64) - ref["scores"]).max()
        assert tt.shape == (n, K) and dt <= MARGIN * err_s, f"transform: {dt:.3e} > {MARGIN} x {err_s:.3e}"
        tn = np.asarray(m.transform(da(X), normalized=True).values).T
        np.testing.assert_allclose(tn, tt / m.data["norms"].astype(np.float32), rtol=1e-6)
    # labelled output: the patterns carry NaN at the dropped features and nowhere else
    comps = np.asarray(m.components().values)
    eofs = np.asarray(m.trend_eofs().values)
    vf = m.preprocessor.valid_feature
    assert comps.shape == (K, X.shape[1]) and eofs.shape == comps.shape
    assert np.array_equal(np.isnan(comps), np.broadcast_to(~vf, comps.shape)) and np.array_equal(np.isnan(eofs), np.isnan(comps))
    assert np.array_equal(comps[:, vf].T, got_c) and np.array_equal(eofs[:, vf].T, m.data["trend_eofs"])
    if CASES[name].get("mask"):
        assert int((~vf).sum()) == X.shape[1] // 3


def test_default_solver_resolves_the_trend_mode(ctx):
    """the randomized branch (the default at this shape): the trend mode is separated (s_2 / s_1 = 0.23), the bulk is not"""
    import xeofs_amd as xe

    m_full, X, Xt, w, ref = fitted(ctx, "plain")
    m = xe.single.TrendEOF(n_modes=K, random_state=5)
    m.ctx = ctx
    m.fit(da(X), dim="time")
    assert m.stats["route"] == "randomized"
    so = ref["s"]
    assert so[1] / so[0] < 0.3
    assert abs(m.data["norms"][0] - so[0]) <= SV_TOL * so[0]
    c = abs(float(np.dot(m.data["trend_eofs"][:, 0].astype(np.float64), m_full.data["trend_eofs"][:, 0].astype(np.float64))))
    assert c >= 1 - COS_TOL, c


def test_labels_match_eof(ctx):
    import xeofs_amd as xe

    n, nlat, nlon = 60, 6, 8
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, nlat, nlon)).astype(np.float32) + np.arange(n, dtype=np.float32)[:, None, None] * 0.05
    X[:, 2, 3] = np.nan
    coords = {"time": np.arange(n) * 10, "lat": np.linspace(-50, 50, nlat), "lon": np.arange(nlon) * 5.0}
    A = xe.DataArray(X, ("time", "lat", "lon"), coords)
    e = xe.single.EOF(n_modes=2, use_coslat=True, random_state=1)
    t = xe.single.TrendEOF(n_modes=2, use_coslat=True, random_state=1)
    e.ctx = t.ctx = ctx
    e.fit(A, dim="time")
    t.fit(A, dim="time")
    for a, b in [(t.components(), e.components()), (t.trend_eofs(), e.components()), (t.scores(), e.scores()),
                 (t.transform(A), e.transform(A)), (t.explained_variance(), e.explained_variance()),
                 (t.explained_variance_ratio(), e.explained_variance_ratio()), (t.singular_values(), e.singular_values())]:
        assert tuple(a.dims) == tuple(b.dims) and a.shape == b.shape
        assert set(a.coords) == set(b.coords)
        for d in a.coords:
            np.testing.assert_array_equal(np.asarray(a.coords[d]), np.asarray(b.coords[d]))
    assert np.isnan(np.asarray(t.components().values)[:, 2, 3]).all()
    assert t.components().name == "components" and t.trend_eofs().name == "trend_eofs" and t.scores().name == "scores"


# ------------------------------------------------------------------------------------------------ 3. by construction
def test_monotone_rank_one_field_by_construction(ctx):
    """X[t, j] = a_j g(t), g strictly increasing and non-linear, a_j of both signs and nonzero; cos-latitude weights times
    user weights.  Every column of Q is the identity or its reverse, so Z = (r - (n - 1) / 2) (sign(a_j) w_j)^T has rank one."""
    import xeofs_amd as xe
    from xeofs_amd import engine

    n, nlat, nlon = 180, 7, 9
    g = np.exp(3.0 * np.arange(n) / n)                             # increments of 1.7 %: no ties in float32, centred or not
    rng = np.random.default_rng(4)
    a = (rng.random((nlat, nlon)) + 0.2) * np.where(rng.random((nlat, nlon)) < 0.5, -1.0, 1.0)
    assert (a > 0).any() and (a < 0).any()
    X = (g[:, None, None] * a).astype(np.float32)
    lat = np.linspace(-75, 75, nlat)
    user = np.linspace(0.5, 2.0, nlon)
    A = xe.DataArray(X, ("time", "lat", "lon"), {"time": np.arange(n), "lat": lat, "lon": np.arange(nlon)})
    W = xe.DataArray(user, ("lon",), {"lon": np.arange(nlon)})
    m = xe.single.TrendEOF(n_modes=1, use_coslat=True)
    m.ctx = ctx
    m.fit(A, dim="time", weights=W)
    w = (np.sqrt(np.cos(np.deg2rad(lat)))[:, None] * user[None, :]).reshape(-1)
    np.testing.assert_allclose(m.preprocessor.feature_weights, w, rtol=1e-14)
    sa = np.sign(a).reshape(-1)
    # the engine's rank matrix of the engine's preprocessed field
    X2 = X.reshape(n, -1)
    mat, _ = engine.preprocess(ctx, X2, True, False, w, in_place=True)
    zmat = engine.rank_matrix(ctx, mat, w)
    try:
        Z = zmat.download().astype(np.float64)
    finally:
        zmat.free()
        mat.free()
    r = np.arange(n) - (n - 1) / 2.0
    for j in range(Z.shape[1]):
        assert np.array_equal(Z[:, j], np.float32(sa[j] * r * w[j]).astype(np.float64)), j      # identity or its reverse
    sv = np.linalg.svd(Z, compute_uv=False)
    assert sv[1] <= 1e-6 * sv[0]                                   # rank one (float32 entries: 2^-24 each)
    tv = m.data["total_variance"]
    assert abs(tv - n * (n + 1) / 12.0 * np.sum(w * w)) <= 4 * np.finfo(np.float64).eps * tv
    # mode 1 explains everything: |s^2 - s_ref^2| <= SV_TOL s_ref (s + s_ref) with s_ref^2 / (n - 1) = total_variance
    ratio = float(np.asarray(m.explained_variance_ratio().values)[0])
    print(f"explained variance ratio of mode 1: {ratio!r}")
    assert abs(ratio - 1.0) <= SV_TOL * (1.0 + np.sqrt(ratio)) + 2.0 ** -22
    v = m.data["trend_eofs"][:, 0].astype(np.float64)
    target = sa * w / np.linalg.norm(w)
    c = float(np.dot(v, target))
    assert abs(c) >= 1 - COS_TOL, c
    assert np.all(np.sign(v * np.sign(c)) == sa)
    pc = m.data["scores"][:, 0].astype(np.float64) * np.sign(c)
    assert np.all(np.diff(pc) > 0)                                 # the leading trend PC is a monotone function of t
    # the pattern of a rank-one field: the regression on the standardized PC is a_j w_j std(g) up to the sign
    pat = m.data["components"][:, 0].astype(np.float64) * np.sign(c)
    want = a.reshape(-1) * w * np.std(g, ddof=1)
    assert np.abs(pat - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(ctx):
    import xeofs_amd as xe

    X = trend_field(40, 12)
    wneg = np.ones(12)
    wneg[4] = -0.5
    m = xe.single.TrendEOF(n_modes=2)
    m.ctx = ctx
    with pytest.raises(ValueError, match="non-negative"):
        m.fit(da(X), dim="time", weights=xe.DataArray(wneg, ("x",), {"x": np.arange(12)}))
    with pytest.raises(ValueError, match="16384"):
        m.fit(da(np.random.default_rng(0).standard_normal((16385, 3)).astype(np.float32)), dim="time")
    with pytest.raises(TypeError, match="complex"):
        m.fit(da(X.astype(np.complex64)), dim="time")
    m.fit(da(X), dim="time")
    with pytest.raises(NotImplementedError, match="orthogonal expansion"):
        m.inverse_transform(m.scores())
    Xnan = X.copy()
    Xnan[3, 5] = np.nan
    e = xe.single.EOF(n_modes=2)
    e.ctx = ctx
    with pytest.raises(ValueError) as eof_err:
        e.fit(da(Xnan), dim="time")
    with pytest.raises(ValueError) as trend_err:                   # an isolated NaN: exactly as EOF
        m.fit(da(Xnan), dim="time")
    assert str(trend_err.value) == str(eof_err.value)
    with pytest.raises(np.linalg.LinAlgError, match="zero variance"):
        m.fit(da(np.full((30, 8), 2.0, np.float32)), dim="time")   # a constant field: every trend PC vanishes
