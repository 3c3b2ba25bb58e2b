"""GPU tests of xeofs_amd.single.ICA against the float64 restatement (tests/ica_reference.py).

(a) A planted field (n = 1024, P = 96): four sources of unit variance with known non-Gaussian laws (uniform, Laplace, bimodal, a
    sine) in 96 mixing patterns plus small noise.  The sources come back up to order and sign: min_j max_i |corr| of the fit is at
    least that of the float64 restatement fed the model's OWN whitened panel and starts, minus 1e-3, and the restatement reaches 0.99
    (tests/test_ica_reference_cpu.py checks the seed on the CPU with numpy's PCA).
(b) Against the restatement fed the model's own PCA, through every preprocessing route: the unmixing matrix within dW = max(16
    times the deviation of the restatement's float32 emulation from its float64 run, 1e-6) as tests/test_gpu_ica_step.py holds a
    whole run; sources, components and filter patterns within that dW carried through the product -- |A| D^-+1 dW 1 1^T -- plus
    the bound test_gpu_pcmul.py holds a float64 product of inner length q to, (q + 2) 2^-53 |A| |M| + 2^-24 |ref|.
(c) The identities, transform / inverse_transform, restarts, reruns and the warning."""

import warnings

import numpy as np
import pytest

import ica_reference as kr

pytestmark = pytest.mark.gpu

LATS = np.array([-60.0, -20.0, 10.0, 45.0])
U24, U53 = 2.0 ** -24, 2.0 ** -53
_cache = {}


def line(X, name="x"):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", name), {"time": np.arange(n), name: np.arange(p)})


def grid(X):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X.reshape(n, 4, p // 4), ("time", "lat", "lon"), {"time": np.arange(n), "lat": LATS, "lon": np.arange(p // 4) * 2.5})


def planted():
    if "field" not in _cache:
        _cache["field"] = kr.planted_field()
    return _cache["field"]


def fit(ctx, inp, weights=None, **kw):
    import xeofs_amd as xe

    m = xe.single.ICA(**kw)
    m.ctx = ctx
    m.fit(inp, dim="time", weights=weights)
    return m


def planted_model(ctx):
    """the fit of the planted field, computed once and shared (nothing changes it)"""
    if "model" not in _cache:
        _cache["model"] = fit(ctx, line(planted()[0]), n_modes=4, random_state=kr.PLANTED_START)
    return _cache["model"]


def restated(m):
    """the float64 restatement (and its float32 emulation) fed the model's own whitened panel, starts and PCA ->
    dict(fit, emu, W, dW, Vq, Wq, ev, order, components, filter_patterns, scores) in the model's order and sign"""
    if hasattr(m, "_restated"):
        return m._restated
    prm, d = m.get_params(), m.data
    Z, W0 = m.whitened(), d["starts"]
    assert Z.dtype == np.float32 and W0.dtype == np.float64
    args = (prm["fun"], prm["alpha"], prm["tol"], prm["max_iter"])
    ref, emu = kr.fit(Z, W0, *args), kr.fit(Z, W0, *args, f32=True)
    W = ref["runs"][ref["best"]]["W"]
    dW = max(16.0 * np.abs(emu["runs"][ref["best"]]["W"] - W).max(), 1e-6)
    n = Z.shape[0]
    Vq, Wq, ev, order = kr.carry_back(W, d["sigma"], n, d["pca_explained_variance"])
    V, S = m._pca_components.astype(np.float64), m._pca_scores.astype(np.float64)
    comp = V @ Wq
    sgn = np.where(np.abs(comp.max(axis=0)) >= np.abs(comp.min(axis=0)), 1.0, -1.0)
    dd = d["sigma"] / np.sqrt(n)
    q = W.shape[0]
    out = dict(fit=ref, emu=emu, W=W, dW=dW, Vq=Vq * sgn, Wq=Wq * sgn, ev=ev, order=order, sgn=sgn, components=comp * sgn,
               filter_patterns=(V @ Vq) * sgn, scores=(S @ Vq) * sgn,
               tol=dict(components=np.abs(V) @ (dd[:, None] * np.full((q, q), dW)) + (q + 2) * U53 * (np.abs(V) @ np.abs(Wq)),
                        filter_patterns=np.abs(V) @ (np.full((q, q), dW) / dd[:, None]) + (q + 2) * U53 * (np.abs(V) @ np.abs(Vq)),
                        scores=np.abs(S) @ (np.full((q, q), dW) / dd[:, None]) + (q + 2) * U53 * (np.abs(S) @ np.abs(Vq))))
    m._restated = out
    return out


def check_against_restatement(m, what):
    r = restated(m)
    best = r["fit"]["best"]
    run = r["fit"]["runs"][best]
    # an iteration count is asserted only of a run that stays clear of the threshold; one that does not is a failure naming the case
    tol = m.get_params()["tol"]
    for t, rn in enumerate(r["fit"]["runs"]):
        assert kr.well_conditioned(rn, tol), f"{what}: restart {t} of the restatement passes lim = {rn['lims']} near tol: choose another random_state"
        assert m.stats["iterations"][t] == rn["iters"] and m.stats["status"][t] == rn["status"], f"{what}: restart {t}"
    assert m.stats["best"] == best
    e = np.abs(m.data["unmixing"] - r["W"]).max()
    assert e <= r["dW"], f"{what}: the unmixing matrix is off by {e / r['dW']:.3g} of its bound"
    assert np.array_equal(m.data["mode_order"], r["order"])
    worst = {}
    for name in ("components", "filter_patterns", "scores"):
        got, ref = m.data[name].astype(np.float64), r[name]
        bound = r["tol"][name] + U24 * np.abs(ref)
        err = np.abs(got - ref)
        worst[name] = float((err / bound).max())
        assert (err <= bound).all(), f"{what}: {name} off by {worst[name]:.3g} of the bound"
    assert np.abs(m.data["explained_variance"] - r["ev"]).max() <= 2 * r["dW"] * m.data["pca_explained_variance"].sum()
    print(f"{what}: {run['iters']} iterations, W at {e / r['dW']:.3g} of dW = {r['dW']:.3g}; " +
          ", ".join(f"{k} at {v:.3g}" for k, v in worst.items()) + " of the bounds")
    return r


# ------------------------------------------------------------------------------------------------ (a) the planted field
def test_planted_sources_come_back(ctx):
    X, S = planted()
    m = planted_model(ctx)
    sc = m.scores()
    assert sc.dims == ("mode", "time") and sc.shape == (4, 1024)
    r = restated(m)
    got = kr.recovery(np.asarray(sc.values, np.float64).T, S)
    ref = kr.recovery(r["scores"], S)
    print(f"planted: recovery {got:.6f}, the restatement's {ref:.6f}; iterations {m.stats['iterations'].tolist()}, "
          f"ms = { {k: round(v, 2) for k, v in m.stats.items() if k.startswith('ms_')} }")
    assert ref >= 0.99 and got >= ref - 1e-3
    assert m.stats["converged"] and m.stats["calls"] == 2 and m.stats["status"].tolist() == [1]
    # every true source is matched by exactly one mode
    C = np.abs(np.corrcoef(np.asarray(sc.values, np.float64), S.T)[:4, 4:])
    assert sorted(C.argmax(axis=0).tolist()) == [0, 1, 2, 3]
    ng = m.negentropy()
    assert ng.dims == ("mode",) and (ng.values > 0).all()
    assert abs(m.restart_contrasts()[0] - ng.values.sum()) <= 1e-12
    with pytest.raises(NotImplementedError):
        m.singular_values()


def test_planted_against_the_restatement(ctx):
    m = planted_model(ctx)
    r = check_against_restatement(m, "planted")
    comp, filt = m.components(), m.filter_patterns()
    assert comp.dims == filt.dims == ("mode", "x") and comp.shape == (4, 96)
    assert np.array_equal(np.asarray(comp.values).T, m.data["components"])
    assert np.abs(m.mixing_matrix() - r["Wq"]).max() <= 2 * r["dW"] * np.abs(r["Wq"]).max() * 4
    # the sign rule: the largest |entry| of every component is positive
    C = m.data["components"]
    assert (np.abs(C.max(axis=0)) >= np.abs(C.min(axis=0))).all()


def test_identities(ctx):
    m = planted_model(ctx)
    Z = m.whitened().astype(np.float64)
    n = Z.shape[0]
    white = np.linalg.norm(Z.T @ Z / n - np.eye(4), 2)
    sc = m.data["scores"].astype(np.float64)
    assert np.abs((sc * sc).sum(axis=0) / n - 1.0).max() <= white + 4 * U24 + 4 * 2e-6      # (2e-6: twice the floor of dW)
    assert np.abs(sc.mean(axis=0)).max() <= 1e-5
    V, S = m._pca_components.astype(np.float64), m._pca_scores.astype(np.float64)
    rec = S @ V.T
    got = sc @ m.data["components"].astype(np.float64).T
    # W orthogonal to 64 q 2^-52 (test_gpu_ica_step.py), float32 factors: 2 2^-24 per term of a sum of q = 4
    tol = 16 * U24 * (np.abs(sc) @ np.abs(m.data["components"].astype(np.float64).T))
    assert (np.abs(got - rec) <= tol).all(), float((np.abs(got - rec) / tol).max())
    ev, evr = m.explained_variance(), m.explained_variance_ratio()
    lam = m.data["pca_explained_variance"]
    assert ev.dims == ("mode",) and (np.diff(ev.values) <= 0).all()
    assert abs(ev.values.sum() - lam.sum()) <= 64 * 4 * 2.0 ** -52 * lam.sum() * 4
    assert np.allclose(evr.values, ev.values / m.data["total_variance"], rtol=1e-12) and 0.9 < evr.values.sum() <= 1.0 + 1e-6
    Wd = m.data["unmixing"]
    assert np.linalg.norm(Wd @ Wd.T - np.eye(4)) <= 64 * 4 * 2.0 ** -52


def test_transform_and_inverse_transform(ctx):
    X, _ = planted()
    m = planted_model(ctx)
    T, S = m.transform(line(X)), m.scores()
    assert T.dims == S.dims and T.shape == S.shape
    # the same scores X V through the same projection kernel, the product with Vq rounded to float32 on both roads
    q = 4
    tol = (q + 2) * U24 * (np.abs(m._pca_scores.astype(np.float64)) @ np.abs(m._Vq)).T + 2 * U24 * np.abs(S.values)
    assert (np.abs(np.asarray(T.values, np.float64) - np.asarray(S.values, np.float64)) <= tol).all()
    rec = m.inverse_transform(S)
    assert rec.dims == ("time", "x") and rec.shape == (1024, 96)
    want = m._pca_scores.astype(np.float64) @ m._pca_components.astype(np.float64).T + X.astype(np.float64).mean(axis=0)
    scale = np.abs(X).max()
    assert np.abs(np.asarray(rec.values, np.float64) - want).max() <= 64 * U24 * scale
    one = m.inverse_transform(S.sel(mode=1))
    assert one.shape == (1024, 96)


# ------------------------------------------------------------------------------------------------ (b) the preprocessing routes
# random_state: chosen so that no lim of the three runs comes within [0.4 tol, 2.5 tol] -- on the device's own PCA, whose signs a
# CPU PCA does not share; check_against_restatement asserts the condition again on every run
ROUTES = {
    "standardize": dict(standardize=True, random_state=0),
    "coslat_weights": dict(use_coslat=True, weights=True, random_state=7),
    "land_mask": dict(mask=True, random_state=4),
    "two_fields": dict(fields=True, random_state=7),
}


@pytest.mark.parametrize("name", list(ROUTES))
@pytest.mark.parametrize("fun", ["logcosh", "exp", "cube"])
def test_every_preprocessing_route_against_the_restatement(ctx, name, fun):
    import xeofs_amd as xe

    c = ROUTES[name]
    X, S = kr.planted_field(kr.PLANTED_SEED + 1, n=512)
    X = (X * np.linspace(0.5, 3.0, 96) + np.linspace(-2.0, 5.0, 96)).astype(np.float32)
    if c.get("mask"):
        X[:, np.arange(96) % 7 == 3] = np.nan
    weights = None
    if c.get("weights"):
        weights = xe.DataArray(np.random.default_rng(3).random((4, 24)) * 1.5 + 0.25, ("lat", "lon"), {"lat": LATS, "lon": np.arange(24) * 2.5})
    inp = [grid(X[:, :64].copy()), line(X[:, 64:].copy())] if c.get("fields") else grid(X)
    m = fit(ctx, inp, weights, n_modes=4, fun=fun, random_state=c["random_state"], standardize=bool(c.get("standardize")), use_coslat=bool(c.get("use_coslat")))
    check_against_restatement(m, f"{name} {fun}")
    comp, sc = m.components(), m.scores()
    if c.get("fields"):
        assert [x.dims for x in comp] == [("mode", "lat", "lon"), ("mode", "x")] and comp[0].shape == (4, 4, 16) and comp[1].shape == (4, 32)
    else:
        assert comp.dims == ("mode", "lat", "lon") and comp.shape == (4, 4, 24)
        valid = ~np.isnan(X).any(axis=0)
        C = np.asarray(comp.values).reshape(4, -1)
        assert np.isnan(C[:, ~valid]).all() and np.isfinite(C[:, valid]).all()
    assert sc.dims == ("mode", "time") and sc.shape == (4, 512)
    print(f"{name} {fun}: recovery of the planted sources {kr.recovery(np.asarray(sc.values, np.float64).T, S):.4f}")


# ------------------------------------------------------------------------------------------------ (c) restarts, reruns, the warning
def test_five_restarts_pick_the_restatements(ctx):
    """two iterations from five starts: the restarts stand at different places, the best contrast leads by more than 1e-3 of itself
    (asserted on the restatement; the device's contrasts are held to 1e-5 of it) and belongs to restart 2"""
    X, S = planted()
    with pytest.warns(UserWarning, match="did not converge"):
        m = fit(ctx, line(X), n_modes=4, n_init=5, fun="exp", random_state=5, max_iter=2)
    r = check_against_restatement_unconverged(m, "five restarts")
    assert m.data["starts"].shape == (5, 4, 4) and m.restart_contrasts().shape == (5,)
    assert np.abs(m.data["starts"] - kr.starts(4, 5, 5)).max() <= 1e-9
    cons = r["fit"]["contrasts"]
    c = np.sort(cons)[::-1]
    assert (c[0] - c[1]) / c[0] >= 1e-3
    assert int(np.argmax(m.restart_contrasts())) == r["fit"]["best"] == m.stats["best"] == 2
    assert np.abs(m.restart_contrasts() - cons).max() <= 1e-5 * np.abs(cons).max()
    assert m.stats["iterations"].tolist() == [2] * 5 and m.stats["status"].tolist() == [0] * 5 and not m.stats["converged"]
    # w_init replaces the draw: given the draw of random_state = PLANTED_START itself, the fit is the planted fit bit for bit
    a = planted_model(ctx)
    W0 = np.random.RandomState(kr.PLANTED_START).normal(size=(4, 4))
    w = fit(ctx, line(X), n_modes=4, w_init=W0, random_state=kr.PLANTED_START)
    for key in ("starts", "unmixing", "components", "scores"):
        assert np.array_equal(a.data[key], w.data[key]), key
    w2 = fit(ctx, line(X), n_modes=4, w_init=-W0[::-1], random_state=kr.PLANTED_START)
    assert np.abs(w2.data["starts"][0] - kr.polar(-W0[::-1])).max() <= 32 * 2.0 ** -52 * np.linalg.cond(W0) ** 2
    assert not np.array_equal(a.data["starts"], w2.data["starts"])


def check_against_restatement_unconverged(m, what):
    """a fit stopped by max_iter: every restart's W within dW of the restatement's after the same iterations"""
    r = restated(m)
    tol = m.get_params()["tol"]
    for t, rn in enumerate(r["fit"]["runs"]):
        assert kr.well_conditioned(rn, tol), f"{what}: restart {t} passes lim = {rn['lims']} near tol"
        dW = max(16.0 * np.abs(r["emu"]["runs"][t]["W"] - rn["W"]).max(), 1e-6)
        assert np.abs(m.data["restart_unmixing"][t] - rn["W"]).max() <= dW, f"{what}: restart {t}"
    return r


def test_two_fits_bit_for_bit(ctx):
    X, _ = planted()
    a = planted_model(ctx)
    b = fit(ctx, line(X), n_modes=4, random_state=kr.PLANTED_START)
    for key in ("components", "filter_patterns", "scores", "unmixing", "restart_unmixing", "explained_variance", "negentropy", "restart_contrasts",
                "starts", "mixing_matrix"):
        assert np.array_equal(a.data[key], b.data[key]), key
    assert np.array_equal(a.whitened(), b.whitened()) and "whitened" not in a.data
    assert np.array_equal(a.stats["iterations"], b.stats["iterations"]) and np.array_equal(a.stats["lim"], b.stats["lim"])


def test_a_fit_in_short_calls_equals_the_fit_in_one(ctx, monkeypatch):
    from xeofs_amd.single import ica

    X, _ = planted()
    a = planted_model(ctx)
    monkeypatch.setattr(ica, "CALL_ITERS", 2)
    b = fit(ctx, line(X), n_modes=4, random_state=kr.PLANTED_START)
    assert b.stats["calls"] == -(-int(a.stats["iterations"][0]) // 2) + 1 and a.stats["iterations"][0] > 2
    for key in ("components", "scores", "unmixing", "negentropy"):
        assert np.array_equal(a.data[key], b.data[key]), key
    assert np.array_equal(a.stats["iterations"], b.stats["iterations"])


def test_the_unconverged_warning_and_refusals_at_fit(ctx):
    import xeofs_amd as xe

    X, _ = planted()
    with pytest.warns(UserWarning, match="did not converge"):
        m = fit(ctx, line(X), n_modes=4, random_state=kr.PLANTED_START, max_iter=1)
    assert not m.stats["converged"] and m.stats["iterations"].tolist() == [1] and m.stats["status"].tolist() == [0]
    ref = kr.run(m.whitened(), m.data["starts"][0], "logcosh", 1.0, 1e-4, 1)
    assert np.abs(m.data["unmixing"] - ref["W"]).max() <= 1e-6
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fit(ctx, line(X), n_modes=4, random_state=kr.PLANTED_START)                  # (the converged fit warns of nothing)
    m = xe.single.ICA(n_modes=2)
    m.ctx = ctx
    with pytest.raises(TypeError, match="complex"):
        m.fit(line(X.astype(np.complex64)), dim="time")
    # rank-deficient scores: two modes asked of a field of rank one
    rs = np.random.RandomState(0)
    X1 = (rs.standard_normal((200, 1)) @ rs.standard_normal((1, 30))).astype(np.float32)
    m = xe.single.ICA(n_modes=2)
    m.ctx = ctx
    with pytest.raises(np.linalg.LinAlgError):
        m.fit(line(X1), dim="time")
