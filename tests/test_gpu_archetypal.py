"""GPU tests of xeofs_amd.single.ArchetypalAnalysis against the float64 restatement (tests/aa_reference.py).

(a) A planted field (n = 96, p = 130, k = 3; rows 5, 40 and 77 are the pure archetypes, the others Dirichlet(1) mixtures): from
    two poor starts the argmax of every row of B is a planted index, and max |A - W| lies within 4 times the figure the
    float64 restatement reaches on the same field from the same start (the float32 run of the rule lands within 1.2 times;
    4 leaves room for a different sequence of accepted steps).  From the default start FurthestSum names the three vertices
    and the fit ends with f / trK within 8 eps_K, eps_K the largest relative error of K's entries against the float64 Gram
    matrix of the same preprocessed field, measured here.
(b) Noisy mixtures through every preprocessing route: the rows of A and B lie on their simplices within the operator bounds
    (test_gpu_simplex.py), the history never increases, sum_{i > k} s_i^2 (1 - eps_K) <= f_final <= f_start.  A fit of five
    outer iterations is replayed by the restatement -- fed the model's K, its start and its recorded steps -- and agrees in A,
    B and Z within a tolerance measured on the same field: four times the largest relative error of engine.panel_tmul on the
    field and on K against float64, times the number of products the five iterations made.
(c) The rest of the surface: transform, inverse_transform, archetypes(), the order of the modes, reruns, refusals.
"""

import numpy as np
import pytest

import aa_reference as ar

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
VERTICES = (5, 40, 77)
LATS = np.array([-60.0, -20.0, 10.0, 45.0])
_cache = {}


def line(X, name="x"):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X, ("time", name), {"time": np.arange(n), name: np.arange(p)})


def grid(X):
    import xeofs_amd as xe

    n, p = X.shape
    return xe.DataArray(X.reshape(n, 4, p // 4), ("time", "lat", "lon"), {"time": np.arange(n), "lat": LATS, "lon": np.arange(p // 4) * 2.5})


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


def model_gram(m):
    """the K the fit saw (the Gram kernel is deterministic: the same bits), the preprocessed field, and eps_K"""
    mat = m.data["input_data"]
    n = mat.n
    K = mat.gram(0)[:n, :n].cpu().numpy().astype(np.float64)
    Xt = mat.download().astype(np.float64)
    K64 = Xt @ Xt.T
    return K, Xt, K64, float(np.abs(K - K64).max() / np.abs(K64).max())


def on_simplex(P):
    """rows >= 0 that sum to 1 within the bound of the projection: (|S| + 2) 2^-24"""
    P = np.asarray(P, dtype=np.float64)
    return bool(np.all(P >= 0.0) and np.all(np.abs(P.sum(axis=1) - 1.0) <= ((P > 0).sum(axis=1) + 2) * EPS))


# ------------------------------------------------------------------------------------------------ (a) the planted field
def planted():
    X, W = ar.planted_field(vertices=VERTICES)
    return X.astype(np.float32), W


@pytest.mark.parametrize("init", [[0, 1, 2], [10, 50, 90]])
def test_planted_field_is_recovered_from_a_poor_start(ctx, init):
    import xeofs_amd as xe

    X, W = planted()
    m = xe.single.ArchetypalAnalysis(n_modes=3, init=init)
    m.ctx = ctx
    m.fit(line(X), dim="time")
    A, B = m.data["scores"].astype(np.float64), m.data["weights"].astype(np.float64)
    picked = B.argmax(axis=1)
    assert sorted(picked.tolist()) == list(VERTICES)
    perm = [VERTICES.index(v) for v in picked]
    err = np.abs(A - W[:, perm]).max()
    K, Xt, K64, eps_k = model_gram(m)
    ref = ar.fit(K64, 3, init)
    rperm = [VERTICES.index(v) for v in ref["B"].argmax(axis=1)]
    err_ref = np.abs(ref["A"] - W[:, rperm]).max()
    print(f"planted, init={init}: device max|A - W| = {err:.4f} in {m.stats['iterations']} iterations, float64 restatement "
          f"{err_ref:.4f} in {len(ref['history'])}; ratio {err / err_ref:.2f}; f/trK = {m.data['objective'] / m.data['trK']:.2e}")
    assert err <= 4.0 * err_ref
    assert on_simplex(A) and on_simplex(B) and not m.stats["stalled"]


def test_planted_field_from_the_default_start(ctx):
    import xeofs_amd as xe

    X, W = planted()
    for seed in (0, 1):
        m = xe.single.ArchetypalAnalysis(n_modes=3, random_state=seed)
        m.ctx = ctx
        m.fit(line(X), dim="time")
        assert m.stats["start"] == np.random.RandomState(seed).randint(96)
        assert sorted(m.stats["init_index"].tolist()) == list(VERTICES)              # FurthestSum names the three vertices
        K, Xt, K64, eps_k = model_gram(m)
        assert m.stats["init_index"].tolist() == ar.furthest_sum(K, 3, m.stats["start"]).tolist()
        miss = m.data["objective"] / m.data["trK"]
        print(f"planted, default start (seed {seed}): f/trK = {miss:.3e}, eps_K = {eps_k:.3e}, ratio to 8 eps_K = {miss / (8 * eps_k):.3f}, "
              f"{m.stats['iterations']} iterations")
        assert abs(miss) <= 8.0 * eps_k
        assert abs(m.explained_variance_fraction() - (1.0 - miss)) <= 1e-15
        perm = [VERTICES.index(v) for v in m.data["weights"].argmax(axis=1)]
        assert np.abs(m.data["scores"] - W[:, perm]).max() <= 5e-3       # (|A - W| is of the order sqrt(f / trK))


# ------------------------------------------------------------------------------------------------ (b) noisy mixtures
CASES = {
    "mask_coslat_weights_300x500_k4": dict(n=300, p=500, k=4, grid=True, use_coslat=True, weights=True, mask=True),
    "standardize_257x129_k8": dict(n=257, p=129, k=8, standardize=True),
    "dataset_300x500_k4": dict(n=300, p=500, k=4, dataset=True),
    "list_257x129_k8": dict(n=257, p=129, k=8, as_list=True),
}


def make_input(name):
    import xeofs_amd as xe

    c = CASES[name]
    n, p = c["n"], c["p"]
    X = (ar.noisy_mixtures(n, p, c["k"], seed=len(name)) + 1.5).astype(np.float32)
    if c.get("mask"):
        X[:, np.arange(p) % 7 == 3] = np.nan
    weights = None
    if c.get("dataset") or c.get("as_list"):
        pa = 48 if p % 4 == 0 else 41
        parts = [grid(X[:, :pa]) if pa % 4 == 0 else line(X[:, :pa], "y"), line(X[:, pa:])]
        inp = xe.Dataset({"a": parts[0], "b": parts[1]}) if c.get("dataset") else parts
    elif c.get("grid"):
        inp = grid(X)
        if c.get("weights"):
            wv = np.random.default_rng(3).random((4, p // 4)) * 1.5 + 0.25
            weights = xe.DataArray(wv, ("lat", "lon"), {"lat": LATS, "lon": np.arange(p // 4) * 2.5})
    else:
        inp = line(X)
    return X, inp, weights


def fit_case(ctx, name, **kw):
    import xeofs_amd as xe

    c = CASES[name]
    X, inp, weights = make_input(name)
    m = xe.single.ArchetypalAnalysis(n_modes=c["k"], standardize=bool(c.get("standardize")), use_coslat=bool(c.get("use_coslat")),
                                     random_state=5, **kw)
    m.ctx = ctx
    m.fit(inp, dim="time", weights=weights)
    return m, X, inp


def fitted(ctx, name):
    """the converged fit of a case with K, the preprocessed field and eps_K: computed once and shared (nothing changes them)"""
    if name not in _cache:
        m, X, inp = fit_case(ctx, name)
        _cache[name] = (m, X, inp) + model_gram(m)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_noisy_mixtures_constraints_history_and_bounds(ctx, name):
    m, X, inp, K, Xt, K64, eps_k = fitted(ctx, name)
    k = CASES[name]["k"]
    n = Xt.shape[0]
    A, B = m.data["scores"], m.data["weights"]
    assert A.shape == (n, k) and B.shape == (k, n) and on_simplex(A) and on_simplex(B)
    h = m.objective_history()
    assert len(h) == m.stats["iterations"] >= 2 and np.all(np.diff(h) <= 0.0) and not m.stats["stalled"]
    s = np.linalg.svd(Xt, compute_uv=False)
    tail = float(np.sum(s[k:] ** 2))
    f = m.data["objective"]
    print(f"{name}: {len(h)} iterations, {m.stats['products']} products, f/trK = {f / m.data['trK']:.4f}, rank bound / trK = "
          f"{tail / m.data['trK']:.4f}, f_start/trK = {m.stats['f_start'] / m.data['trK']:.4f}, eps_K = {eps_k:.2e}, "
          f"ms = { {k_: round(v, 2) for k_, v in m.stats.items() if k_.startswith('ms_')} }")
    assert f == h[-1] and tail * (1.0 - eps_k) <= f <= m.stats["f_start"]
    assert abs(m.data["trK"] - np.trace(K)) <= 1e-12 * np.trace(K)
    # f as the model states it against |Xt - A B Xt|^2 computed directly in float64
    direct = ar.objective_direct(Xt, A.astype(np.float64), B.astype(np.float64))
    assert abs(direct - f) <= 8.0 * eps_k * m.data["trK"]
    assert np.all(np.diff(A.astype(np.float64).sum(axis=0)) <= 0.0)              # the order of the modes
    # Z = B Xt in the input's coordinates, NaN at the masked points
    Z = flat(m.components(), k)
    valid = m.preprocessor.valid_feature
    assert np.isnan(Z[:, ~valid]).all() and rel(Z[:, valid], B.astype(np.float64) @ Xt) <= 1e-5


def product_calibration(ctx, m, K, Xt, k):
    """the largest relative error of engine.panel_tmul (prec="f32") on the resident field and on K against float64"""
    from xeofs_amd import engine

    rng = np.random.default_rng(11)
    n = Xt.shape[0]
    mat = m.data["input_data"]
    W = rng.dirichlet(np.ones(n), k).T                                          # [n x k]: columns like the rows of B
    L = engine.panel_width(k)
    Zp = engine.panel_import(ctx, np.ascontiguousarray(W, dtype=np.float32), mat.n_pad, L)
    got = mat.compact_rows(engine.panel_export(ctx, engine.panel_tmul(ctx, mat, Zp, prec="f32"), mat.p_phys, k))
    e_field = rel(got, Xt.T @ W.astype(np.float32).astype(np.float64))
    Kmat = engine.from_dense(ctx, np.ascontiguousarray(K, dtype=np.float32))
    try:
        G = rng.standard_normal((n, k))
        Zp = engine.panel_import(ctx, np.ascontiguousarray(G, dtype=np.float32), Kmat.n_pad, L)
        got = engine.panel_export(ctx, engine.panel_tmul(ctx, Kmat, Zp, prec="f32"), n, k)
        e_k = rel(got, K.T @ G.astype(np.float32).astype(np.float64))
    finally:
        Kmat.free()
    return max(e_field, e_k)


@pytest.mark.parametrize("name", list(CASES))
def test_five_iterations_replayed_by_the_restatement(ctx, name):
    k = CASES[name]["k"]
    m, X, inp = fit_case(ctx, name, max_iter=5)
    K, Xt, K64, eps_k = model_gram(m)
    assert m.stats["iterations"] == 5 and len(m.stats["steps"]) == 5
    ref = ar.fit(K, k, m.stats["init_index"], replay=m.stats["steps"])
    products = m.stats["products"] + 1                                           # (and the one that makes Z)
    tol = 4.0 * product_calibration(ctx, m, K, Xt, k) * products
    A, B = m.data["scores"], m.data["weights"]
    assert np.array_equal(ref["order"], m.data["mode_order"])
    errs = dict(A=rel(A, ref["A"]), B=rel(B, ref["B"]), Z=rel(flat(m.components(), k)[:, m.preprocessor.valid_feature], ref["B"] @ Xt),
                f=abs(m.data["objective"] - ref["history"][-1]) / m.data["trK"])
    print(f"{name}: replay of 5 iterations, {products} products, tolerance {tol:.3e}, relative errors {errs}, "
          f"worst ratio {max(errs.values()) / tol:.3f}")
    for key, e in errs.items():
        assert e <= tol, (key, e, tol)


# ------------------------------------------------------------------------------------------------ (c) the rest of the surface
def surface_model(ctx):
    if "surface" not in _cache:
        import xeofs_amd as xe

        X = (ar.noisy_mixtures(120, 92, 3, seed=9, noise=0.2) + 2.0).astype(np.float32)
        m = xe.single.ArchetypalAnalysis(n_modes=3, random_state=1)
        m.ctx = ctx
        m.fit(grid(X), dim="time")
        _cache["surface"] = (m, X)
    return _cache["surface"]


def test_transform_of_the_training_field_returns_the_scores(ctx):
    """transform stops when a batch of inner_iter iterations moves no entry by more than sqrt(tol) = 1e-3, and the fit's own A
    is the result of inner_iter iterations per outer iteration on archetypes that were still moving by about as much: both lie
    within a few sqrt(tol) of the minimiser for the final archetypes.  Asserted: 5 sqrt(tol); the measured value is printed."""
    m, X = surface_model(ctx)
    T = m.transform(grid(X))
    S = m.scores()
    assert T.dims == S.dims and T.shape == S.shape
    d = float(np.abs(T.values - S.values).max())
    print(f"transform of the training field: max |transform - scores| = {d:.2e} after {m.stats['transform_batches']} batches")
    assert d <= 5.0 * np.sqrt(1e-6)
    assert on_simplex(T.values.T) and m.stats["transform_batches"] < 100
    # new samples: convex combinations of the archetypes come back as their own weights
    Z = flat(m.archetypes(), 3)
    Wn = np.random.default_rng(2).dirichlet(np.ones(3), 17)
    Tn = m.transform(grid((Wn @ Z).astype(np.float32)))
    assert np.abs(Tn.values.T - Wn).max() <= 0.05


def test_inverse_transform_of_the_scores_has_residual_f(ctx):
    m, X = surface_model(ctx)
    rec = m.inverse_transform(m.scores())
    assert rec.dims == ("time", "lat", "lon")
    res = float(np.sum((np.asarray(rec.values, dtype=np.float64).reshape(120, -1) - X.astype(np.float64)) ** 2))   # (centred only: same units)
    f, trK = m.data["objective"], m.data["trK"]
    print(f"inverse_transform: residual / trK = {res / trK:.6f}, f / trK = {f / trK:.6f}")
    assert abs(res - f) <= 1e-5 * trK


@pytest.mark.parametrize("name", ["mask_coslat_weights_300x500_k4", "standardize_257x129_k8", "dataset_300x500_k4"])
def test_archetypes_undo_the_preprocessing(ctx, name):
    """the rows of B sum to 1, so the archetypes in the field's own units are the same convex combinations of the raw samples"""
    m, X, inp, K, Xt, K64, eps_k = fitted(ctx, name)
    k = CASES[name]["k"]
    Za = flat(m.archetypes(), k)
    valid = m.preprocessor.valid_feature
    want = m.data["weights"].astype(np.float64) @ X[:, valid].astype(np.float64)
    assert np.isnan(Za[:, ~valid]).all()
    assert np.abs(Za[:, valid] - want).max() <= 2e-5 * np.abs(want).max()
    arch = m.archetypes()
    comp = m.components()
    first = (arch[0], comp[0]) if isinstance(arch, list) else (arch, comp)
    if not hasattr(arch, "data_vars"):
        assert first[0].dims == first[1].dims and first[0].dims[0] == "mode"
    W = m.archetype_weights()
    assert W.dims == ("mode", "time") and np.array_equal(W.values, m.data["weights"])
    assert np.array_equal(m.scores().values, m.data["scores"].T)


def test_two_fits_with_one_random_state_are_equal_bit_for_bit(ctx):
    a, X, inp = fit_case(ctx, "standardize_257x129_k8", max_iter=12)
    b, _, _ = fit_case(ctx, "standardize_257x129_k8", max_iter=12)
    for key in ("scores", "weights", "components", "history"):
        assert np.array_equal(a.data[key], b.data[key]), key
    assert [s["mu"] for s in a.stats["steps"]] == [s["mu"] for s in b.stats["steps"]]


def test_refusals_at_fit(ctx):
    import xeofs_amd as xe

    X = np.random.default_rng(0).standard_normal((6, 20)).astype(np.float32)
    for kw, exc, word in ((dict(n_modes=7), ValueError, "n_modes"), (dict(n_modes=2, init=[1, 6]), ValueError, "init")):
        m = xe.single.ArchetypalAnalysis(**kw)
        m.ctx = ctx
        with pytest.raises(exc, match=word):
            m.fit(line(X), dim="time")
    m = xe.single.ArchetypalAnalysis(n_modes=2)
    m.ctx = ctx
    with pytest.raises(TypeError, match="complex"):
        m.fit(line(X.astype(np.complex64)), dim="time")
    with pytest.raises(ValueError, match="variance"):
        m.fit(line(np.ones((6, 20), np.float32)), dim="time")
    # k = n: every sample is picked as an archetype
    m = xe.single.ArchetypalAnalysis(n_modes=6, max_iter=3)
    m.ctx = ctx
    m.fit(line(X), dim="time")
    assert sorted(m.stats["init_index"].tolist()) == list(range(6)) and m.data["objective"] <= m.stats["f_start"]
