"""GPU tests of xeofs_amd.single.KMeans against the float64 restatement (tests/kmeans_reference.py).

(a) A planted field (n = 600, P = 2048): four blobs of 240, 180, 120 and 60 samples, of unit standard deviation in a
    three-dimensional subspace and ten standard deviations apart, plus white noise.  From n_init = 8 the fit recovers the planted
    labels exactly and in population order, frequencies(), and classifiability() above 0.99.  The restatement, fed the model's
    own scores and seeds, follows EVERY restart: the same labels and the same iteration counts -- and asserts that its
    trajectory met no undecided row (a margin at most 2 (q + 3) 2^-24); one that did is a failure naming the seed.
    components() is V32 c^T within the bound test_gpu_pcmul.py holds engine.pcmul to: (q + 2) 2^-53 |V| |c^T| + 2^-24 |ref|.
(b) centroids() through every preprocessing route: the inverse preprocessing restated from the raw field with numpy, NaN at
    masked points, and the raw mean of every cluster's samples within 6 sigma / sqrt(count) + 1e-3 of the field's scale: a
    centroid is the projection of the cluster mean onto the kept PCs, which holds the planted subspace and takes the mean's
    white noise (sigma / sqrt(count) per feature) only down.
(c) The rest of the surface: transform, inverse_transform, init= and random_state, reruns, max_iter, refusals.
"""

import numpy as np
import pytest

import kmeans_reference as kr

pytestmark = pytest.mark.gpu

LATS = np.array([-60.0, -20.0, 10.0, 45.0])
U24, U53 = 2.0 ** -24, 2.0 ** -53
SEED = 1                                     # random_state of the planted fits (on the field of seed 0)
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
        X, lab = kr.planted_field()
        _cache["field"] = (X.astype(np.float32), lab)
    return _cache["field"]


def fit(ctx, inp, weights=None, **kw):
    import xeofs_amd as xe

    m = xe.single.KMeans(**kw)
    m.ctx = ctx
    m.fit(inp, dim="time", weights=weights)
    return m


def planted_model(ctx):
    """the fit of the planted field, computed once and shared (nothing changes it)"""
    if "model" not in _cache:
        X, lab = planted()
        _cache["model"] = fit(ctx, line(X), n_modes=4, n_init=8, random_state=SEED)
    return _cache["model"]


def fitted_labels(m):
    return np.asarray(m.labels().values).astype(np.int64) - 1


# ------------------------------------------------------------------------------------------------ (a) the planted field
def test_planted_labels_frequencies_and_classifiability(ctx):
    X, lab = planted()
    m = planted_model(ctx)
    L = m.labels()
    assert L.dims == ("time",) and L.shape == (600,)
    assert np.array_equal(fitted_labels(m), lab)                                  # exactly, and in population order
    f = m.frequencies()
    assert f.dims == ("mode",) and np.array_equal(f.values, np.array(kr.PLANTED_SIZES) / 600.0)
    c = m.classifiability()
    print(f"planted: classifiability {c:.6f}, iterations {m.stats['iterations'].tolist()}, launches {m.stats['launches']}, "
          f"inertias {np.round(m.restart_inertias(), 2).tolist()}, ms = { {k: round(v, 2) for k, v in m.stats.items() if k.startswith('ms_')} }")
    assert c > 0.99 and c == kr.classifiability(m.data["restart_centroids"])
    S = m.scores()
    assert S.dims == ("mode", "time") and np.array_equal(S.values.argmax(axis=0), lab) and np.array_equal(S.values.sum(axis=0), np.ones(600))
    assert m.stats["n_empty"] == 0 and m.stats["converged"].all() and m.stats["launches"] == 1 and m.stats["n_pca_modes"] == 14
    assert m.inertia() == m.restart_inertias()[m.stats["best"]] == m.restart_inertias().min()
    S32 = m.data["input_data"].astype(np.float64)
    assert m.explained_variance_fraction() == 1.0 - m.inertia() / float((S32 * S32).sum()) and 0.9 < m.explained_variance_fraction() < 1.0
    D = m.distances()
    assert D.dims == ("mode", "time") and np.array_equal(D.values.argmin(axis=0), lab)
    assert abs(float((D.values.min(axis=0) ** 2).sum()) - m.inertia()) <= 17 * U24 * m.inertia()
    for name in ("singular_values", "explained_variance", "explained_variance_ratio"):
        with pytest.raises(NotImplementedError):
            getattr(m, name)()


def test_the_restatement_follows_every_restart(ctx):
    m = planted_model(ctx)
    S32 = m.data["input_data"]
    seeds = m.stats["seeds"]
    assert S32.dtype == np.float32 and S32.shape == (600, 14) and seeds.shape == (8, 4)
    assert seeds.tolist() == kr.kmeanspp_seeds(S32, 4, 8, SEED).tolist()
    thr = kr.undecided_margin(14)
    for r in range(8):
        ref = kr.lloyd(S32, S32[seeds[r]], 300)
        assert ref["min_margin"] > thr, f"restart {r} of random_state {SEED} meets an undecided row: margin {ref['min_margin']:.3e}"
        assert ref["iters"] == m.stats["iterations"][r] and ref["converged"] == 1
        assert np.array_equal(ref["labels"], m.data["restart_labels"][r])
        assert abs(ref["inertia"] - m.restart_inertias()[r]) <= (17 * U24 + 600 * U53) * ref["inertia"]
    assert len(set(m.stats["iterations"].tolist())) > 1                           # the restarts did not all take the same road
    best = kr.lloyd(S32, S32[seeds[m.stats["best"]]], 300)
    order = np.argsort(-best["counts"], kind="stable")
    assert np.array_equal(order, m.data["mode_order"]) and np.array_equal(best["counts"][order], m.data["counts"])


def test_components_against_float64_within_the_bound_of_pcmul(ctx):
    m = planted_model(ctx)
    V, c = m._pca_components.astype(np.float64), m.data["centroids_pc"].astype(np.float64)      # [P x q], [k x q]
    ref = V @ c.T
    got = np.asarray(m.components().values, dtype=np.float64).T                   # (mode, x) -> [P x k]
    bound = (14 + 2) * U53 * (np.abs(V) @ np.abs(c.T)) + U24 * np.abs(ref)
    err = np.abs(got - ref)
    print(f"components: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert got.shape == (2048, 4) and np.all(err <= bound)
    # every centroid is the mean of its members' scores: the fit ended at a fixed point
    S32, lab = m.data["input_data"].astype(np.float64), m.data["labels"]
    for j in range(4):
        mean = S32[lab == j].mean(axis=0)
        assert np.all(np.abs(c[j] - mean) <= 600 * U53 * np.abs(S32[lab == j]).sum(axis=0) / (lab == j).sum() + U24 * np.abs(mean))


# ------------------------------------------------------------------------------------------------ (b) the preprocessing routes
ROUTES = {
    "plain_grid": dict(),
    "standardize": dict(standardize=True),
    "coslat_weights": dict(use_coslat=True, weights=True),
    "land_mask": dict(mask=True),
}
SIGMA = 0.05


def route_input(name):
    import xeofs_amd as xe

    c = ROUTES[name]
    X, lab = kr.planted_field(n=300, p=512, sizes=(120, 90, 60, 30), noise=SIGMA, seed=3)
    X = X * np.linspace(0.5, 3.0, 512) + np.linspace(-2.0, 5.0, 512)              # every feature its own scale and mean
    X = X.astype(np.float32)
    if c.get("mask"):
        X[:, np.arange(512) % 7 == 3] = np.nan
    weights = None
    if c.get("weights"):
        wv = np.random.default_rng(3).random((4, 128)) * 1.5 + 0.25
        weights = xe.DataArray(wv, ("lat", "lon"), {"lat": LATS, "lon": np.arange(128) * 2.5})
    return X, lab, grid(X), weights


@pytest.mark.parametrize("name", list(ROUTES))
def test_centroids_undo_the_preprocessing(ctx, name):
    c = ROUTES[name]
    X, lab, inp, weights = route_input(name)
    m = fit(ctx, inp, weights, n_modes=4, n_pca_modes=6, n_init=6, random_state=0, standardize=bool(c.get("standardize")),
            use_coslat=bool(c.get("use_coslat")), center=c.get("center", True))
    assert np.array_equal(fitted_labels(m), lab) and m.classifiability() > 0.99
    cen, comp = m.centroids(), m.components()
    assert cen.dims == comp.dims == ("mode", "lat", "lon") and cen.shape == (4, 4, 128)
    Z, Cp = np.asarray(cen.values, np.float64).reshape(4, -1), np.asarray(comp.values, np.float64).reshape(4, -1)
    valid = ~np.isnan(X).any(axis=0)
    assert np.isnan(Z[:, ~valid]).all() and np.isnan(Cp[:, ~valid]).all() and np.isfinite(Z[:, valid]).all()
    # the inverse preprocessing restated from the raw field: x = comp / w * std + mean
    X64 = X.astype(np.float64)
    w = np.ones(512)
    if c.get("use_coslat"):
        w = w * np.repeat(np.sqrt(np.cos(np.deg2rad(LATS))), 128)
    if weights is not None:
        w = w * np.asarray(weights.values, np.float64).reshape(-1)
    std = X64.std(axis=0) if c.get("standardize") else np.ones(512)
    mean = X64.mean(axis=0) if c.get("center", True) else np.zeros(512)
    want = Cp[:, valid] / w[valid] * std[valid] + mean[valid]
    scale = np.abs(X64[:, valid]).max()
    assert np.abs(Z[:, valid] - want).max() <= 4 * U24 * scale * max(1.0, float(np.max(std[valid])))
    # the raw mean of every cluster's samples
    worst = 0.0
    for j in range(4):
        mem = lab == j
        raw = X64[mem][:, valid].mean(axis=0)
        tol = 6.0 * SIGMA * 3.0 / np.sqrt(mem.sum()) + 1e-3 * scale                # (3: the largest feature scale of the field)
        worst = max(worst, float(np.abs(Z[j, valid] - raw).max() / tol))
        assert np.abs(Z[j, valid] - raw).max() <= tol
    print(f"{name}: centroids against the raw cluster means, worst ratio to the tolerance {worst:.3f}")


# ------------------------------------------------------------------------------------------------ (c) the rest of the surface
def test_transform_of_the_training_field_returns_the_labels(ctx):
    X, lab = planted()
    m = planted_model(ctx)
    T = m.transform(line(X))
    S = m.scores()
    assert T.dims == S.dims and T.shape == S.shape and np.array_equal(T.values, S.values)
    # new samples: a centroid in the field's units belongs to its own mode
    cen = np.asarray(m.centroids().values, np.float32)
    Tn = m.transform(line(cen[[2, 0, 3, 1, 2]]))
    assert np.array_equal(Tn.values.argmax(axis=0), [2, 0, 3, 1, 2]) and np.array_equal(Tn.values.sum(axis=0), np.ones(5))


def test_inverse_transform_of_the_scores_returns_every_samples_centroid(ctx):
    X, lab = planted()
    m = planted_model(ctx)
    rec = m.inverse_transform(m.scores())
    assert rec.dims == ("time", "x") and rec.shape == (600, 2048)
    cen = np.asarray(m.centroids().values, np.float64)
    got = np.asarray(rec.values, np.float64)
    assert np.abs(got - cen[lab]).max() <= 4 * U24 * np.abs(cen).max()
    one = m.inverse_transform(m.scores().sel(mode=2))                             # one mode: its centroid's departure from the mean
    dev = np.asarray(one.values, np.float64)
    assert np.abs(dev[lab != 1] - dev[lab != 1][0]).max() <= 4 * U24 * np.abs(cen).max()


def test_init_random_state_and_two_fits_bit_for_bit(ctx):
    X, lab = planted()
    a = planted_model(ctx)
    b = fit(ctx, line(X), n_modes=4, n_init=8, random_state=SEED)
    for key in ("components", "centroids_pc", "labels", "counts", "restart_inertias", "restart_centroids", "restart_labels"):
        assert np.array_equal(a.data[key], b.data[key]), key
    assert a.inertia() == b.inertia() and np.array_equal(a.stats["iterations"], b.stats["iterations"])
    other = fit(ctx, line(X), n_modes=4, n_init=8, random_state=SEED + 1)
    assert other.stats["seeds"].tolist() != a.stats["seeds"].tolist() and np.array_equal(fitted_labels(other), lab)
    # init= replaces the seeding: one restart from the named samples
    init = [int(np.nonzero(lab == j)[0][0]) for j in (3, 1, 0, 2)]
    c = fit(ctx, line(X), n_modes=4, init=init, random_state=SEED)              # (the random_state is the inner PCA's as well)
    assert np.array_equal(c.data["input_data"], a.data["input_data"])
    assert c.stats["seeds"].tolist() == [init] and c.restart_inertias().shape == (1,) and np.isnan(c.classifiability())
    assert np.array_equal(fitted_labels(c), lab) and c.data["mode_order"].tolist() == [2, 1, 3, 0]
    assert np.array_equal(c.data["centroids_pc"], a.data["centroids_pc"])         # the same partition: the same float64 means
    ref = kr.lloyd(c.data["input_data"], c.data["input_data"][init], 300)
    assert ref["iters"] == c.stats["iterations"][0] and ref["min_margin"] > kr.undecided_margin(14)


def test_max_iter_leaves_a_restart_unconverged(ctx):
    X, lab = planted()
    a = planted_model(ctx)
    m = fit(ctx, line(X), n_modes=4, n_init=8, random_state=SEED, max_iter=2)
    full = a.stats["iterations"]
    assert (full > 2).any() and (full <= 2).any()
    assert np.array_equal(m.stats["converged"], full <= 2) and np.array_equal(m.stats["iterations"], np.minimum(full, 2))
    assert (m.restart_inertias() >= a.restart_inertias()).all() and m.stats["launches"] == 1
    S32, seeds = m.data["input_data"], m.stats["seeds"]
    for r in range(8):
        assert np.array_equal(kr.lloyd(S32, S32[seeds[r]], 2)["labels"], m.data["restart_labels"][r])


def test_a_fit_in_short_launches_equals_the_fit_in_one(ctx, monkeypatch):
    """past the cap of a launch the model chains launches: with the cap lowered to 2 updates the same fit takes three launches
    and ends in the same state, with the same iteration counts"""
    from xeofs_amd.single import kmeans as km

    X, lab = planted()
    a = planted_model(ctx)
    monkeypatch.setattr(km, "LAUNCH_ITERS", 2)
    m = fit(ctx, line(X), n_modes=4, n_init=8, random_state=SEED)
    assert m.stats["launches"] == 3 and a.stats["launches"] == 1                  # the slowest restart takes 5 updates
    assert np.array_equal(m.stats["iterations"], a.stats["iterations"]) and m.stats["converged"].all()
    for key in ("components", "centroids_pc", "labels", "counts", "restart_inertias", "restart_centroids", "restart_labels"):
        assert np.array_equal(a.data[key], m.data[key]), key


def test_refusals_at_fit(ctx):
    import xeofs_amd as xe

    X = np.random.default_rng(0).standard_normal((6, 20)).astype(np.float32)
    for kw, exc, word in ((dict(n_modes=7, n_pca_modes=3), ValueError, "n_modes"),
                          (dict(n_modes=2, n_pca_modes=3, init=[1, 6]), ValueError, "init")):
        m = xe.single.KMeans(**kw)
        m.ctx = ctx
        with pytest.raises(exc, match=word):
            m.fit(line(X), dim="time")
    m = xe.single.KMeans(n_modes=2, n_pca_modes=3)
    m.ctx = ctx
    with pytest.raises(TypeError, match="complex"):
        m.fit(line(X.astype(np.complex64)), dim="time")
    # k = n: every sample its own mode
    m = fit(ctx, line(X), n_modes=6, n_pca_modes=3, n_init=3, random_state=0)
    assert sorted(fitted_labels(m).tolist()) == list(range(6)) and m.inertia() == 0.0 and m.stats["n_empty"] == 0
