"""GPU tests of geographically weighted PCA (csrc/eofx_gw.hpp, engine.gwpca, xeofs_amd.single.GWPCA).

The checker is a float64 numpy restatement of the per-location algorithm (xeofs/single/gwpca.py, numba_utils.py:13-76):
weights of every location by the kernel of its distance, the weighted mean and covariance, the eigenpairs of C / W.
Algorithm-level tests feed it the engine's own preprocessed matrix (promoted to float64), so only the algorithm is compared.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_EARTH = 6371.0


# ------------------------------------------------------------------------------------------------ the restatement
def distances(xy, i, metric):
    if metric == "haversine":
        lon, lat = np.radians(xy[:, 0]), np.radians(xy[:, 1])
        a = np.sin((lat - lat[i]) / 2) ** 2 + np.cos(lat[i]) * np.cos(lat) * np.sin((lon - lon[i]) / 2) ** 2
        a = np.clip(a, 0.0, 1.0)
        return R_EARTH * 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))
    return np.sqrt(((xy - xy[i]) ** 2).sum(axis=1))


def weights(d, bw, kernel):
    u = d / bw
    if kernel == "bisquare":
        return np.where(d <= bw, (1 - u ** 2) ** 2, 0.0)
    if kernel == "gaussian":
        return np.exp(-0.5 * u ** 2)
    return np.exp(-0.5 * u)


def sign_rule(V):
    return np.where(np.abs(V.max(axis=0)) >= np.abs(V.min(axis=0)), 1.0, -1.0)


def local_pca(X, xy, metric, kernel, bw, k, centres):
    """-> full spectra [m, p] (descending), signed eigenvectors [m, p, k], total variances [m], neighbour counts [m]"""
    lam, vec, tv, cnt = [], [], [], []
    for i in centres:
        w = weights(distances(xy, i, metric), bw, kernel)
        keep = w > 0
        w, x = w[keep], X[keep]
        W = w.sum()
        mu = (w[:, None] * x).sum(0) / W
        y = x - mu
        C = (w[:, None] * y).T @ y / W
        ev, V = np.linalg.eigh(C)
        ev, V = ev[::-1], V[:, ::-1]
        V = V[:, :k] * sign_rule(V[:, :k])
        lam.append(ev)
        vec.append(V)
        tv.append(np.trace(C))
        cnt.append(keep.sum())
    return np.array(lam), np.array(vec), np.array(tv), np.array(cnt)


def check_parity(ev, V, tv, lam, Vr, tvr, k):
    """the gates of the issue: eigenvalues to 1e-5 lambda_1, total variance to 1e-6, |cos| >= 1 - 1e-5 with the same sign
    for modes with a relative gap >= 1e-3 (the sign only where the rule's max / min are not a near tie)"""
    lam1 = np.maximum(lam[:, 0], 1e-300)
    assert np.all(np.abs(ev - np.maximum(lam[:, :k], 0)) <= 1e-5 * lam1[:, None] + 1e-300), np.abs(ev - lam[:, :k]).max()
    assert np.all(np.abs(tv - tvr) <= 1e-6 * np.abs(tvr) + 1e-300)
    checked = 0
    for i in range(len(ev)):
        full = np.concatenate([lam[i], [-np.inf]])
        for m in range(k):
            gap = min(full[m - 1] - full[m] if m > 0 else np.inf, full[m] - full[m + 1]) / lam1[i]
            if gap < 1e-3 or lam[i, m] <= 1e-12 * lam1[i]:
                continue
            c = float(np.dot(V[i, :, m].astype(np.float64), Vr[i, :, m]))
            assert abs(c) >= 1 - 1e-5, (i, m, c)
            v = Vr[i, :, m]
            if abs(abs(v.max()) - abs(v.min())) > 1e-4:
                assert c > 0, (i, m, c)
            checked += 1
    assert checked > 0


def scatter(n, seed):
    """irregular points on the sphere, some across the dateline and within 2 degrees of both poles"""
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-180, 180, n)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    m = n // 20
    lon[:m] = rng.choice([-1, 1], m) * rng.uniform(178.5, 180, m)
    lat[m:2 * m] = rng.choice([-1, 1], m) * rng.uniform(88, 90, m)
    return np.stack([lon, lat], 1)


def field(xy, p, seed, offset=0.0):
    """locally structured data: a rotation that turns with the longitude over decreasing scales (clear local gaps)"""
    rng = np.random.default_rng(seed)
    n = xy.shape[0]
    s = np.linspace(6.0, 0.5, p) ** 1.5
    z = rng.normal(size=(n, p)) * s
    th = np.radians(xy[:, 0]) + 0.5 * np.radians(xy[:, 1])
    X = z.copy()
    X[:, 0] = np.cos(th) * z[:, 0] - np.sin(th) * z[:, 1]
    X[:, 1] = np.sin(th) * z[:, 0] + np.cos(th) * z[:, 1]
    if offset:
        X += offset * (1.0 + 0.5 * np.sin(np.radians(xy[:, 1]))[:, None] * np.cos(np.arange(p))[None, :])
    return X.astype(np.float32)


def fit_engine(ctx, X, xy, k, bw, metric, kernel):
    from xeofs_amd import engine

    mat, _ = engine.preprocess(ctx, X, True, False, None, True)
    Xp = mat.download().astype(np.float64)
    out = engine.gwpca(ctx, mat, xy, k, bw, metric, kernel)
    mat.free()
    return Xp, out


BANDWIDTH = {("haversine", "bisquare"): 1500.0, ("haversine", "gaussian"): 600.0, ("haversine", "exponential"): 300.0,
             ("euclidean", "bisquare"): 15.0, ("euclidean", "gaussian"): 6.0, ("euclidean", "exponential"): 3.0}


@pytest.mark.parametrize("metric", ["haversine", "euclidean"])
@pytest.mark.parametrize("kernel", ["bisquare", "gaussian", "exponential"])
def test_parity_metric_kernel(ctx, metric, kernel):
    xy = scatter(2000, 1)
    X = field(xy, 12, 2)
    bw = BANDWIDTH[(metric, kernel)]
    Xp, (V, ev, tv, st) = fit_engine(ctx, X, xy, 3, bw, metric, kernel)
    assert V.shape == (2000, 12, 3) and ev.shape == (2000, 3) and tv.shape == (2000,)
    idx = np.arange(0, 2000, 4)
    lam, Vr, tvr, _ = local_pca(Xp, xy, metric, kernel, bw, 3, idx)
    check_parity(ev[idx], V[idx], tv[idx], lam, Vr, tvr, 3)
    orth = np.einsum("npk,npl->nkl", V.astype(np.float64), V.astype(np.float64))
    assert np.abs(orth - np.eye(3)).max() < 1e-5
    assert 0 < st["tile_pairs_visited"] <= st["tile_pairs_total"]
    if kernel == "bisquare":
        assert st["tile_pairs_visited"] < st["tile_pairs_total"]


def test_offset_field(ctx):
    xy = scatter(2000, 3)
    X = field(xy, 12, 4, offset=1e3)
    Xp, (V, ev, tv, st) = fit_engine(ctx, X, xy, 3, 1500.0, "haversine", "bisquare")
    idx = np.arange(1, 2000, 4)
    lam, Vr, tvr, _ = local_pca(Xp, xy, "haversine", "bisquare", 1500.0, 3, idx)
    check_parity(ev[idx], V[idx], tv[idx], lam, Vr, tvr, 3)


def _spd_cases(rng):
    out = []
    for p in (1, 2, 17, 64):
        B = rng.normal(size=(p, p))
        out.append(("spd", B @ B.T + 0.1 * np.eye(p)))
        Q, _ = np.linalg.qr(rng.normal(size=(p, p)))
        d = np.ones(p)
        d[: p // 2] = 3.0
        out.append(("repeated", (Q * d) @ Q.T))
        Bl = rng.normal(size=(p, min(2, p)))
        out.append(("rank", Bl @ Bl.T))
        out.append(("zero", np.zeros((p, p))))
        out.append(("diag", np.diag(rng.permutation(np.arange(1.0, p + 1)))))
    return out


@pytest.mark.parametrize("case", range(20))
def test_batched_syev_vs_numpy(ctx, case):
    import torch

    from xeofs_amd import engine

    kind, A = _spd_cases(np.random.default_rng(5))[case]
    p = A.shape[0]
    batch = np.stack([A, 2 * A, A])
    w, V = engine.batched_syev(ctx, torch.as_tensor(batch, device="cuda"), p)
    w, V = w.cpu().numpy(), V.cpu().numpy()
    ref = np.linalg.eigvalsh(A)[::-1]
    scale = max(1.0, np.abs(ref).max())
    np.testing.assert_allclose(w[0], np.maximum(ref, 0), atol=1e-12 * scale * p, rtol=0)
    np.testing.assert_allclose(w[1], np.maximum(2 * ref, 0), atol=2e-12 * scale * p, rtol=0)
    assert np.array_equal(w[0], w[2]) and np.array_equal(V[0], V[2])        # same input, same bits
    for b in range(3):
        assert np.abs(V[b].T @ V[b] - np.eye(p)).max() < 1e-12 * max(p, 4)
        resid = batch[b] @ V[b] - V[b] * w[b]
        assert np.abs(resid).max() < 1e-11 * scale * p
        assert np.all(np.diff(w[b]) <= 0) and np.all(w[b] >= 0)
        assert np.all(np.abs(V[b].max(0)) >= np.abs(V[b].min(0)))           # the sign rule
    if kind == "zero":
        assert np.array_equal(V[0], np.eye(p))


def test_library_route_p100(ctx):
    xy = scatter(600, 7)
    X = field(xy, 100, 8)
    Xp, (V, ev, tv, st) = fit_engine(ctx, X, xy, 3, 2500.0, "haversine", "bisquare")
    assert V.shape == (600, 100, 3)
    idx = np.arange(0, 600, 3)
    lam, Vr, tvr, _ = local_pca(Xp, xy, "haversine", "bisquare", 2500.0, 3, idx)
    check_parity(ev[idx], V[idx], tv[idx], lam, Vr, tvr, 3)


def test_scale_one_degree_grid(ctx):
    lat = np.arange(-89.5, 90, 1.0)
    lon = np.arange(-179.5, 180, 1.0)
    g0, g1 = np.meshgrid(lat, lon, indexing="ij")
    xy = np.stack([g1.reshape(-1), g0.reshape(-1)], 1)
    assert xy.shape[0] == 64800
    X = field(xy, 16, 9)
    Xp, (V, ev, tv, st) = fit_engine(ctx, X, xy, 4, 500.0, "haversine", "bisquare")
    assert st["tile_pairs_visited"] < 0.1 * st["tile_pairs_total"]
    idx = np.sort(np.random.default_rng(10).choice(64800, 200, replace=False))
    lam, Vr, tvr, _ = local_pca(Xp, xy, "haversine", "bisquare", 500.0, 4, idx)
    check_parity(ev[idx], V[idx], tv[idx], lam, Vr, tvr, 4)


def test_two_fits_bitwise_equal(ctx):
    xy = scatter(1500, 11)
    X = field(xy, 20, 12)
    _, a = fit_engine(ctx, X, xy, 4, 1200.0, "haversine", "gaussian")
    _, b = fit_engine(ctx, X, xy, 4, 1200.0, "haversine", "gaussian")
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(u, v)


# ------------------------------------------------------------------------------------------------ model level
def mock_data_array():
    import xeofs_amd as xe

    rng = np.random.default_rng(7)
    noise = rng.normal(5, 3, size=(25, 5, 4))
    signal = 2 * np.sin(np.linspace(0, 2 * np.pi, 25))[:, None, None]
    return xe.DataArray(signal + noise, dims=("time", "lat", "lon"),
                        coords={"time": np.arange(25), "lat": [20.0, 30.0, 40.0, 50.0, 60.0], "lon": [-10.0, 0.0, 10.0, 20.0]},
                        name="t2m")


def _vals(a):
    from xeofs_amd import labelled

    return labelled.unpack(a)


@pytest.mark.parametrize("kernel", ["bisquare", "gaussian", "exponential"])
def test_model_mock_data(ctx, kernel):
    import xeofs_amd as xe

    X = mock_data_array()
    m = xe.single.GWPCA(n_modes=2, metric="haversine", kernel=kernel, bandwidth=5000)
    m.fit(X, dim=("lat", "lon"))
    comps = m.components()
    v, dims, coords, name, _ = _vals(comps)
    assert dims == ("mode", "time", "lat", "lon") and v.shape == (2, 25, 5, 4) and name == "components"
    np.testing.assert_array_equal(coords["mode"], [1, 2])
    ev, dims_e, _, _, _ = _vals(m.explained_variance())
    assert dims_e == ("mode", "lat", "lon") and ev.shape == (2, 5, 4)
    r, _, _, _, _ = _vals(m.explained_variance_ratio())
    assert np.all((r >= 0) & (r <= 1 + 1e-12)) and np.all(r.sum(0) <= 1 + 1e-12)
    assert np.all(ev[0] >= ev[1])
    llwc, dims_l, _, _, _ = _vals(m.largest_locally_weighted_components())
    assert dims_l == ("mode", "lat", "lon")
    assert set(np.unique(llwc)) <= set(range(25))
    # the argmax of |component| over the features maps to their time labels
    i = np.abs(v[0, :, 2, 1]).argmax()
    assert llwc[0, 2, 1] == i
    # dim order: the same local PCAs
    m2 = xe.single.GWPCA(n_modes=2, metric="haversine", kernel=kernel, bandwidth=5000).fit(X, dim=("lon", "lat"))
    ev2, dims2, _, _, _ = _vals(m2.explained_variance())
    assert dims2 == dims_e
    np.testing.assert_allclose(ev2, ev, rtol=1e-6)
    c2 = _vals(m2.components())[0]
    np.testing.assert_allclose(np.abs(c2), np.abs(v), atol=1e-4)


def test_model_matches_restatement(ctx):
    import xeofs_amd as xe

    X = mock_data_array()
    m = xe.single.GWPCA(n_modes=2, metric="haversine", kernel="gaussian", bandwidth=2000).fit(X, ("lat", "lon"))
    Xs = np.asarray(X.values).reshape(25, 20).T.astype(np.float32).astype(np.float64)
    Xs = Xs - Xs.mean(0)
    lat, lon = np.meshgrid([20.0, 30.0, 40.0, 50.0, 60.0], [-10.0, 0.0, 10.0, 20.0], indexing="ij")
    xy = np.stack([lon.reshape(-1), lat.reshape(-1)], 1)
    lam, _, tvr, _ = local_pca(Xs, xy, "haversine", "gaussian", 2000.0, 2, range(20))
    ev = _vals(m.explained_variance())[0].reshape(2, 20).T
    np.testing.assert_allclose(ev, lam[:, :2], rtol=1e-4)


def test_model_station_euclidean(ctx):
    import xeofs_amd as xe

    rng = np.random.default_rng(3)
    x, y = rng.uniform(0, 100, 60), rng.uniform(0, 100, 60)
    X = xe.DataArray(rng.normal(size=(60, 30)), dims=("station", "time"), coords={"x": x, "y": y})
    m = xe.single.GWPCA(n_modes=3, metric="euclidean", kernel="bisquare", bandwidth=40.0).fit(X, "station")
    v, dims, _, _, _ = _vals(m.components())
    assert dims == ("mode", "station", "time") and v.shape == (3, 60, 30)
    ev = _vals(m.explained_variance())[0]
    Xs = np.asarray(X.values, dtype=np.float32).astype(np.float64)
    lam, _, _, _ = local_pca(Xs - Xs.mean(0), np.stack([x, y], 1), "euclidean", "bisquare", 40.0, 3, range(60))
    np.testing.assert_allclose(ev.T, lam[:, :3], rtol=1e-4, atol=1e-5 * lam[:, 0].max())


def test_model_nan_row_and_isolated_locations(ctx):
    import xeofs_amd as xe

    X = mock_data_array()
    vals = np.array(X.values)
    vals[:, 1, :] = np.nan                    # the lat = 30 row: dropped, neither centre nor neighbour
    Xn = xe.DataArray(vals, X.dims, X.coords, "t2m")
    m = xe.single.GWPCA(n_modes=3, metric="haversine", kernel="bisquare", bandwidth=800.0).fit(Xn, ("lat", "lon"))
    ev = _vals(m.explained_variance())[0]
    assert np.all(np.isnan(ev[:, 1, :])) and np.all(np.isfinite(np.delete(ev, 1, axis=1)))
    c = _vals(m.components())[0]
    assert np.all(np.isnan(c[:, :, 1, :]))
    ok = np.stack([np.delete(vals, 1, axis=1)[:, :, :]]).reshape(25, -1).T
    keep_lat = [20.0, 40.0, 50.0, 60.0]
    lat, lon = np.meshgrid(keep_lat, [-10.0, 0.0, 10.0, 20.0], indexing="ij")
    xy = np.stack([lon.reshape(-1), lat.reshape(-1)], 1)
    Xs = ok.astype(np.float32).astype(np.float64)
    lam, _, _, cnt = local_pca(Xs - Xs.mean(0), xy, "haversine", "bisquare", 800.0, 3, range(16))
    got = np.delete(ev, 1, axis=1).reshape(3, 16).T
    np.testing.assert_allclose(got, np.maximum(lam[:, :3], 0), rtol=1e-5, atol=1e-6 * lam[:, 0].max())
    assert cnt.min() < 3                      # some locations have fewer neighbours than modes: trailing values are 0
    few = cnt < 3
    assert np.all(got[few, 2] <= 1e-9 * got[few, 0])
    V = np.delete(c, 1, axis=2).reshape(3, 25, 16).transpose(2, 1, 0)             # (loc, time, mode)
    for i in range(16):
        assert np.abs(V[i].T.astype(np.float64) @ V[i] - np.eye(3)).max() < 1e-5


def test_model_isolated_location_is_zero_covariance(ctx):
    import xeofs_amd as xe

    rng = np.random.default_rng(4)
    x = np.array([0.0, 1.0, 2.0, 500.0])           # the last station has no neighbour but itself
    X = xe.DataArray(rng.normal(size=(4, 6)), dims=("station", "time"), coords={"x": x, "y": np.zeros(4)})
    m = xe.single.GWPCA(n_modes=2, metric="euclidean", kernel="bisquare", bandwidth=5.0).fit(X, "station")
    ev = _vals(m.explained_variance())[0]
    r = _vals(m.explained_variance_ratio())[0]
    c = _vals(m.components())[0]
    assert np.all(ev[:, 3] == 0) and np.all(np.isnan(r[:, 3]))
    np.testing.assert_array_equal(c[:, 3, :], np.eye(6)[:2])
    with pytest.raises(NotImplementedError):
        m.scores()
    with pytest.raises(NotImplementedError):
        m.transform(X)
    with pytest.raises(NotImplementedError):
        m.inverse_transform(None)


def test_model_two_fits_bitwise_equal(ctx):
    import xeofs_amd as xe

    X = mock_data_array()
    a = xe.single.GWPCA(n_modes=2, bandwidth=3000).fit(X, ("lat", "lon"))
    b = xe.single.GWPCA(n_modes=2, bandwidth=3000).fit(X, ("lat", "lon"))
    for key in ("components", "explained_variance", "explained_variance_ratio"):
        assert np.array_equal(a.data[key], b.data[key], equal_nan=True)


# ------------------------------------------------------------------------------------------------ chunks
@pytest.mark.parametrize("kernel, chunk", [("bisquare", 48), ("gaussian", 1000), ("exponential", 700)])
def test_chunked_every_location(ctx, kernel, chunk):
    """many chunks (and an uneven last one): every location, so every chunk boundary, against the restatement, and against
    the single-chunk fit"""
    from xeofs_amd import engine

    xy = scatter(2000, 21)
    X = field(xy, 12, 22)
    bw = BANDWIDTH[("haversine", kernel)]
    mat, _ = engine.preprocess(ctx, X, True, False, None, True)
    Xp = mat.download().astype(np.float64)
    V, ev, tv, st = engine.gwpca(ctx, mat, xy, 3, bw, "haversine", kernel, chunk=chunk)
    V1, ev1, tv1, st1 = engine.gwpca(ctx, mat, xy, 3, bw, "haversine", kernel, chunk=2000)
    mat.free()
    assert st["chunks"] == -(-2000 // (-(-chunk // 16) * 16)) and st1["chunks"] == 1
    lam, Vr, tvr, _ = local_pca(Xp, xy, "haversine", kernel, bw, 3, range(2000))
    check_parity(ev, V, tv, lam, Vr, tvr, 3)
    np.testing.assert_allclose(ev, ev1, rtol=0, atol=1e-10 * lam[:, :1].max())
    np.testing.assert_allclose(tv, tv1, rtol=1e-12)


def test_scale_p32_four_chunks(ctx):
    """the 1-degree grid at p = 32: the automatic chunk size gives 4 chunks, the last one short; every location against a
    single-chunk fit, a random subset against the restatement"""
    from xeofs_amd import engine

    lat = np.arange(-89.5, 90, 1.0)
    lon = np.arange(-179.5, 180, 1.0)
    g0, g1 = np.meshgrid(lat, lon, indexing="ij")
    xy = np.stack([g1.reshape(-1), g0.reshape(-1)], 1)
    X = field(xy, 32, 23)
    mat, _ = engine.preprocess(ctx, X, True, False, None, True)
    Xp = mat.download().astype(np.float64)
    V, ev, tv, st = engine.gwpca(ctx, mat, xy, 4, 700.0, "haversine", "bisquare")
    V1, ev1, tv1, st1 = engine.gwpca(ctx, mat, xy, 4, 700.0, "haversine", "bisquare", chunk=64800)
    mat.free()
    assert st["chunks"] == 4 and st1["chunks"] == 1 and 64800 % st["chunk"] != 0
    np.testing.assert_allclose(ev, ev1, rtol=0, atol=1e-10 * ev1[:, 0].max())
    np.testing.assert_allclose(tv, tv1, rtol=1e-12)
    idx = np.sort(np.random.default_rng(24).choice(64800, 200, replace=False))
    lam, Vr, tvr, _ = local_pca(Xp, xy, "haversine", "bisquare", 700.0, 4, idx)
    check_parity(ev[idx], V[idx], tv[idx], lam, Vr, tvr, 4)


def test_library_route_chunks(ctx):
    """p = 100 in chunks of 128 locations (eofx_gw_cov_f64 with first > 0, an uneven last chunk): every location"""
    from xeofs_amd import engine

    xy = scatter(600, 25)
    X = field(xy, 100, 26)
    mat, _ = engine.preprocess(ctx, X, True, False, None, True)
    Xp = mat.download().astype(np.float64)
    V, ev, tv, st = engine.gwpca(ctx, mat, xy, 3, 2500.0, "haversine", "bisquare", chunk=128)
    mat.free()
    assert st["chunks"] == 5
    lam, Vr, tvr, _ = local_pca(Xp, xy, "haversine", "bisquare", 2500.0, 3, range(600))
    check_parity(ev, V, tv, lam, Vr, tvr, 3)


# ------------------------------------------------------------------------------------------------ C ABI arguments
def test_abi_rejects_bad_arguments(ctx):
    import torch

    from xeofs_amd import _lib, engine

    xy = scatter(100, 27)
    mat, _ = engine.preprocess(ctx, field(xy, 8, 28), True, False, None, True)
    lib, h = ctx.lib, ctx.handle
    comps = torch.empty((100, 8, 8), dtype=torch.float32, device="cuda")
    ev = torch.empty((100, 8), dtype=torch.float64, device="cuda")
    tv = torch.empty(100, dtype=torch.float64, device="cuda")
    cov = torch.empty((100, 8, 8), dtype=torch.float64, device="cuda")

    def gw(xy_, metric=1, kernel=0, bw=500.0, k=2, chunk=0):
        xy_ = np.ascontiguousarray(xy_, dtype=np.float64)
        return lib.eofx_gwpca_f64(h, mat.handle, xy_.ctypes.data, metric, kernel, bw, k, chunk, _lib.ptr(comps), _lib.ptr(ev),
                                  _lib.ptr(tv), None)

    def cv(first, count, bw=500.0):
        return lib.eofx_gw_cov_f64(h, mat.handle, xy.ctypes.data, 1, 0, bw, first, count, _lib.ptr(cov), _lib.ptr(tv), None)

    bad_xy = xy.copy()
    bad_xy[17, 1] = np.nan
    inf_xy = xy.copy()
    inf_xy[3, 0] = np.inf
    for rc in (gw(xy, bw=0.0), gw(xy, bw=-1.0), gw(xy, metric=2), gw(xy, kernel=3), gw(xy, kernel=-1), gw(xy, k=0),
               gw(xy, k=9), gw(bad_xy), gw(inf_xy), gw(xy, chunk=-5), cv(-1, 10), cv(95, 10), cv(0, 0), cv(0, 10, bw=0.0)):
        assert rc == _lib.ERR_ARG
    A = torch.zeros((2, 8, 8), dtype=torch.float64, device="cuda")
    w = torch.empty((2, 8), dtype=torch.float64, device="cuda")
    V = torch.empty((2, 8, 8), dtype=torch.float64, device="cuda")
    for p_, k_ in ((0, 1), (65, 1), (8, 0), (8, 9)):
        assert lib.eofx_batched_syev_f64(h, _lib.ptr(A), 2, p_, k_, _lib.ptr(w), _lib.ptr(V)) == _lib.ERR_ARG
    assert gw(xy) == _lib.EOFX_OK and cv(10, 50) == _lib.EOFX_OK
    with pytest.raises(ValueError, match="not finite"):
        engine.gwpca(ctx, mat, bad_xy, 2, 500.0)
    mat.free()


def test_model_limits(ctx):
    import xeofs_amd as xe

    rng = np.random.default_rng(29)
    X = xe.DataArray(rng.normal(size=(4, 3, 300)), dims=("lat", "lon", "time"))
    with pytest.raises(ValueError, match="at most 256"):
        xe.single.GWPCA(n_modes=2, bandwidth=5000).fit(X, ("lat", "lon"))
    small = xe.DataArray(rng.normal(size=(4, 3, 10)), dims=("lat", "lon", "time"))
    with pytest.raises(ValueError, match="n_modes"):
        xe.single.GWPCA(n_modes=11, bandwidth=5000).fit(small, ("lat", "lon"))
    x = np.arange(6.0)
    x[2] = np.nan
    S = xe.DataArray(rng.normal(size=(6, 5)), dims=("station", "time"), coords={"x": x, "y": np.zeros(6)})
    with pytest.raises(ValueError, match="not finite"):
        xe.single.GWPCA(n_modes=1, bandwidth=5.0, metric="euclidean").fit(S, "station")


def test_llwc_datetime_feature_labels(ctx):
    import xeofs_amd as xe

    X = mock_data_array()
    time = np.arange("2001", "2026", dtype="datetime64[Y]").astype("datetime64[ns]")
    vals = np.array(X.values)
    vals[:, 0, 0] = np.nan                     # one dropped location
    Xt = xe.DataArray(vals, X.dims, dict(X.coords, time=time), "t2m")
    m = xe.single.GWPCA(n_modes=2, bandwidth=3000).fit(Xt, ("lat", "lon"))
    llwc = _vals(m.largest_locally_weighted_components())[0]
    assert llwc.dtype == np.dtype("datetime64[ns]")
    assert np.isnat(llwc[:, 0, 0]).all() and not np.isnat(llwc[:, 1:, :]).any()
    c = _vals(m.components())[0]
    assert llwc[1, 2, 3] == time[np.abs(c[1, :, 2, 3]).argmax()]
    assert set(llwc[~np.isnat(llwc)].tolist()) <= set(time.tolist())
