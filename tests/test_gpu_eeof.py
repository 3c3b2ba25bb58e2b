"""GPU tests of Extended EOF analysis (xeofs_amd.single.ExtendedEOF, csrc/eofx_lag.hpp).  Expected values come from a numpy
restatement of the reference's eager embedding (xeofs/single/eeof.py:124-134) and the float64 oracle."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eof_oracle as orc  # noqa: E402  (checker only)
from test_gpu_parity import _check_svd, _field  # noqa: E402


def embed(X, tau, E):
    """eeof.py:124-134: E copies shifted by e tau, lag-major columns, the last (E - 1) tau samples cut"""
    n_emb = X.shape[0] - (E - 1) * tau
    return np.concatenate([X[e * tau:e * tau + n_emb] for e in range(E)], axis=1)


def centred_embedding(X, tau, E):
    Xe = embed(np.asarray(X, dtype=np.float64), tau, E)
    return Xe - Xe.mean(axis=0)


def mock_values():
    rng = np.random.default_rng(7)
    return rng.normal(5, 3, size=(25, 5, 4)) + 2 * np.sin(np.linspace(0, 2 * np.pi, 25))[:, None, None]


def mock_data_array(values=None):
    import xeofs_amd as xe

    return xe.DataArray(mock_values() if values is None else values, dims=("time", "lat", "lon"),
                        coords={"time": np.arange(2001, 2026), "lat": [20.0, 30.0, 40.0, 50.0, 60.0],
                                "lon": [-10.0, 0.0, 10.0, 20.0]}, name="t2m")


@pytest.fixture(scope="module")
def field700():
    return _field(700, 3000, seed=11)


# --------------------------------------------------------------------------- operator products
@pytest.mark.parametrize("in_place", [False, True], ids=["owned", "in_place"])
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_lag_products(ctx, in_place, prec):
    import torch
    from xeofs_amd import engine

    rng = np.random.default_rng(3)
    X = (rng.standard_normal((300, 200)) + 2.0).astype(np.float32)
    mat, st = engine.preprocess(ctx, X, center=True, in_place=in_place)
    assert mat.layout()[1] == in_place
    Xp = mat.download().astype(np.float64)
    cases = [(E, tau, L) for E in (1, 3, 8) for tau in (1, 4) for L in (32, 96)] + [(40, 1, 32)]   # last: E L above the group cap
    for E, tau, L in cases:
        n_emb = 300 - (E - 1) * tau
        mean, tv = engine.lag_stats(ctx, mat, tau, E)
        Xe = embed(Xp, tau, E)
        mu = Xe.mean(axis=0)
        Xc = Xe - mu
        got_mu = mean.cpu().numpy().reshape(E, mat.p_pad)
        assert not got_mu[:, 200:].any()
        assert np.allclose(got_mu[:, :200].reshape(-1), mu, rtol=1e-10, atol=1e-10 * np.abs(mu).max())
        tv_ref = (Xc ** 2).sum() / (n_emb - 1)
        assert abs(tv - tv_ref) <= 1e-10 * tv_ref, (E, tau, tv, tv_ref)
        Z = rng.standard_normal((n_emb, L)).astype(np.float32)
        Y = rng.standard_normal((E * 200, L)).astype(np.float32)
        npad = (n_emb + 511) // 512 * 512
        Zp = engine.panel_import(ctx, Z, npad, L)
        Yp = torch.zeros((E * mat.p_pad, L), dtype=torch.float32, device=Zp.device)
        Yp.view(E, mat.p_pad, L)[:, :200] = torch.as_tensor(Y, device=Zp.device).view(E, 200, L)
        got_t = engine.lag_tmul(ctx, mat, tau, E, mean, Zp, prec=prec).cpu().numpy().reshape(E, mat.p_pad, L)
        got_m = engine.lag_mul(ctx, mat, tau, E, mean, Yp, prec=prec).cpu().numpy()
        assert not got_t[:, 200:].any() and not got_m[n_emb:].any()
        got_t = got_t[:, :200].reshape(E * 200, L)
        ref_t, ref_m = Xc.T @ Z, Xc @ Y
        if prec == "f32":
            for got, ref in ((got_t, ref_t), (got_m[:n_emb], ref_m)):
                assert np.linalg.norm(got - ref) <= 1e-6 * np.linalg.norm(ref), (E, tau, L)
        else:           # the f16x3 class of test_gpu_parity.test_panel_tmul_mul, on the centred operator
            bt = np.abs(Xe).T @ np.abs(Z) + np.abs(mu)[:, None] * np.abs(Z.sum(axis=0))
            bm = np.abs(Xe) @ np.abs(Y) + np.abs(mu @ Y)
            assert np.all(np.abs(got_t - ref_t) <= 1e-5 * bt), (E, tau, L)
            assert np.all(np.abs(got_m[:n_emb] - ref_m) <= 1e-5 * bm), (E, tau, L)
        emb = engine.lag_embed(ctx, mat, tau, E).cpu().numpy()
        assert np.array_equal(emb, Xe.astype(np.float32))
    mat.free()


# --------------------------------------------------------------------------- model against the oracle
def _fit_field(X, **kw):
    import xeofs_amd as xe

    return xe.single.ExtendedEOF(**kw).fit(xe.DataArray(X, dims=("time", "x")), "time")


def test_randomized_route_vs_oracle(field700):
    X = field700
    k, tau, E = 12, 2, 8
    m = _fit_field(X, n_modes=k, tau=tau, embedding=E, random_state=5, solver="randomized")
    Xc = centred_embedding(X, tau, E)
    Uo, so, Vo = orc.decomposer_fit(Xc, k, random_state=5, solver="randomized")
    n_emb = X.shape[0] - (E - 1) * tau
    s = m.data["norms"]
    U = m.data["scores"][:n_emb] / s.astype(np.float32)
    _check_svd(U, s, m.data["components"], Uo, so, Vo, Xc, k)
    tv = (Xc ** 2).sum() / (n_emb - 1)
    assert abs(m.data["total_variance"] - tv) <= 1e-6 * tv
    assert np.allclose(m.explained_variance_ratio().values, so ** 2 / (n_emb - 1) / tv, rtol=2e-5)
    assert np.isnan(m.data["scores"][n_emb:]).all()
    # the same seed: bitwise the same fit
    m2 = _fit_field(X, n_modes=k, tau=tau, embedding=E, random_state=5, solver="randomized")
    for key in ("components", "scores", "norms"):
        assert np.array_equal(m.data[key], m2.data[key], equal_nan=True), key


def test_exact_branch_and_inverse_transform():
    rng = np.random.default_rng(4)
    X = (rng.standard_normal((60, 8)) * np.linspace(1, 3, 8) + 10.0).astype(np.float32)
    tau, E = 2, 3
    n_emb = 60 - (E - 1) * tau
    k = min(n_emb, E * 8)
    m = _fit_field(X, n_modes=k, tau=tau, embedding=E, solver="full")
    pre = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    Xc = centred_embedding(pre, tau, E)
    so = np.linalg.svd(Xc, compute_uv=False)[:k]
    s = m.data["norms"]
    assert np.all(np.abs(s - so) <= 1e-5 * so[0])
    comps = m.components()
    assert comps.dims == ("mode", "embedding", "x") and list(comps.coords["embedding"]) == [0, 2, 4]
    rec = m.inverse_transform(m.scores()).values
    expect = X[:n_emb].astype(np.float64) - pre[:n_emb].mean(axis=0)
    assert np.allclose(rec[:n_emb], expect, atol=2e-4 * np.abs(X).max())
    assert np.isnan(rec[n_emb:]).all()


@pytest.mark.parametrize("center", [True, False])
def test_pca_route_vs_restatement(center):
    rng = np.random.default_rng(9)
    X = _field(200, 60, seed=9)
    if not center:
        X = X - X.mean(axis=0) + rng.standard_normal(60).astype(np.float32)
    tau, E, mp, k = 2, 3, 10, 4
    m = _fit_field(X, n_modes=k, tau=tau, embedding=E, n_pca_modes=mp, center=center, random_state=2)
    pre = X.astype(np.float64) - (X.astype(np.float64).mean(axis=0) if center else 0.0)
    Up, sp, Vp = orc.decomposer_fit(pre - pre.mean(axis=0), mp, random_state=2)
    Xc = centred_embedding(Up * sp, tau, E)
    Ue, se, Ve = orc.decomposer_fit(Xc, k, random_state=2)
    V = np.concatenate([Vp @ Ve[e * mp:(e + 1) * mp] for e in range(E)], axis=0)
    s = m.data["norms"]
    assert np.all(np.abs(s - se) <= 1e-4 * se[0]), (s, se)
    got = m.data["components"].astype(np.float64)
    for j in range(k):
        if _gap(se, j) > 1e-2:
            c = np.dot(got[:, j], V[:, j]) / np.linalg.norm(got[:, j]) / np.linalg.norm(V[:, j])
            assert c >= 1 - 1e-4, (j, c)
    assert m.components().dims == ("mode", "embedding", "x")


def _gap(s, j):
    lo = abs(s[j] - s[j + 1]) / s[j] if j + 1 < len(s) else 1.0
    hi = abs(s[j - 1] - s[j]) / s[j] if j > 0 else 1.0
    return min(lo, hi)


def test_embedding_one_is_eof():
    import xeofs_amd as xe

    X = _field(300, 900, seed=2)
    a = _fit_field(X, n_modes=5, tau=1, embedding=1, random_state=3, solver="randomized")
    b = xe.single.EOF(n_modes=5, random_state=3, solver="randomized").fit(xe.DataArray(X, dims=("time", "x")), "time")
    sb = b.data["norms"]
    assert np.all(np.abs(a.data["norms"] - sb) <= 1e-5 * sb[0])
    ca, cb = a.components().values[:, 0], b.components().values
    for j in range(5):
        assert np.dot(ca[j].astype(np.float64), cb[j]) >= 1 - 1e-5, j
    assert abs(a.data["total_variance"] - b.data["total_variance"]) <= 1e-6 * b.data["total_variance"]


# --------------------------------------------------------------------------- the reference's contract (test_eeof.py)
@pytest.mark.parametrize("dim", [("time",), ("lat", "lon"), ("lon", "lat")])
def test_reference_contract(dim):
    import xeofs_amd as xe

    X = mock_data_array()
    m = xe.single.ExtendedEOF(n_modes=5, tau=2, embedding=2, random_state=0).fit(X, dim)
    fdims = tuple(d for d in X.dims if d not in dim)
    c, sc = m.components(), m.scores()
    assert set(c.dims) == {"mode", "embedding", *fdims} and set(sc.dims) == {"mode", *dim}
    assert (m.explained_variance().values > 0).all() and m.explained_variance_ratio().values.sum() <= 1 + 1e-5
    assert c.attrs["model"] == "Extended EOF Analysis"
    # inverse_transform: a scalar mode and a slice (test_eeof.py:411-...)
    one = xe.DataArray(sc.values[0], dims=sc.dims[1:], coords=dict({d: sc.coords[d] for d in sc.dims[1:]}, mode=1))
    r1 = m.inverse_transform(one)
    assert set(r1.dims) == set(X.dims)
    r2 = m.inverse_transform(sc.isel(mode=slice(1, 3)))
    assert set(r2.dims) == set(X.dims)
    # NaN fixtures (conftest.py:265-278)
    for kind in ("full_dimensional", "boundary"):
        v = mock_values()
        v[:, 1, :] = np.nan
        v[1 if kind == "full_dimensional" else 0] = np.nan
        mm = xe.single.ExtendedEOF(n_modes=3, tau=2, embedding=2, random_state=0).fit(mock_data_array(v), dim)
        assert set(mm.components().dims) == {"mode", "embedding", *fdims} and set(mm.scores().dims) == {"mode", *dim}
    # Dataset and list inputs
    X2 = mock_data_array(mock_values() ** 2)
    ds = xe.Dataset({"a": X, "b": X2})
    out = xe.single.ExtendedEOF(n_modes=3, tau=2, embedding=2, random_state=0).fit(ds, dim).components()
    assert set(out.data_vars) == {"a", "b"} and set(out["a"].dims) == {"mode", "embedding", *fdims}
    out = xe.single.ExtendedEOF(n_modes=3, tau=2, embedding=2, random_state=0).fit([X, X2], dim).components()
    assert isinstance(out, list) and len(out) == 2 and set(out[1].dims) == {"mode", "embedding", *fdims}
    # isolated NaN
    v = mock_values()
    v[0, 1, 0] = np.nan
    with pytest.raises(ValueError):
        xe.single.ExtendedEOF(n_modes=3, tau=2, embedding=2).fit(mock_data_array(v), dim)


def test_scores_nan_tail_and_dropped_samples():
    import xeofs_amd as xe

    v = mock_values()
    v[3] = np.nan                                     # a dropped sample: the shift runs over the 24 valid ones
    m = xe.single.ExtendedEOF(n_modes=3, tau=2, embedding=3, random_state=0).fit(mock_data_array(v), "time")
    s = m.scores().values
    assert np.isnan(s[:, 3]).all() and np.isnan(s[:, -4:]).all()
    assert not np.isnan(np.delete(s[:, :-4], 3, axis=1)).any()


# --------------------------------------------------------------------------- at scale: no E-fold copy
def test_no_embedding_copy_at_scale(ctx):
    import torch
    import xeofs_amd as xe

    n, p, E, tau, k = 4096, 131072, 24, 3, 10
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((n, 16), device="cuda", generator=g) @ torch.randn((16, p), device="cuda", generator=g)
    X += 0.3 * torch.randn((n, p), device="cuda", generator=g)
    torch.cuda.synchronize()
    field = n * p * 4
    free0, _ = torch.cuda.mem_get_info()
    m = xe.single.ExtendedEOF(n_modes=k, tau=tau, embedding=E, random_state=1).fit(xe.DataArray(X, dims=("time", "x")), "time")
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * field, (free0 - free1) / field
    n_emb = n - (E - 1) * tau
    # U[t] s = X_ext[t] V for the centred embedded rows: window means from float64 column sums
    S = torch.zeros(p, dtype=torch.float64, device="cuda")
    for r in range(0, n, 256):
        S += X[r:r + 256].double().sum(0)
    wmean = torch.stack([(S - X[:e * tau].double().sum(0) - X[e * tau + n_emb:].double().sum(0)) / n_emb for e in range(E)])
    V = torch.as_tensor(m.data["components"], device="cuda").double()
    rows = np.random.default_rng(0).choice(n_emb, 64, replace=False)
    Xr = torch.stack([torch.cat([X[t + e * tau].double() - wmean[e] for e in range(E)]) for t in rows])
    ref = (Xr @ V).cpu().numpy()
    got = m.data["scores"][rows].astype(np.float64)
    assert np.linalg.norm(got - ref) <= 1e-4 * np.linalg.norm(ref)
