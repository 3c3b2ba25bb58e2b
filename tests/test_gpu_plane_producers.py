"""The fp16 planes of the in-place X Y pass written by the kernel that PRODUCES the panel (atb_f16_kernel<.., PLANES> for
Y = X'^T Z, panel_matmul_kernel<false, true> for the Q of a Cholesky-QR) instead of by axb_bsplit_kernel on the finished panel.

The scale of the split then comes from a bound on max |panel| known before the producer runs (2 for Q; 2 sqrt(n) max |x'| for
X'^T Z with orthonormal Z) and not from the measured maximum.  Checked here, with EOFX_AXB_DMA=1 so that the LDS-DMA route runs
at small shapes:
  * the producers' planes are, bit for bit, axb_bsplit_kernel's planes of the same float32 panel with the same bound;
  * W from the new route is, bit for bit, W of the register kernel axb_f16_kernel given that scale;
  * max |panel| <= bound on every panel handed over (EOFX_AXB_CHECK_BOUND=1 turns a wrong bound into an error);
  * fits pass the float64-oracle gate of the other small-shape fit tests (singular values to 1e-5 of the leading one);
  * with a bound 2^6 and more above the panel's maximum (one outlier in the field), W differs from W with the measured maximum
    by no more than the product model of tests/test_gpu_product_routes.py with the bound in place of the maximum
    (tests/test_plane_bound_model_host.py checks in float64, without a GPU, that the model admits the case).
The shapes: n = 300 (two 256-row tiles, the second ragged) x p = 200 (K_all = 256, the last feature pair ragged) at L = 64 and
L = 96 (a 64- and a 32-column tile), and n = 257 x p = 64.  At 96 columns the X'^T Z product runs in the 128-column tile, which
has no plane epilogue: that panel goes through axb_bsplit_kernel as before (asserted), the Cholesky-QR producer covers it.
The plane epilogue of atb_f16_kernel belongs to the single-split launch (a split-K product is finished by the reduction and
split by axb_bsplit_kernel as before, asserted too): small shapes reach it with EOFX_ATB_SPLITS=1.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eof_oracle as orc  # noqa: E402  (checker only)

import test_gpu_product_routes as routes  # noqa: E402

SHAPES = [(300, 200, 64), (300, 200, 96), (257, 64, 64), (300, 200, 32)]      # (n, p, L); the last: the 32-column tile alone


@pytest.fixture()
def pctx(monkeypatch):
    """a context of its own: the route switches are read by a context at its first in-place product"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xeofs_amd import engine

    monkeypatch.setenv("EOFX_AXB_DMA", "1")
    monkeypatch.setenv("EOFX_NO_WIDE_XT", "1")          # 96 columns stay on the in-place route
    monkeypatch.setenv("EOFX_AXB_CHECK_BOUND", "1")
    monkeypatch.setenv("EOFX_ATB_SPLITS", "1")          # X'^T Z in one split: the kernel's own epilogue finishes the tile
    c = engine.Context(0)
    yield c
    c.close()


def field(n, p, seed, outlier=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)).astype(np.float32)
    if outlier:      # ONE sample-feature entry 2^10 times the typical magnitude
        X[n // 3, p // 2] = 1024.0
    return X


def orthonormal_panel(ctx, mat, L, seed):
    from xeofs_amd import engine

    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((mat.n, L)))
    return engine.panel_import(ctx, np.ascontiguousarray(Q, dtype=np.float32), mat.n_pad, L)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("producer", [0, 1], ids=["tmul", "cholqr"])
@pytest.mark.parametrize("n, p, L", SHAPES)
def test_producer_planes_and_product_bit_for_bit(pctx, n, p, L, producer):
    import torch
    from xeofs_amd import engine

    mat, st = engine.preprocess(pctx, torch.as_tensor(field(n, p, seed=n + L), device="cuda"), in_place=True)
    Zn = orthonormal_panel(pctx, mat, L, seed=7)
    if producer == 0 and L >= 96:
        with pytest.raises(ValueError, match="wrote no planes"):
            engine.axb_planes_probe(pctx, mat, Zn, producer)
        mat.free()
        return
    engine.plane_stats(pctx)
    r = engine.axb_planes_probe(pctx, mat, Zn, producer)
    stats = engine.plane_stats(pctx)
    assert (stats["produced_tmul"], stats["produced_cholqr"]) == ((1, 0), (0, 1))[producer] and stats["consumed"] == 1
    assert stats["checked"] == 1 and stats["min_slack"] >= 1.0
    # the planes: those of the splitting pass, every half of them (pad columns and the ragged last pair included)
    assert r["planes_prod"].size == ((L + 63) // 64) * ((p + 63) // 64) * 8192
    assert np.array_equal(r["planes_prod"], r["planes_split"])
    assert r["planes_prod"].any()
    # the product: the same bits from the producer's planes, the split planes and the register kernel with that scale
    assert np.array_equal(bits(r["w_prod"]), bits(r["w_split"]))
    assert np.array_equal(bits(r["w_prod"]), bits(r["w_reg"]))
    w = r["w_prod"].cpu().numpy()
    assert np.isfinite(w).all() and np.abs(w[:n]).max() > 0 and not w[n:].any()
    # the bound holds element by element
    y = r["y"].cpu().numpy()
    expect = 2.0 if producer else 2.0 * np.sqrt(np.float32(n)) * np.float32(np.abs(_centered(mat, st, n, p)).max())
    # (the matrix maximum the engine keeps comes from the column statistics: never below the true one, a rounding above it)
    assert float(expect) * (1 - 1e-6) <= r["bound"] <= float(expect) * 1.001
    assert np.abs(y).max() <= r["bound"] and not y[p:].any()
    if producer:
        G = y[:p].astype(np.float64).T @ y[:p].astype(np.float64)
        assert np.abs(G - np.eye(L)).max() < 1e-5          # (what the bound of 2 rests on)
    # against the measured maximum: the same product to the model's accuracy
    _within_model(_centered(mat, st, n, p), y[:p], r["bound"], w[:n], r["w_max"].cpu().numpy()[:n])
    mat.free()


def test_split_k_product_keeps_the_splitting_pass(pctx, monkeypatch):
    """X'^T Z over several sample splits ends in the split-K reduction: no plane epilogue, the request is declined"""
    import torch
    from xeofs_amd import engine

    monkeypatch.delenv("EOFX_ATB_SPLITS")
    n, p, L = 300, 200, 64
    assert routes.tmul_splits(n, p, L) > 1
    mat, st = engine.preprocess(pctx, torch.as_tensor(field(n, p, seed=1), device="cuda"), in_place=True)
    with pytest.raises(ValueError, match="wrote no planes"):
        engine.axb_planes_probe(pctx, mat, orthonormal_panel(pctx, mat, L, seed=7), 0)
    mat.free()


def _centered(mat, st, n, p):
    """the float32 matrix the in-place products stream: the field through the fitted map"""
    return mat.download()[:n, :p]


def _within_model(Xp, Y, bound, w_bound, w_max):
    """|W(bound) - W(maximum)| <= the product model with the bound in place of max |Y| (and both within it of float64)"""
    ref, rel, _ = routes.product_bounds(Xp.T, Y, routes.TOL["f16x3"])          # A = X'^T [p x n], B = Y [p x L]
    A64, B64 = np.abs(Xp.T.astype(np.float64)), np.abs(Y.astype(np.float64))
    absb = 2.0 ** -38 * (A64.max() * B64.sum(0)[None, :] + float(bound) * A64.sum(0)[:, None])
    model = rel + absb
    assert np.all(np.abs(w_bound.astype(np.float64) - w_max.astype(np.float64)) <= model)
    assert np.all(np.abs(w_bound.astype(np.float64) - ref) <= model)


@pytest.mark.parametrize("producer", [0, 1], ids=["tmul", "cholqr"])
def test_bound_far_above_the_maximum(pctx, producer):
    """one outlier of 2^10: the X'^T Z bound (2 sqrt(n) times the outlier) lies 2^6 and more above the panel's maximum (the
    outlier times one entry of an orthonormal column); for the Cholesky-QR producer a larger slack is forced by handing the
    probe a bound of 2^9"""
    import torch
    from xeofs_amd import engine

    n, p, L = 300, 200, 64
    mat, st = engine.preprocess(pctx, torch.as_tensor(field(n, p, seed=11, outlier=True), device="cuda"), in_place=True)
    Zn = orthonormal_panel(pctx, mat, L, seed=3)
    r = engine.axb_planes_probe(pctx, mat, Zn, producer, bound=512.0 if producer else 0.0)
    y = r["y"].cpu().numpy()
    slack = r["bound"] / np.abs(y).max()
    print(f"bound {r['bound']:.6g}, max |panel| {np.abs(y).max():.6g}, slack 2^{np.log2(slack):.2f}")
    assert slack >= 2.0 ** 6
    assert np.array_equal(r["planes_prod"], r["planes_split"])
    assert np.array_equal(bits(r["w_prod"]), bits(r["w_reg"]))
    _within_model(_centered(mat, st, n, p), y[:p], r["bound"], r["w_prod"].cpu().numpy()[:n], r["w_max"].cpu().numpy()[:n])
    mat.free()


def _gate(s, ref):
    assert np.all(np.abs(s - ref["norms"]) <= 1e-5 * ref["norms"][0]), (s, ref["norms"])


@pytest.mark.parametrize("n, p, k", [(300, 200, 40), (300, 200, 70), (257, 64, 40)])
def test_fit_at_the_issue_shapes(pctx, n, p, k):
    """(n > p: the tall side of these fits is the sample side, so the X Y pass is not their back product -- the gate holds on
    whatever route they take)"""
    from xeofs_amd import engine

    X = routes_field(n, p, seed=n + k)
    mat, st, U, s, V = engine.fit(pctx, X, k, random_state=3)
    _gate(s, orc.eof_fit(X.astype(np.float64), k, random_state=3))
    mat.free()


def routes_field(n, p, seed, rank=10, signal=None):
    """ten modes over unit noise, offset 5 (the field of the other fit tests); signal: their amplitude factor"""
    rng = np.random.default_rng(seed)
    amp = 3.0 * 0.8 ** np.arange(rank)
    X = (rng.standard_normal((n, rank)) * amp) @ rng.standard_normal((rank, p)) / np.sqrt(rank)
    return (X * (np.sqrt(max(n, p)) ** 0.5 if signal is None else signal) + rng.standard_normal((n, p)) + 5.0).astype(np.float32)


# fits whose back product IS the in-place X Y pass (n < p).  Small tall panels are re-orthonormalised in every iteration: every
# panel comes from the Cholesky-QR producer.  The last shape's tall panel is above that rule's 16 MiB (66 560 x 64 floats): from
# the second iteration on its panels come from the X'^T Z producer, the third and later without a float32 copy -- its modes are
# kept weak (sigma_1 / sigma_l = 4.3), since a peaked spectrum (above 30) re-orthonormalises the tall panel in every iteration.
@pytest.mark.parametrize("n, p, k, masked", [(150, 300, 40, False), (150, 300, 70, False), (120, 1000, 20, True),
                                             (96, 66052, 50, False)])
def test_fit_through_the_producers(pctx, monkeypatch, n, p, k, masked):
    from xeofs_amd import engine

    big = p > 60000
    X = routes_field(n, p, seed=n + k, signal=0.5 if big else None)
    if masked:
        X[:, 100:340] = np.nan
        X[:, ::17] = np.nan
    engine.plane_stats(pctx)
    mat, st, U, s, V = engine.fit(pctx, X, k, random_state=3, allow_masked=masked)
    stats = engine.plane_stats(pctx)
    print(stats)
    assert mat.masked == masked and st["fused"] == (k + 10 <= 64)      # (a wider sketch: statistics pass + eofx_rsvd_f32, same route)
    _gate(s, orc.eof_fit(X.astype(np.float64), k, random_state=3))
    assert stats["consumed"] == stats["checked"] == stats["produced_tmul"] + stats["produced_cholqr"] >= 3      # none went unused
    assert stats["min_slack"] >= 1.0          # (a panel above its bound fails the fit itself)
    if big:
        assert stats["produced_tmul"] >= 2 and stats["produced_cholqr"] == 2
    else:
        assert stats["produced_tmul"] == 0
    # the same fit without the verification (the float32 copy of a panel that only the X Y pass reads is then not written),
    # and with the route switched off altogether (axb_bsplit_kernel with the measured maxima)
    monkeypatch.setenv("EOFX_AXB_CHECK_BOUND", "0")
    c2 = engine.Context(0)
    mat2, st2, U2, s2, V2 = engine.fit(c2, X, k, random_state=3, allow_masked=masked)
    stats2 = engine.plane_stats(c2)
    assert stats2["checked"] == 0 and stats2["consumed"] == stats["consumed"]
    assert np.array_equal(s, s2) and np.array_equal(U, U2) and np.array_equal(V, V2)
    mat2.free()
    c2.close()
    monkeypatch.setenv("EOFX_AXB_DMA", "0")
    c3 = engine.Context(0)
    mat3, st3, U3, s3, V3 = engine.fit(c3, X, k, random_state=3, allow_masked=masked)
    assert engine.plane_stats(c3)["consumed"] == 0
    assert np.all(np.abs(s3 - s) <= 2e-6 * s[0]), (s, s3)
    mat3.free()
    c3.close()
    mat.free()


def test_two_step_fit_takes_the_producers_too(pctx):
    """eofx_rsvd_f32 on an in-place matrix (statistics pass first): the same route"""
    import torch
    from xeofs_amd import engine

    n, p, k = 150, 300, 40
    X = routes_field(n, p, seed=5)
    mat, st = engine.preprocess(pctx, torch.as_tensor(X, device="cuda"), in_place=True)
    engine.plane_stats(pctx)
    U, s, V = engine.rsvd(pctx, mat, k, random_state=3)
    stats = engine.plane_stats(pctx)
    assert stats["consumed"] == stats["checked"] == stats["produced_cholqr"] >= 3
    _gate(s, orc.eof_fit(X.astype(np.float64), k, random_state=3))
    mat.free()
