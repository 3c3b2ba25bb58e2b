"""GPU parity of the bootstrap path: `eofx_resample_f32` and
`xeofs_amd.validation.EOFBootstrapper` against the oracle restatement of xeofs/validation/bootstrapper.py."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eof_oracle as orc  # noqa: E402  (checker only)


@pytest.mark.parametrize("n,p", [(70, 300), (600, 1100), (513, 64)])
def test_resample_matches_numpy(ctx, n, p):
    from xeofs_amd import engine

    rng = np.random.default_rng(0)
    X = (rng.standard_normal((n, p)) + np.linspace(-2, 2, p)).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    idx = rng.choice(n, n, replace=True)
    for center in (True, False):
        bm, mean, tv = engine.resample(ctx, mat, idx, center=center)
        Xb = X[idx].astype(np.float64)
        ref = Xb - Xb.mean(0) if center else Xb
        got = bm.download()
        assert got.shape == (n, p)
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
        assert np.allclose(mean, Xb.mean(0), atol=1e-6)
        assert np.isclose(tv, Xb.var(axis=0, ddof=1).sum(), rtol=1e-6)
        bm.free()
    with pytest.raises(ValueError):
        engine.resample(ctx, mat, np.array([0, n]))
    mat.free()


def test_eof_bootstrapper_vs_oracle(ctx):
    import xeofs_amd as xe

    vals = orc.synthetic_field(120, 8, 10, rank=6, seed=3)[0].reshape(120, 8, 10)
    X = xe.DataArray(vals, dims=("time", "lat", "lon"))
    model = xe.single.EOF(n_modes=3, random_state=1).fit(X, "time")
    had_layout = model.data["input_data"].has_sample_layout()
    bs = xe.validation.EOFBootstrapper(n_bootstraps=5, seed=11).fit(model, random_state=0)
    Xs = vals.reshape(120, -1).astype(np.float64)
    eof = orc.eof_fit(Xs, 3, random_state=1)
    eof["input_data"] = Xs - Xs.mean(0)
    ref = orc.eof_bootstrap(eof, 3, n_bootstraps=5, seed=11, random_state=0)
    assert bs.get_params() == {"n_bootstraps": 5, "seed": 11}
    ev = bs.explained_variance()
    assert ev.dims == ("n", "mode") and ev.shape == (5, 3) and list(ev.coords["n"]) == [1, 2, 3, 4, 5]
    assert np.allclose(ev.values, ref["explained_variance"], rtol=2e-4)
    assert np.allclose(bs.total_variance().values, ref["total_variance"], rtol=1e-5)
    comps = bs.components()
    assert comps.dims == ("n", "mode", "lat", "lon") and comps.shape == (5, 3, 8, 10)
    C = comps.values.reshape(5, 3, -1).transpose(0, 2, 1)
    for b in range(5):
        for j in range(3):
            assert np.dot(C[b, :, j], ref["components"][b, :, j]) > 1 - 1e-4, (b, j)   # incl. the aligned sign
    sc = bs.scores()
    assert sc.dims == ("n", "mode", "time") and sc.shape == (5, 3, 120)
    S = sc.values.transpose(0, 2, 1)
    assert np.allclose(S, ref["scores"], atol=2e-3 * np.abs(ref["scores"]).max())
    # seed determinism of the member selection
    bs2 = xe.validation.EOFBootstrapper(n_bootstraps=5, seed=11).fit(model, random_state=0)
    assert np.array_equal(bs2.data["scores"], bs.data["scores"])
    assert (bs.explained_variance_ratio().values <= 1).all()
    # the sample-contiguous copy the members run over is released again: the model's matrix keeps its footprint
    assert model.data["input_data"].has_sample_layout() == had_layout


def test_bootstrap_member_operator(ctx):
    """`BootstrapOps`: the member X_b = H X through panel products on the ORIGINAL matrix -- against the resampled,
    re-centred matrix itself; H / H^T are the engine's gather / segment-sum kernels (`eofx_panel_bootstrap_f32`, no
    library GEMM), on an in-place matrix (no layout is built), plus the member's total variance from the row norms."""
    import torch
    from xeofs_amd import engine
    from xeofs_amd.validation.bootstrapper import BootstrapOps

    n, p = 333, 1100
    rng = np.random.default_rng(4)
    X = (rng.standard_normal((n, p)) * rng.uniform(0.5, 3, p) + rng.standard_normal(p)).astype(np.float32)
    mat, _ = engine.preprocess(ctx, torch.as_tensor(X, device="cuda"), want_stats=False, keep_raw=True, in_place=True)
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    idx = rng.integers(0, n, n)
    Xb = Xc[idx] - Xc[idx].mean(0)
    Z = torch.zeros((mat.n_pad, 32), device="cuda"); Z[:n] = torch.randn((n, 32), device="cuda")
    Y = torch.zeros((mat.p_pad, 32), device="cuda"); Y[:p] = torch.randn((p, 32), device="cuda")
    outs = []
    for rep in range(2):
        ops = BootstrapOps(ctx, mat, idx)
        # H and H^T on their own against dense float64 algebra
        Hd = -np.bincount(idx, minlength=n)[None, :].repeat(n, 0) / n
        Hd[np.arange(n), idx] += 1.0
        Zh = Z[:n].double().cpu().numpy()
        assert np.abs(ops._h(Z)[:n].double().cpu().numpy() - Hd @ Zh).max() <= 1e-6 * np.abs(Zh).max()
        assert np.abs(ops._ht(Z)[:n].double().cpu().numpy() - Hd.T @ Zh).max() <= 1e-6 * np.abs(Zh).max()
        assert not bool(ops._h(Z)[n:].any()) and not bool(ops._ht(Z)[n:].any())      # padding rows stay zero
        t = ops.tmul(Z)[:p].double().cpu().numpy()
        m = ops.mul(Y)[:n].double().cpu().numpy()
        want_t = Xb.T @ Z[:n].double().cpu().numpy()
        want_m = Xb @ Y[:p].double().cpu().numpy()
        assert np.abs(t - want_t).max() <= 2e-5 * np.abs(want_t).max()
        assert np.abs(m - want_m).max() <= 2e-5 * np.abs(want_m).max()
        c = ops.counts.cpu().numpy()
        tv = (c @ engine.sample_norms(ctx, mat) ** 2 - n * ops.mean_sumsq()) / (n - 1)
        assert np.isclose(tv, (Xb ** 2).sum() / (n - 1), rtol=1e-5)
        outs.append((t, m))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])     # bitwise reproducible
    assert mat.layout()[0] in (False, 0)          # still in place: no layout was materialised


# --------------------------------------------------------------------------- the member operator at its edges
# (n, rows_pad, L): one and two samples; a panel far longer than n; the minimal width 4; widths above 64, where
# panel_colsum_part_kernel walks column blocks (96 = 64 + 32, 160 = 64 + 64 + 32); n one past a 512 boundary
BST_SHAPES = [(1, 512, 4), (2, 512, 32), (333, 512, 96), (513, 1024, 160), (700, 2048, 64)]
BST_DRAWS = ["identity", "reversed", "all_last", "all_first", "random", "lower_half"]


def bst_draw(kind, n, rng):
    if kind == "identity":
        return np.arange(n, dtype=np.int64)
    if kind == "reversed":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    if kind == "all_last":
        return np.full(n, n - 1, dtype=np.int64)
    if kind == "all_first":
        return np.zeros(n, dtype=np.int64)
    if kind == "random":
        return rng.integers(0, n, n).astype(np.int64)
    return rng.integers(0, max(1, n // 2), n).astype(np.int64)      # the upper half of the rows: empty segments


def bst_arrays(idx, n):
    """what eofx_panel_bootstrap_f32 documents: order = stable argsort of the draw, rowptr = where every source row starts"""
    order = np.argsort(idx, kind="stable").astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))]).astype(np.int64)
    return order, rowptr


def bst_reference(idx, P64):
    """[(transpose, float64 reference, per-element bound)] of H W and H^T Z for the draw idx on the float64 panel P64 [n x L],
    H = G - 1 c^T / n dense:
      H W     the gather is exact, the rank-one term is subtracted in float64 and rounded once:
              |err| <= 2^-23 (|W[idx[i]]| + |c^T W| / n)   (2^-24 of the result's magnitude, with room for the float64 sums)
      H^T Z   the float64 segment sum is rounded to float32, the rank-one term subtracted in float64 and rounded again:
              |err| <= 2^-23 (sum over the segment of |Z| + c_r |1^T Z| / n)"""
    n = P64.shape[0]
    counts = np.bincount(idx, minlength=n)
    Gd = np.zeros((n, n))
    Gd[np.arange(n), idx] = 1.0
    Hd = Gd - counts[None, :] / n
    eps = 2.0 ** -23
    return [(False, Hd @ P64, eps * (np.abs(P64[idx]) + np.abs(counts @ P64)[None, :] / n)),
            (True, Hd.T @ P64, eps * (Gd.T @ np.abs(P64) + counts[:, None] * np.abs(P64.sum(axis=0))[None, :] / n))]


@pytest.mark.parametrize("kind", BST_DRAWS)
@pytest.mark.parametrize("n,rows_pad,L", BST_SHAPES)
def test_bootstrap_operator_edges(ctx, n, rows_pad, L, kind):
    """`engine.panel_bootstrap` on its own against the dense float64 H = G - 1 c^T / n, per element within the bounds of
    `bst_reference`, from an output full of NaN (padding rows >= n exact zeros afterwards), twice with equal bits."""
    import torch
    from xeofs_amd import engine

    rng = np.random.default_rng(1000 * n + L + BST_DRAWS.index(kind))
    idx = bst_draw(kind, n, rng)
    order, rowptr = bst_arrays(idx, n)
    counts = np.diff(rowptr)
    if kind == "lower_half" and n >= 2:
        assert rowptr[n] == rowptr[n - 1] and (counts[n // 2:] == 0).all()      # empty segments, the last row among them
    if kind in ("all_last", "all_first"):
        assert counts.max() == n                                                # one row drawn n times
    P = np.zeros((rows_pad, L), np.float32)
    P[:n] = rng.standard_normal((n, L)) * 10.0 ** rng.uniform(-2, 2, L) + rng.standard_normal(L)
    P64 = P[:n].astype(np.float64)
    dev = f"cuda:{ctx.device}"
    Pd, di, do, dr = (torch.as_tensor(a, device=dev) for a in (P, idx, order, rowptr))
    for transpose, ref, bound in bst_reference(idx, P64):
        outs = []
        for rep in range(2):
            out = torch.full((rows_pad, L), float("nan"), dtype=torch.float32, device=dev)
            got = engine.panel_bootstrap(ctx, Pd, n, di, do, dr, transpose, out=out)
            assert got is out
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        g = outs[0]
        what = f"{'H^T Z' if transpose else 'H W'} n={n} L={L} {kind}"
        assert np.array_equal(g, outs[1], equal_nan=True), f"{what}: not reproducible"
        assert np.isfinite(g).all(), f"{what}: {np.count_nonzero(~np.isfinite(g))} elements unwritten"
        assert not g[n:].any(), f"{what}: padding rows are not exact zeros"
        err = np.abs(g[:n].astype(np.float64) - ref)
        print(f"{what}: worst error / bound = {(err / (bound + 1e-300)).max():.3g}")
        assert np.all(err <= bound), f"{what}: {np.count_nonzero(err > bound)} elements outside the bound"


def test_bootstrap_ops_hands_over_the_documented_arrays(ctx):
    """`BootstrapOps` gives the kernels the same idx / order / rowptr as the numpy construction of the test above"""
    from xeofs_amd import engine
    from xeofs_amd.validation.bootstrapper import BootstrapOps

    n = 333
    rng = np.random.default_rng(8)
    mat = engine.from_dense(ctx, rng.standard_normal((n, 8)).astype(np.float32))
    for kind in BST_DRAWS:
        idx = bst_draw(kind, n, rng)
        order, rowptr = bst_arrays(idx, n)
        ops = BootstrapOps(ctx, mat, idx)
        for got, want in ((ops.idx, idx), (ops.order, order), (ops.rowptr, rowptr), (ops.counts, np.diff(rowptr))):
            g = got.cpu().numpy()
            assert g.shape == want.shape and np.array_equal(g, want), kind
        assert ops.idx.dtype == ops.order.dtype == ops.rowptr.dtype == engine._torch().int64
    mat.free()


def test_bootstrap_operator_argument_errors(ctx):
    """EOFX_ERR_ARG (ValueError) for an output that aliases the input, rows_pad < n, a width off a multiple of 4 and
    n = 0; nothing is written, and the context serves a correct call afterwards"""
    import torch
    from xeofs_amd import engine

    n, dev = 40, f"cuda:{ctx.device}"
    rng = np.random.default_rng(2)
    idx = bst_draw("random", n, rng)
    order, rowptr = bst_arrays(idx, n)
    di, do, dr = (torch.as_tensor(a, device=dev) for a in (idx, order, rowptr))
    P = torch.zeros((512, 8), dtype=torch.float32, device=dev)
    P[:n] = torch.as_tensor(rng.standard_normal((n, 8)).astype(np.float32), device=dev)
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=torch.float32, device=dev)      # noqa: E731
    for transpose, ref, bound in bst_reference(idx, P[:n].double().cpu().numpy()):
        with pytest.raises(ValueError):
            engine.panel_bootstrap(ctx, P, n, di, do, dr, transpose, out=P)                   # P_out aliases P_in
        out = nan(32, 8)
        with pytest.raises(ValueError):
            engine.panel_bootstrap(ctx, P[:32], n, di, do, dr, transpose, out=out)            # rows_pad < n
        assert bool(torch.isnan(out).all())
        out = nan(512, 6)
        with pytest.raises(ValueError):
            engine.panel_bootstrap(ctx, torch.zeros((512, 6), device=dev), n, di, do, dr, transpose, out=out)     # L = 6
        assert bool(torch.isnan(out).all())
        out = nan(512, 8)
        with pytest.raises(ValueError):
            engine.panel_bootstrap(ctx, P, 0, di, do, dr, transpose, out=out)                 # n = 0
        assert bool(torch.isnan(out).all())
        got = engine.panel_bootstrap(ctx, P, n, di, do, dr, transpose, out=nan(512, 8)).cpu().numpy()
        assert np.all(np.abs(got[:n].astype(np.float64) - ref) <= bound) and not got[n:].any()       # the bounds of the edges test
