"""The delay-embedding operator of ExtendedEOF (csrc/eofx_lag.hpp: eofx_lag_stats_f64 / _tmul_f32 / _mul_f32 / _embed_f32)
at its edges, case by case against float64.  The rules are those of tests/test_gpu_product_routes.py:

  reference     the float64 embedding `embed()` / `centred_embedding()` of tests/test_gpu_eeof.py applied to the float32 matrix
                the engine holds: `mat.download()`; for an in-place or raw matrix the download of the two-layout matrix
                preprocessed with the same arguments
  products      per element TOL[prec] * bound (TOL of tests/test_gpu_product_routes.py) with the absolute-value product of the
                centred operator that test_gpu_eeof.py::test_lag_products uses:
                    bt = |Xe|^T |Z| + |mu| |1^T Z|          bm = |Xe| |Y| + |mu . Y|
  dirty output  `out=` is full of NaN before the call; the rows j >= p of every lag block of Ye and the rows t >= n' of Wn are
                exact zeros afterwards; both are allocated with GUARD rows behind the documented size, which stay NaN
  lag_embed     bitwise equal to `embed()` cast to float32
  window means  |mu - ref| <= 4 n eps64 (sum_t |x_t|) / n': the kernel takes a window sum as the difference F(b) - F(a) of
                a naive float64 prefix sum; F(t) of at most n terms carries at most (n - 1) eps64 sum|x| (u = eps64 / 2 per
                addition, first order), the difference twice that, the subtraction and the division one rounding each
  variance      |tv - ref| <= 8 n eps64 Q / (n' - 1), Q the sum of squares over all windows: tv = (q - n' sum mu^2) / (n' - 1)
                per feature with q a naive float64 sum of at most n products (<= n eps64 Q_j) and n' mu^2 <= Q_j known to
                4 n eps64 relative from the means' bound squared; for a centred field the 1e-10 relative bound of
                test_lag_products is kept wherever it is the tighter one
  reproducible  every call is repeated once and compared bitwise (fixed summation order, no atomics)
  size          every matrix is at most 64 MB

CASES are the shapes (n, p, E, tau, L) that reach each edge; `lag_groupsize`, `lag_groups`, `n_emb`, `tmul_nt_ok` restate
the host rules of csrc/eofx_plans.hpp ONLY to choose shapes and to prove (tests/test_lag_model_host.py, no GPU needed) that
the list reaches them; tests/test_plans_cpu.py compares them with the header itself.  p is used as given for an owned matrix and rounded up to a multiple of 4 for an in-place or raw
one (a field stays in place when its feature count is a multiple of 4).

The sample-contiguous source (LagSrc.mode == 2): no public call yields a matrix with that layout alone from a real field
except the Hilbert stage on its lean route -- `engine.hilbert` of an in-place matrix returns the imaginary part in the
sample-contiguous layout only (tests/test_gpu_complex.py::test_complex_rsvd_lean_layout) --, so mode 2 is covered with
that output.  Only the statistics and lag_embed read the field through LagSrc; the products go through panel_tmul /
panel_mul, which build the layout they need.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_eeof import centred_embedding, embed  # noqa: E402
from test_gpu_product_routes import TOL  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)
GUARD = 64
LAG_GROUP_COLS = 1024           # EOFX_LAG_GROUP_COLS

CASES = [
    (1037, 2331, 3, 7, 32),     # several row and feature tiles; p % 4 != 0; n' = 1023
    (1037, 2331, 2, 525, 64),   # n' = 512 exactly; n'_pad = 512 < n_pad = 1536; windows disjoint
    (1037, 2331, 2, 524, 64),   # n' = 513, n'_pad = 1024
    (29, 45, 4, 9, 32),         # n' = 2: the variance divides by 1; padding dominates
    (29, 45, 2, 20, 32),        # n' = 9; rows 9..19 lie in no window
    (301, 900, 1, 1, 96),       # E = 1: must equal the plain centred products
    (301, 900, 11, 3, 96),      # G = 10, last group of 1
    (301, 900, 5, 2, 256),      # G = 4, last group of 1; Lw = 1024 and 256
    (301, 900, 3, 2, 544),      # G = 1; every lag is its own group at a panel above 512 columns
    (333, 5000, 8, 4, 64),      # in place: the split-K in-place X.Y under the fold
]
# one more than the list above: none of its shapes has BOTH n >= 512 and a group of 512 columns, so none reaches the NT
# kernel of the f16x3 X^T W (tmul_nt_ok); this one does (G = 2, Lw = 512), CASES[0] stays on the streaming tiles
NT_CASE = (1037, 2331, 2, 524, 256)
# and one with SEVERAL full groups before the shorter last one (G = 10: groups of 10, 10 and 1 lags): the middle group takes
# lag_fold_kernel's accumulator path (neither first nor last) with more than one lag, which CASES[8] reaches with G = 1 only
GROUPS_CASE = (301, 900, 21, 3, 96)
EXTRA_CASES = [NT_CASE, GROUPS_CASE]
ALL_PREC_CASES = (CASES[0], CASES[6])
IN_PLACE_ONLY = CASES[9]

# (case, source): every case on an owned matrix, the edges that depend on the source on the others
PLAN = ([(c, "owned") for c in CASES if c != IN_PLACE_ONLY] + [(c, "owned") for c in EXTRA_CASES]
        + [(CASES[i], "in_place") for i in (0, 1, 4, 6, 7, 9)]
        + [(CASES[i], "raw") for i in (0, 6)]
        + [(CASES[i], "sample_only") for i in (6, 7)])


def _up(a, b):
    return (a + b - 1) // b * b


def n_emb(n, E, tau):
    """n' = n - (E - 1) tau"""
    return n - (E - 1) * tau


def lag_groupsize(E, L):
    """lag_groupsize of csrc/eofx_plans.hpp"""
    return max(1, min(E, LAG_GROUP_COLS // max(L, 1)))


def lag_groups(E, L):
    """the lags per group, in launch order"""
    G = lag_groupsize(E, L)
    return [min(G, E - e0) for e0 in range(0, E, G)]


def tmul_nt_ok(n, Lw):
    """tmul_nt_ok for a written or raw matrix at these sizes (p_pad is a multiple of 512, the 32-bit limit is far away)"""
    return Lw >= 512 and n >= 512


def precisions(case, source):
    if source == "owned" and case in ALL_PREC_CASES:
        return list(TOL)
    return ["f16x3", "f32"]      # f16x3 first: it leaves an in-place matrix in place, the others build the written layout


def field(n, p, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, p)) * (0.5 + rng.random(p)) + 2.0 * rng.standard_normal(p)).astype(np.float32)


def uncentred_field():
    """(301 x 900), every feature offset by 1000 of its standard deviations"""
    rng = np.random.default_rng(77)
    sd = 0.5 + rng.random(900)
    return (rng.standard_normal((301, 900)) * sd + 1000.0 * sd * rng.choice([-1.0, 1.0], 900)).astype(np.float32)


def stats_reference(Xp, tau, E):
    """float64 window means [E p], total variance, and the two bounds of the module docstring"""
    n = Xp.shape[0]
    ne = n_emb(n, E, tau)
    X64 = Xp.astype(np.float64)
    Xe = embed(X64, tau, E)
    mu = Xe.mean(axis=0)
    tv = ((Xe - mu) ** 2).sum() / (ne - 1)
    mu_bound = np.tile(4.0 * n * EPS64 * np.abs(X64).sum(axis=0) / ne, E)
    tv_bound = 8.0 * n * EPS64 * (Xe ** 2).sum() / (ne - 1)
    return Xe, mu, tv, mu_bound, tv_bound


# ----------------------------------------------------------------------------------------------------------------------
def _nan(ctx, rows, L):
    import torch

    return torch.full((rows, L), float("nan"), dtype=torch.float32, device=f"cuda:{ctx.device}")


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _source(ctx, X, source):
    """-> (matrix under test, reference matrix or None, [matrices to free])"""
    from xeofs_amd import engine

    if source == "owned":
        mat, _ = engine.preprocess(ctx, X, center=True, in_place=False)
        assert mat.layout() == (True, False)
        return mat, mat, [mat]
    if source == "sample_only":
        A, _ = engine.preprocess(ctx, X, center=True, in_place=True)
        assert A.layout() == (False, True)
        B, _ = engine.hilbert(ctx, A, "exp", 0.2)
        assert B.layout() == (False, False) and B.has_sample_layout()
        return B, None, [A, B]
    m2, _ = engine.preprocess(ctx, X, center=True)
    mat, _ = engine.preprocess(ctx, X, center=True, keep_raw=source == "raw", in_place=source == "in_place")
    assert mat.layout() == (False, True) and mat.has_sample_layout() == (source == "raw")
    return mat, m2, [mat, m2]


def _stats(ctx, mat, tau, E, p, Xp, what, centred=True):
    """lag_stats twice (bitwise), against the float64 reference; -> (device means, total variance, Xe, mu)"""
    from xeofs_amd import engine

    mean, tv = engine.lag_stats(ctx, mat, tau, E)
    mean2, tv2 = engine.lag_stats(ctx, mat, tau, E)
    got = _host(mean).reshape(E, mat.p_pad)
    assert np.array_equal(got, _host(mean2).reshape(E, mat.p_pad)) and tv == tv2, f"{what}: statistics not reproducible"
    Xe, mu, tv_ref, mu_bound, tv_bound = stats_reference(Xp, tau, E)
    assert not got[:, p:].any(), f"{what}: window means of the padding features are not exact zeros"
    err = np.abs(got[:, :p].reshape(-1) - mu)
    print(f"{what}: worst window-mean error / bound = {(err / mu_bound).max():.3g}")
    assert np.all(err <= mu_bound), f"{what}: {np.count_nonzero(err > mu_bound)} window means outside the bound"
    if centred:
        tv_bound = min(tv_bound, 1e-10 * tv_ref)
    print(f"{what}: total variance error / bound = {abs(tv - tv_ref) / tv_bound:.3g}")
    assert abs(tv - tv_ref) <= tv_bound, (what, tv, tv_ref, tv_bound)
    return mean, tv, Xe, mu


def _embed(ctx, mat, tau, E, Xe, what):
    from xeofs_amd import engine

    a = _host(engine.lag_embed(ctx, mat, tau, E))
    b = _host(engine.lag_embed(ctx, mat, tau, E))
    assert np.array_equal(a, Xe.astype(np.float32)), f"{what}: lag_embed is not the embedding bit for bit"
    assert np.array_equal(a, b)


def _panels(ctx, mat, p, E, ne, L, seed):
    """random Z [n' x L] and Y [E p x L] with their zero-padded device panels (Y lag-major, p_pad rows per lag)"""
    import torch
    from xeofs_amd import engine

    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((ne, L)).astype(np.float32)
    Y = rng.standard_normal((E * p, L)).astype(np.float32)
    Zp = engine.panel_import(ctx, Z, _up(ne, 512), L)
    Yp = torch.zeros((E * mat.p_pad, L), dtype=torch.float32, device=Zp.device)
    Yp.view(E, mat.p_pad, L)[:, :p] = torch.as_tensor(Y, device=Zp.device).view(E, p, L)
    return Z, Y, Zp, Yp


def _check(g, ref, bound, what):
    assert np.isfinite(g).all(), f"{what}: {np.count_nonzero(~np.isfinite(g))} elements unwritten or not finite"
    err = np.abs(g.astype(np.float64) - ref)
    ratio = float((err / (bound + 1e-300)).max())
    print(f"{what}: worst error / bound = {ratio:.3g}")
    bad = np.argwhere(err > bound + 1e-300)
    assert bad.size == 0, f"{what}: {len(bad)} elements outside the bound, first at {bad[0]}, worst ratio {ratio:.3g}"


def _products(ctx, mat, tau, E, p, mean, Xe, mu, Z, Y, Zp, Yp, prec, what):
    """both products from NaN-filled outputs with guard rows, twice, against float64 within TOL[prec] * (bt, bm)"""
    from xeofs_amd import engine

    ne, L = Z.shape
    ne_pad, rows_t = _up(ne, 512), E * mat.p_pad
    Xc = Xe - mu
    Z64, Y64 = Z.astype(np.float64), Y.astype(np.float64)
    bt = np.abs(Xe).T @ np.abs(Z64) + np.abs(mu)[:, None] * np.abs(Z64.sum(axis=0))
    bm = np.abs(Xe) @ np.abs(Y64) + np.abs(mu @ Y64)
    outs = []
    for rep in range(2):
        Ye, Wn = _nan(ctx, rows_t + GUARD, L), _nan(ctx, ne_pad + GUARD, L)
        engine.lag_tmul(ctx, mat, tau, E, mean, Zp, out=Ye[:rows_t], prec=prec)
        engine.lag_mul(ctx, mat, tau, E, mean, Yp, out=Wn[:ne_pad], prec=prec)
        outs.append((_host(Ye), _host(Wn)))
    (ye, wn), (ye2, wn2) = outs
    assert np.array_equal(ye, ye2, equal_nan=True) and np.array_equal(wn, wn2, equal_nan=True), f"{what}: not reproducible"
    assert np.isnan(ye[rows_t:]).all(), f"{what}: X_ext^T Z wrote behind its E p_pad rows"
    assert np.isnan(wn[ne_pad:]).all(), f"{what}: X_ext Y wrote behind its n'_pad rows"
    blocks = ye[:rows_t].reshape(E, mat.p_pad, L)
    assert np.isfinite(blocks).all(), f"{what}: X_ext^T Z left elements unwritten"
    assert not blocks[:, p:].any(), f"{what}: rows j >= p of a lag block are not exact zeros"
    assert np.isfinite(wn[:ne_pad]).all(), f"{what}: X_ext Y left elements unwritten"
    assert not wn[ne:ne_pad].any(), f"{what}: rows t >= n' of Wn are not exact zeros"
    _check(blocks[:, :p].reshape(E * p, L), Xc.T @ Z64, TOL[prec] * bt, f"{what} XtZ {prec}")
    _check(wn[:ne], Xc @ Y64, TOL[prec] * bm, f"{what} XY {prec}")
    return ye, wn


def _plain_products(ctx, mat, p, mean, Z, Y, Yp, ye, wn, prec, what):
    """E = 1: the lag operator is the plain centred operator.  Spread, relayout and fold are copies then, so the wide
    products inside are engine.panel_tmul / panel_mul of the same panels bit for bit, and the results are those minus the
    rank-one mean term, formed in float64 and rounded once:
        |Ye - (P - mu (1^T Z))| <= 2^-24 |P - mu (1^T Z)| + n eps64 |mu| sum|Z|       (round to nearest; the float64 column sum)
        |Wn - (P - mu^T Y)|     <= 2^-24 |P - mu^T Y|     + 2 p eps64 |mu|^T |Y|      (likewise; the weighted column sum)"""
    from xeofs_amd import engine

    n, L = Z.shape
    mu_dev = _host(mean)[:p]
    Z64, Y64 = Z.astype(np.float64), Y.astype(np.float64)
    Pt = _host(engine.panel_tmul(ctx, mat, engine.panel_import(ctx, Z, mat.n_pad, L), out=_nan(ctx, mat.p_pad, L), prec=prec))
    Pm = _host(engine.panel_mul(ctx, mat, Yp, out=_nan(ctx, mat.n_pad, L), prec=prec))
    want_t = Pt[:p].astype(np.float64) - mu_dev[:, None] * Z64.sum(axis=0)
    want_m = Pm[:n].astype(np.float64) - mu_dev @ Y64
    _check(ye[:p], want_t, 2.0 ** -24 * np.abs(want_t) + n * EPS64 * np.abs(mu_dev)[:, None] * np.abs(Z64).sum(axis=0),
           f"{what} XtZ {prec} against panel_tmul")
    _check(wn[:n], want_m, 2.0 ** -24 * np.abs(want_m) + 2 * p * EPS64 * (np.abs(mu_dev) @ np.abs(Y64)),
           f"{what} XY {prec} against panel_mul")


@pytest.mark.parametrize("case,source", PLAN, ids=[f"{'-'.join(map(str, c))}-{s}" for c, s in PLAN])
def test_lag_case(monkeypatch, ctx, case, source):
    """statistics, lag_embed and both products of one case on one source, in every precision `precisions` lists.
    In place: EOFX_NO_WIDE_XT keeps the f16x3 X Y on the in-place kernel at every panel width (the matrix must still hold
    no layout afterwards); the first other precision then makes the engine write the feature-contiguous layout, and the
    statistics read THAT (LagSrc.mode 0 instead of 1): the window means must not move by a bit, because lag_load applies the
    very expression (aff_map) that wrote the layout.
    Sample-contiguous only: the statistics and lag_embed run BEFORE the reference is downloaded -- the download (like
    X_ext^T Z) builds the feature-contiguous layout by an exact transpose, after which LagSrc would read mode 0."""
    n, p, E, tau, L = case
    if source in ("in_place", "raw"):
        p = _up(p, 4)
    assert n * p * 4 <= 64 << 20
    ne = n_emb(n, E, tau)
    what = f"{case} {source}"
    monkeypatch.setenv("EOFX_NO_WIDE_XT", "1")
    mat, ref, owned = _source(ctx, field(n, p, seed=n + p + E + tau), source)
    assert (mat.n, mat.p, mat.n_pad, mat.p_pad) == (n, p, _up(n, 512), _up(p, 512))
    if source == "sample_only":
        from xeofs_amd import engine

        (m1, tv1), (m1b, tv1b) = engine.lag_stats(ctx, mat, tau, E), engine.lag_stats(ctx, mat, tau, E)
        e1, e1b = _host(engine.lag_embed(ctx, mat, tau, E)), _host(engine.lag_embed(ctx, mat, tau, E))
        assert mat.layout() == (False, False) and mat.has_sample_layout()      # all four were read through mode 2
        assert np.array_equal(_host(m1), _host(m1b)) and tv1 == tv1b and np.array_equal(e1, e1b), f"{what}: mode 2 not reproducible"
        Xp = mat.download()
        assert mat.layout()[0] is True
        # mode 0 now, held to the bounds by _stats; mode 2 walks the same values in the same order: equal bits, tv included
        mean, tv, Xe, mu = _stats(ctx, mat, tau, E, p, Xp, what)
        assert np.array_equal(_host(m1), _host(mean)) and tv1 == tv, f"{what}: mode 2 statistics differ from mode 0"
        assert np.array_equal(e1, Xe.astype(np.float32)), f"{what}: mode 2 lag_embed is not the embedding bit for bit"
    else:
        Xp = ref.download()
        mean, _, Xe, mu = _stats(ctx, mat, tau, E, p, Xp, what)
        _embed(ctx, mat, tau, E, Xe, what)
    Z, Y, Zp, Yp = _panels(ctx, mat, p, E, ne, L, seed=L + E)
    for prec in precisions(case, source):
        ye, wn = _products(ctx, mat, tau, E, p, mean, Xe, mu, Z, Y, Zp, Yp, prec, what)
        if E == 1:
            _plain_products(ctx, mat, p, mean, Z, Y, Yp, ye, wn, prec, what)
        if prec == "f16x3" and case in (NT_CASE, CASES[0]) and source == "owned":
            # either side of tmul_nt_ok: the same bound with the NT kernel switched off (test_gpu_gram.py)
            assert tmul_nt_ok(n, lag_groups(E, L)[0] * L) == (case == NT_CASE)
            monkeypatch.setenv("EOFX_NO_TMUL_NT", "1")
            ye2, wn2 = _products(ctx, mat, tau, E, p, mean, Xe, mu, Z, Y, Zp, Yp, prec, what + " no NT")
            monkeypatch.delenv("EOFX_NO_TMUL_NT")
            assert np.array_equal(wn, wn2, equal_nan=True)
            if case != NT_CASE:
                assert np.array_equal(ye, ye2, equal_nan=True)      # the switch changes nothing below 512 columns
            else:       # two routes were compared: the NT kernel rounds differently from the streaming tiles
                assert not np.array_equal(ye, ye2, equal_nan=True), f"{what}: the NT kernel did not run"
        if source == "in_place" and prec == "f16x3":
            assert mat.layout() == (False, True) and not mat.has_sample_layout(), f"{what}: no longer in place"
    if source in ("in_place", "raw"):
        assert mat.layout()[0] is True          # a non-f16x3 product wrote the feature-contiguous layout
        mean2, _, _, _ = _stats(ctx, mat, tau, E, p, Xp, what + " after the layout was written")
        assert np.array_equal(_host(mean), _host(mean2)), f"{what}: window means moved with the layout"
        _embed(ctx, mat, tau, E, Xe, what)
    for m in owned:
        m.free()


def test_uncentred_field(ctx):
    """a field 1000 standard deviations off zero, straight from `from_dense`: the window sums cancel nothing, the variance
    cancels six digits -- the derived bound on tv is about 1e-6 relative here while an error in a window boundary is of
    order 1 / n'.  The float64 reference itself stays well inside the bound: tests/test_lag_model_host.py recomputes it in
    long double on this very field."""
    from xeofs_amd import engine

    X = uncentred_field()
    n, p = X.shape
    mat = engine.from_dense(ctx, X)
    assert np.array_equal(mat.download(), X)
    for E, tau, L in [(5, 2, 256), (2, 200, 32), (3, 7, 32)]:
        what = f"uncentred E={E} tau={tau}"
        mean, _, Xe, mu = _stats(ctx, mat, tau, E, p, X, what, centred=False)
        _embed(ctx, mat, tau, E, Xe, what)
        Z, Y, Zp, Yp = _panels(ctx, mat, p, E, n_emb(n, E, tau), L, seed=E)
        _products(ctx, mat, tau, E, p, mean, Xe, mu, Z, Y, Zp, Yp, "f64", what)
    mat.free()


# ----------------------------------------------------------------------------------------------------------------------
def _serves(ctx, mat, Xp, what):
    """the context still serves a correct call"""
    n, p = Xp.shape
    mean, _, Xe, mu = _stats(ctx, mat, 9, 3, p, Xp, what + ": afterwards")
    Z, Y, Zp, Yp = _panels(ctx, mat, p, 3, n_emb(n, 3, 9), 32, seed=1)
    _products(ctx, mat, 9, 3, p, mean, Xe, mu, Z, Y, Zp, Yp, "f32", what + ": afterwards")


def test_argument_errors(ctx):
    """every argument error of the four entries raises what `engine.raise_for` maps its code to (EOFX_ERR_ARG and
    EOFX_ERR_SHAPE: ValueError, told apart by the engine's message) and leaves the context able to serve a correct call"""
    import torch
    from test_gpu_product_routes import _layout_field
    from xeofs_amd import _lib, engine

    n, p = 29, 45
    X = field(n, p, seed=5)
    mat, _ = engine.preprocess(ctx, X, center=True)
    Xp = mat.download()
    mean, _ = engine.lag_stats(ctx, mat, 9, 3)
    dev = mean.device
    Z32 = torch.zeros((512, 32), dtype=torch.float32, device=dev)
    Y32 = torch.zeros((8 * mat.p_pad, 32), dtype=torch.float32, device=dev)      # (sized for the largest embedding below)
    mean8 = torch.zeros(8 * mat.p_pad, dtype=torch.float64, device=dev)

    def every_entry(tau, E, match):
        """(straight to the ABI where the wrapper would size a buffer from n' or from embedding = 0)"""
        with pytest.raises(ValueError, match=match):
            _lib.raise_for(ctx.lib.eofx_lag_stats_f64(ctx.handle, mat.handle, tau, E, _lib.ptr(mean8), None), ctx.handle)
        with pytest.raises(ValueError, match=match):
            engine.lag_tmul(ctx, mat, tau, E, mean8, Z32, out=_nan(ctx, 8 * mat.p_pad, 32))
        with pytest.raises(ValueError, match=match):
            engine.lag_mul(ctx, mat, tau, E, mean8, Y32, out=_nan(ctx, 512, 32))
        with pytest.raises(ValueError, match=match):
            _lib.raise_for(ctx.lib.eofx_lag_embed_f32(ctx.handle, mat.handle, tau, E, _lib.ptr(Y32)), ctx.handle)

    # n' = 1, n' = 0, n' < 0: EOFX_ERR_SHAPE
    for tau, E in [(7, 5), (29, 2), (8, 5)]:
        assert n_emb(n, E, tau) == {(7, 5): 1, (29, 2): 0, (8, 5): -3}[(tau, E)]
        every_entry(tau, E, "at least 2 are needed")
        _serves(ctx, mat, Xp, f"n' = {n_emb(n, E, tau)}")
    # tau = 0, embedding = 0: EOFX_ERR_ARG
    every_entry(0, 3, "tau >= 1, embedding >= 1")
    _serves(ctx, mat, Xp, "tau = 0")
    every_entry(3, 0, "tau >= 1, embedding >= 1")
    _serves(ctx, mat, Xp, "embedding = 0")
    # a panel width that is no multiple of 32
    with pytest.raises(ValueError, match="bad argument"):
        engine.lag_tmul(ctx, mat, 9, 3, mean, torch.zeros((512, 48), device=dev), out=_nan(ctx, 3 * mat.p_pad, 48))
    with pytest.raises(ValueError, match="bad argument"):
        engine.lag_mul(ctx, mat, 9, 3, mean, torch.zeros((3 * mat.p_pad, 48), device=dev), out=_nan(ctx, 512, 48))
    _serves(ctx, mat, Xp, "L = 48")
    # window means on the host
    host_mean = np.zeros(3 * mat.p_pad)
    with pytest.raises(ValueError, match="mean must be a device buffer"):
        engine.lag_tmul(ctx, mat, 9, 3, host_mean, Z32, out=_nan(ctx, 3 * mat.p_pad, 32))
    with pytest.raises(ValueError, match="mean must be a device buffer"):
        engine.lag_mul(ctx, mat, 9, 3, host_mean, Y32, out=_nan(ctx, 512, 32))
    with pytest.raises(ValueError, match="mean must be a device buffer"):
        _lib.raise_for(ctx.lib.eofx_lag_stats_f64(ctx.handle, mat.handle, 9, 3, _lib.ptr(host_mean), None), ctx.handle)
    _serves(ctx, mat, Xp, "host mean")
    # a precision the ABI does not know (the wrapper's own table has no name for it)
    for fn, a, b in ((ctx.lib.eofx_lag_tmul_f32, Z32, _nan(ctx, 3 * mat.p_pad, 32)), (ctx.lib.eofx_lag_mul_f32, Y32, _nan(ctx, 512, 32))):
        assert 7 not in _lib.PREC.values()
        with pytest.raises(ValueError, match="bad argument"):
            _lib.raise_for(fn(ctx.handle, mat.handle, 9, 3, _lib.ptr(mean), _lib.ptr(a), 32, _lib.ptr(b), 7), ctx.handle)
    with pytest.raises(KeyError):
        engine.lag_tmul(ctx, mat, 9, 3, mean, Z32, prec="f8")
    _serves(ctx, mat, Xp, "invalid precision")
    # a masked in-place matrix: EOFX_ERR_ARG from every entry
    Xm, w = _layout_field(301, 900, True, seed=1201)
    mm, _ = engine.preprocess(ctx, Xm, True, True, w, in_place=True, allow_masked=True)
    assert mm.masked
    mean_m = torch.zeros(3 * mm.p_pad, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="compacted matrix"):
        engine.lag_stats(ctx, mm, 2, 3)
    with pytest.raises(ValueError, match="compacted matrix"):
        engine.lag_tmul(ctx, mm, 2, 3, mean_m, Z32, out=_nan(ctx, 3 * mm.p_pad, 32))
    with pytest.raises(ValueError, match="compacted matrix"):
        engine.lag_mul(ctx, mm, 2, 3, mean_m, torch.zeros((3 * mm.p_pad, 32), device=dev), out=_nan(ctx, 512, 32))
    with pytest.raises(ValueError, match="compacted matrix"):
        _lib.raise_for(ctx.lib.eofx_lag_embed_f32(ctx.handle, mm.handle, 2, 3, _lib.ptr(_nan(ctx, 297, 3 * mm.p_phys))), ctx.handle)
    _serves(ctx, mat, Xp, "masked matrix")
    mm.free()
    mat.free()
