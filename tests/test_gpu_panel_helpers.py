"""The small panel kernels that decide signs, maxima and norms for every model, each against numpy in float64 (or bit for
bit where the operation is exact): ties, signed zeros, constant columns, row counts of 1 and 3, row counts off the unroll and
the grid stride, row counts beyond the partial cap (the part loop wraps), panel widths 32, 64, 96 and 256.

Tolerances: exact / bitwise where stated; 1 ulp of float32 for |re + i im|; 1e-14 * sum|a||b| for the float64 dot product;
1e-12 relative for the float64 norms; rows * 2^-53 * sum|a||b| for the float64 Gram matrix of a panel; the per-element product bound 1e-5 * sum|a||b| of tests/test_gpu_parity.py for the
Gram and complex products; 2e-5 of the series' scale for the Hilbert operator (test_hilbert_stage_vs_oracle);
1e-12 / 1e-11 * ||A|| for the host eigensolver.
"""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eof_oracle as orc  # noqa: E402  (checker only)

EOFX_ERR_ARG = -1
# 1, 3: tiny; 4 k + 1 and 16 k + 5: off the unrolls; 40005 > 2048 * 16 and 140003 > 1024 * 128: the part loops wrap
ROWS_WIDTHS = [(1, 32), (3, 96), (4097, 64), (16 * 300 + 5, 256), (40005, 32), (40005, 64), (40005, 96), (40005, 256),
               (140003, 32), (140003, 64)]


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _tie_panel(rows, L, seed):
    """[rows + 7, L] float32: N(0,1) with, per column in turn, exact ties of the maximum (+9) and of the minimum (-9) at
    rows (r, r + 4 * grid) -- the same thread one trip later --, (r, r + 1), (first, last), (3, 4) -- two workgroups --,
    a constant column, a column of zeros of both signs; the 7 rows beyond `rows` hold larger values and must be ignored"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((rows + 7, L)).astype(np.float32)
    grid = max(1, min((rows + 15) // 16, 2048))
    r = rows // 3
    pairs = [(r, r + 4 * grid), (r, r + 1), (0, rows - 1), (3, 4)]
    for c in range(L):
        kind = c % 7
        if kind < 4:
            a, b = (min(x, rows - 1) for x in pairs[kind])
            P[[a, b], c] = 9.0
            a2, b2 = (1, rows - 2) if kind == 2 else (min(x + 2, rows - 1) for x in pairs[kind])
            if rows > 4:
                P[[a2, b2], c] = -9.0
        elif kind == 4:
            P[:rows, c] = 0.75
        elif kind == 5:
            P[:rows, c] = np.where(np.arange(rows) % 2 == 0, -0.0, 0.0).astype(np.float32)
    P[rows:] = 100.0 * np.where(np.arange(L) % 2 == 0, 1.0, -1.0).astype(np.float32)
    P[rows + 3:] *= -1.0
    return P


@pytest.mark.parametrize("rows,L", ROWS_WIDTHS)
def test_panel_colargminmax(ctx, rows, L):
    """np.argmax / np.argmin per column over the first `rows` rows: the LOWEST row wins a tie wherever the two rows sit
    (same thread, neighbouring threads, two workgroups, first and last row); a constant column gives row 0 for both;
    +0.0 does not beat -0.0; rows beyond `rows` are ignored"""
    from xeofs_amd import engine

    P = _tie_panel(rows, L, rows + L)
    amax, amin = engine.panel_colargminmax(ctx, _dev(P), rows)
    amax, amin = _host(amax), _host(amin)
    assert np.array_equal(amax, np.argmax(P[:rows], axis=0)), np.flatnonzero(amax != np.argmax(P[:rows], axis=0))
    assert np.array_equal(amin, np.argmin(P[:rows], axis=0)), np.flatnonzero(amin != np.argmin(P[:rows], axis=0))
    const = [c for c in range(L) if c % 7 in (4, 5)]
    assert not amax[const].any() and not amin[const].any()


def test_panel_colargminmax_without_a_candidate_row(ctx):
    """a column in which no row takes part (no rows at all here; on the internal path every row masked through `rowscale`)
    gives row 0 -- a defined index inside the panel, never -1 (cpanel_pick_kernel reads the panel at that row)"""
    from xeofs_amd import engine

    P = _dev(np.ones((8, 64), np.float32))
    amax, amin = engine.panel_colargminmax(ctx, P, 0)
    assert not _host(amax).any() and not _host(amin).any()


@pytest.mark.parametrize("rows,L", ROWS_WIDTHS)
def test_panel_colminmax(ctx, rows, L):
    """max / min per column over the first `rows` rows, bit for bit (a zero of either sign where both occur).  Contract for
    NaN: a column holding one NaN returns the max / min of the others (fmaxf / fminf semantics)."""
    from xeofs_amd import engine

    P = _tie_panel(rows, L, rows + L)
    mx, mn = engine.panel_colminmax(ctx, _dev(P), rows)
    mx, mn = _host(mx), _host(mn)
    zero = np.array([c % 7 == 5 for c in range(L)])
    assert np.array_equal(mx[~zero].view(np.uint32), P[:rows].max(0)[~zero].view(np.uint32))
    assert np.array_equal(mn[~zero].view(np.uint32), P[:rows].min(0)[~zero].view(np.uint32))
    assert not mx[zero].any() and not mn[zero].any()
    if rows >= 3:
        Q = P.copy()
        Q[rows // 2, ::3] = np.nan
        mx, mn = engine.panel_colminmax(ctx, _dev(Q), rows)
        assert np.array_equal(_host(mx), np.nanmax(Q[:rows], axis=0)) and np.array_equal(_host(mn), np.nanmin(Q[:rows], axis=0))


def test_quad_kernels_reject_widths_that_are_not_a_multiple_of_four(ctx):
    """eofx_panel_colminmax_f32 and eofx_panel_import_f32 move 16-byte quads: L % 4, L <= 0 and rows < 0 are argument errors
    (the entries return before anything is launched); eofx_panel_colargminmax_f32 rejects L <= 0 and rows < 0"""
    import ctypes as C

    import torch
    from xeofs_amd._lib import ptr

    P = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    a = torch.zeros(64, dtype=torch.float32, device="cuda")
    b = torch.zeros(64, dtype=torch.float32, device="cuda")
    ia = torch.zeros(64, dtype=torch.int64, device="cuda")
    ib = torch.zeros(64, dtype=torch.int64, device="cuda")
    src = np.zeros((8, 6), np.float32)
    lib, h = ctx.lib, ctx.handle
    for rows, L in [(8, 30), (8, 2), (8, 0), (8, -4), (-1, 32)]:
        assert lib.eofx_panel_colminmax_f32(h, ptr(P), C.c_int64(rows), L, ptr(a), ptr(b)) == EOFX_ERR_ARG, (rows, L)
    for rows, l, rows_pad, L in [(8, 6, 64, 30), (8, 6, 64, 6), (8, 0, 64, 0), (-1, 6, 64, 32), (8, -1, 64, 32)]:
        assert lib.eofx_panel_import_f32(h, ptr(src), C.c_int64(rows), l, ptr(P), C.c_int64(rows_pad), L) == EOFX_ERR_ARG, (rows, l, L)
    for rows, L in [(8, 0), (8, -64), (-1, 64)]:
        assert lib.eofx_panel_colargminmax_f32(h, ptr(P), C.c_int64(rows), L, ptr(ia), ptr(ib)) == EOFX_ERR_ARG, (rows, L)
    assert lib.eofx_panel_colminmax_f32(h, ptr(P), C.c_int64(8), 64, ptr(a), ptr(b)) == 0       # the context still works


@pytest.mark.parametrize("L", [2, 4, 8, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("rows", [1, 3, 1029, 20005])
def test_cpanel_colabsmax(ctx, rows, L):
    """max over the rows of |re + i im| per complex column, in float32 arithmetic to 1 ulp (the kernel may fuse a * a + b * b);
    an all-zero column gives 0; `rows` smaller than the 256 / h rows a workgroup takes at a time"""
    from xeofs_amd import engine

    h = L // 2
    rng = np.random.default_rng(rows + L)
    P = (rng.standard_normal((rows + 3, L)) * 10.0 ** rng.uniform(-3, 3, L)).astype(np.float32)
    if h > 1:
        P[:, h - 1] = 0.0
        P[:, L - 1] = 0.0
    P[rows:] = 1.0e6                      # beyond `rows`: ignored
    got = _host(engine.cpanel_colabsmax(ctx, _dev(P), rows))
    a, b = P[:rows, :h], P[:rows, h:]
    ref = np.sqrt(a * a + b * b).max(0)
    assert ref.dtype == np.float32 and got.shape == (h,)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(ref)), (got, ref)
    assert h == 1 or got[h - 1] == 0.0


@pytest.mark.parametrize("rows,L", [(1, 2), (3, 64), (1029, 96), (20005, 64), (512, 256)])
@pytest.mark.parametrize("conj_left", [True, False])
def test_cpanel_combine(ctx, rows, L, conj_left):
    """out = P1 + sgn * [P2.im | -P2.re] with sgn = +1 for Z^H W (conj_left) and -1 for Z Y: one add per element, so bit for
    bit; also in place on P1, the form complex_svd.py uses"""
    from xeofs_amd import engine

    rng = np.random.default_rng(rows + L)
    P1 = rng.standard_normal((rows, L)).astype(np.float32)
    P2 = (rng.standard_normal((rows, L)) * 10.0 ** rng.uniform(-2, 2, L)).astype(np.float32)
    h, sg = L // 2, np.float32(1.0 if conj_left else -1.0)
    ref = np.concatenate([P1[:, :h] + sg * P2[:, h:], P1[:, h:] - sg * P2[:, :h]], axis=1)
    d1, d2 = _dev(P1), _dev(P2)
    out = _host(engine.cpanel_combine(ctx, d1, d2, conj_left))
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(_host(d1), P1)
    same = engine.cpanel_combine(ctx, d1, d2, conj_left, out=d1)
    assert same is d1 and np.array_equal(_host(d1).view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("count", [1, 255, 256, 257, 3_000_001])
def test_vec_dot(ctx, count):
    """float64 dot product of float32 vectors against math.fsum of the (exact) float64 products; a fixed reduction tree:
    two calls give equal bits"""
    from xeofs_amd import engine

    rng = np.random.default_rng(count)
    a = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(np.float32)
    b = rng.standard_normal(count).astype(np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)
    da, db = _dev(a), _dev(b)
    got = engine.vec_dot(ctx, da, db)
    assert abs(got - math.fsum(prod)) <= 1e-14 * math.fsum(np.abs(prod))
    assert np.float64(engine.vec_dot(ctx, da, db)).view(np.uint64) == np.float64(got).view(np.uint64)


@pytest.mark.parametrize("rows,L", [(1, 32), (3, 64), (4097, 96), (4805, 256), (40005, 32)])
def test_panel_rownorm(ctx, rows, L):
    from xeofs_amd import engine

    rng = np.random.default_rng(rows + L)
    P = (rng.standard_normal((rows + 2, L)) * 10.0 ** rng.uniform(-3, 3, (rows + 2, 1))).astype(np.float32)
    got = engine.panel_rownorm(ctx, _dev(P), rows)
    ref = np.sqrt((P[:rows].astype(np.float64) ** 2).sum(1))
    assert np.all(np.abs(got - ref) <= 1e-12 * ref)


@pytest.mark.parametrize("L", [32, 64, 96, 160, 256])
@pytest.mark.parametrize("rows", [1, 5, 4099])
def test_panel_gram_edges(ctx, rows, L):
    """eofx_panel_gram_f64 at its edges: fewer rows than one k-step of four, a ragged k-step, 33 row partials with a ragged
    tail; half a 64-column sub-block, one, a ragged second, three, four.  The products of float32 values are exact in
    float64, so only the rows - 1 additions round: |G - P^T P| <= rows 2^-53 |P|^T |P| per element.  G == G^T bit for
    bit (the mirrored stores, the diagonal tiles) and a second call returns the same bits."""
    from xeofs_amd import engine

    rng = np.random.default_rng(1000 * rows + L)
    P = (rng.standard_normal((rows, L)) * 10.0 ** rng.uniform(-2, 2, (1, L))).astype(np.float32)
    dP = _dev(P)
    G = _host(engine.panel_gram(ctx, dP))
    P64 = P.astype(np.float64)
    ref, S = P64.T @ P64, np.abs(P64).T @ np.abs(P64)
    assert np.all(np.abs(G - ref) <= rows * 2.0 ** -53 * S)
    assert np.array_equal(G.view(np.uint64), G.T.view(np.uint64))
    assert np.array_equal(G.view(np.uint64), _host(engine.panel_gram(ctx, dP)).view(np.uint64))


@pytest.mark.parametrize("layout", ["written", "in_place", "masked"])
def test_feature_and_sample_norms(ctx, layout):
    """norms of the rows and columns of the resident matrix in float64; an in-place matrix takes the norms of its samples
    through the Scaler map without building a layout (rownorm_aff_kernel), a masked one skips its zero columns"""
    from xeofs_amd import engine

    n, P = 333, 2332                      # (a multiple of 4: the field can stay in place)
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((n, P)) * (1.0 + 3.0 * rng.random(P)) + np.linspace(-40.0, 250.0, P)).astype(np.float32)
    if layout == "masked":
        X[:, 100:300] = np.nan
        X[:, rng.integers(0, P, 40)] = np.nan
    w = np.linspace(0.2, 1.7, P)
    m2, _ = engine.preprocess(ctx, X, True, True, w)
    D = m2.download().astype(np.float64)
    mat, _ = engine.preprocess(ctx, X, True, True, w, in_place=layout != "written", allow_masked=layout == "masked")
    assert mat.masked == (layout == "masked")
    got = engine.sample_norms(ctx, mat)
    ref = np.sqrt((D ** 2).sum(1))
    assert np.all(np.abs(got - ref) <= 1e-12 * ref)
    if layout != "written":
        assert not mat.has_sample_layout() and mat.layout() == (False, True)
    if layout != "masked":
        got = engine.feature_norms(ctx, mat)
        ref = np.sqrt((D ** 2).sum(0))
        assert got.shape == (mat.p,) and np.all(np.abs(got - ref) <= 1e-12 * ref)
    mat.free()
    m2.free()


def _gram_check(G, A, B, side, d_valid):
    """G [d_pad x d_pad] against A B^T (side 0) or A^T B (side 1) in float64 under 1e-5 * sum|a||b|; padding exact zeros"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = A64.T @ B64 if side else A64 @ B64.T
    bound = 1e-5 * (np.abs(A64).T @ np.abs(B64) if side else np.abs(A64) @ np.abs(B64).T)
    g = _host(G)
    assert np.all(np.abs(g[:d_valid, :d_valid] - ref) <= bound)
    assert not g[d_valid:].any() and not g[:, d_valid:].any()


@pytest.mark.parametrize("n,p", [(300, 1037), (1037, 300), (29, 45)])
def test_cross_gram(ctx, n, p):
    """A_a A_b^T and A_a^T A_b against the float64 products, per element; `a is b`; shapes that differ (the feature counts on
    the sample side included: the entry takes two matrices of one shape) raise"""
    from xeofs_amd import engine

    rng = np.random.default_rng(n + p)
    A = rng.standard_normal((n, p)).astype(np.float32)
    B = (rng.standard_normal((n, p)) * (1.0 + rng.random(p))).astype(np.float32)
    a, b = engine.from_dense(ctx, A), engine.from_dense(ctx, B)
    for side in (0, 1):
        _gram_check(a.cross_gram(b, side), A, B, side, p if side else n)
        _gram_check(a.cross_gram(a, side), A, A, side, p if side else n)
    c = engine.from_dense(ctx, rng.standard_normal((n, p + 5)).astype(np.float32))
    d = engine.from_dense(ctx, rng.standard_normal((n + 1, p)).astype(np.float32))
    for other in (c, d):
        for side in (0, 1):
            with pytest.raises(ValueError):
                a.cross_gram(other, side)
    for m in (a, b, c, d):
        m.free()


def _complex_check(got, Zm, Pc, rows, Am, Bm):
    """got [rows_pad x 2h] = [Re | Im] of Zm @ Pc (complex128) under 1e-5 * sum|a||b| per element, padding exact zeros"""
    ref = Zm @ Pc
    bound = 1e-5 * ((np.abs(Am) + np.abs(Bm)) @ (np.abs(Pc.real) + np.abs(Pc.imag)))
    g = _host(got).astype(np.float64)
    h = Pc.shape[1]
    assert np.all(np.abs(g[:rows, :h] - ref.real) <= bound) and np.all(np.abs(g[:rows, h:] - ref.imag) <= bound)
    assert not g[rows:].any()


@pytest.mark.parametrize("lean", [False, True])
def test_cmat_mul(ctx, lean):
    """one pass of Z = A + iB over a [Re | Im] panel, Z^H W and Z Y, against complex128 element by element, at panel widths
    64 and 128; a written pair and the lean layout (A in place, B as the Hilbert stage leaves it); the `final` flag selects
    the precision of the final passes -- the same by default --, so its result meets the same bound"""
    from xeofs_amd import engine

    n, p = 301, 1036                      # (a multiple of 4: the real part can stay in place)
    rng = np.random.default_rng(11)
    Xa = (rng.standard_normal((n, p)) * (1.0 + rng.random(p))).astype(np.float32)
    if lean:
        A, _ = engine.preprocess(ctx, Xa, True, False, None, in_place=True)
        B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    else:
        A = engine.from_dense(ctx, Xa)
        B = engine.from_dense(ctx, rng.standard_normal((n, p)).astype(np.float32))
    results = []
    for L in (64, 128):
        h = L // 2
        W = rng.standard_normal((n, L)).astype(np.float32)
        Y = rng.standard_normal((p, L)).astype(np.float32)
        Wp, Yp = engine.panel_import(ctx, W, A.n_pad, L), engine.panel_import(ctx, Y, A.p_pad, L)
        if lean and L == 64:
            assert A.layout() == (False, True)
        for final in (False, True):
            results.append((L, True, W[:, :h] + 1j * W[:, h:], engine.cmat_mul(ctx, A, B, Wp, True, final)))
            results.append((L, False, Y[:, :h] + 1j * Y[:, h:], engine.cmat_mul(ctx, A, B, Yp, False, final)))
    if lean:
        m2, _ = engine.preprocess(ctx, Xa, True, False, None)
        Am = m2.download().astype(np.float64)
        m2.free()
    else:
        Am = A.download().astype(np.float64)
    Bm = B.download().astype(np.float64)
    Z = Am + 1j * Bm
    for L, conj_left, Pc, got in results:
        if conj_left:
            _complex_check(got, Z.conj().T, Pc.astype(np.complex128), p, Am.T, Bm.T)
        else:
            _complex_check(got, Z, Pc.astype(np.complex128), n, Am, Bm)
    A.free()
    B.free()


@pytest.mark.parametrize("n", [2, 3, 33, 256, 513])
@pytest.mark.parametrize("padding", ["exp", None])
def test_hilbert_operator(ctx, n, padding):
    """H x for the returned n x n operator is the imaginary part of the oracle's Hilbert transform of x, for random and for
    constant series, to 2e-5 of the series' scale (the tolerance of test_hilbert_stage_vs_oracle)"""
    from xeofs_amd import engine

    H = engine.hilbert_operator(ctx, n, padding, 0.2).astype(np.float64)
    assert H.shape == (n, n)
    rng = np.random.default_rng(n)
    x = np.concatenate([rng.standard_normal((n, 5)), np.full((n, 1), 3.5), np.full((n, 1), -250.0)], axis=1)
    ref = orc.hilbert_transform(x, padding=padding, decay_factor=0.2).imag
    scale = np.abs(x).max(0)
    assert np.all(np.abs(H @ x - ref) <= 2e-5 * scale[None, :])


def _eigh_check(A):
    from xeofs_amd import engine

    n = A.shape[0]
    w, V = engine.host_eigh(A)
    nrm = max(np.linalg.norm(A, 2), 1e-300)
    wr = np.linalg.eigh(A)[0][::-1]
    assert np.all(np.diff(w) <= 0)                                         # the entry's own descending order
    assert np.all(np.abs(w - wr) <= 1e-12 * nrm)
    assert np.linalg.norm(A @ V - V * w[None, :], 2) <= 1e-11 * nrm
    assert np.linalg.norm(V.T @ V - np.eye(n), 2) <= 1e-11


@pytest.mark.parametrize("n", [1, 2, 30, 240])
def test_host_eigh(n):
    """eofx_host_eigh_f64 against numpy.linalg.eigh: eigenvalues to 1e-12 ||A||, residual to 1e-11 ||A||, orthonormality to
    1e-11; a random symmetric matrix, one with a repeated eigenvalue and a diagonal one (host code, run beside the GPU suite)"""
    rng = np.random.default_rng(n)
    S = rng.standard_normal((n, n))
    _eigh_check((S + S.T) * 0.5 * 37.0)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = np.linspace(1.0, 2.0, n)
    lam[: (n + 1) // 2] = 5.0                                              # a repeated eigenvalue
    R = (Q * lam[None, :]) @ Q.T
    _eigh_check((R + R.T) * 0.5)
    _eigh_check(np.diag(rng.standard_normal(n) * 1.0e3))


@pytest.mark.parametrize("rows,l,L", [(1, 1, 32), (3, 5, 32), (4097, 60, 64), (4805, 96, 96), (700, 250, 256)])
def test_panel_import_export(ctx, rows, l, L):
    """import zero-pads a dense [rows x l] array into a NaN-filled [rows_pad x L] panel: the padding rows and columns are
    exact zeros, the body is the source bit for bit; export returns the leading k < l columns, with a sign per column"""
    import torch
    from xeofs_amd import engine
    from xeofs_amd._lib import ptr, raise_for

    rng = np.random.default_rng(rows + l)
    src = rng.standard_normal((rows, l)).astype(np.float32)
    rows_pad = (rows + 511) // 512 * 512
    P = torch.full((rows_pad, L), float("nan"), dtype=torch.float32, device="cuda")
    raise_for(ctx.lib.eofx_panel_import_f32(ctx.handle, ptr(src), rows, l, ptr(P), rows_pad, L), ctx.handle)
    Ph = _host(P)
    assert np.array_equal(Ph[:rows, :l].view(np.uint32), src.view(np.uint32))
    assert not Ph[rows:].any() and not Ph[:, l:].any() and np.isfinite(Ph).all()
    assert np.array_equal(_host(engine.panel_import(ctx, src, rows_pad, L)), Ph)
    assert np.array_equal(engine.panel_export(ctx, P, rows, l), src)                     # round trip
    k = max(1, l - 2)
    sign = np.where(np.arange(k) % 3 == 0, -1.0, 1.0)
    want = src[:, :k] * sign[None, :].astype(np.float32)
    assert np.array_equal(engine.panel_export(ctx, P, rows, k, sign=sign), want)
    assert np.array_equal(_host(engine.panel_export(ctx, P, rows, k, sign=sign, device_out=True)), want)
    assert np.array_equal(engine.panel_export(ctx, P, rows, k), src[:, :k])
