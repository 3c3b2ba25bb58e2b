"""The two streaming products, X^T Z (eofx_panel_tmul_f32) and X Y (eofx_panel_mul_f32), route by route against float64.

Every case follows the same rules:

  reference     the float64 product of the float32 matrix the engine holds: `mat.download()` of a written matrix; for a
                raw, in-place or masked matrix the download of the two-layout matrix preprocessed with the same arguments
                (test_in_place_mode shows it to be bitwise the same matrix)
  bound         per element, tol * sum_k |a_k| |b_k| with the tolerances of tests/test_gpu_parity.py's header: 1e-5 for
                f32 / bf16x6 / f16x3, 4e-5 for bf16x3, 2e-7 for f64
  dirty output  the output tensor is full of NaN before the call (`out=`): a tile the launch plan forgets shows up
  padding       the padding rows of the output are exact zeros afterwards
  size          every matrix is at most 64 MB

Tile decomposition of a panel of L columns (atb_tiles in csrc/eofx_plans.hpp; "P96" is the partial 96-of-128 tile):

    L     f16x3 (XᵀZ, X·Y over a written matrix)   other precisions, in-place X·Y (axb)
    32    32                                         32
    64    64                                         64
    96    P96                                        64 + 32
    128   128                                        64 + 64
    160   128 + 32                                   64 + 64 + 32
    192   128 + 64                                   3 x 64
    224   128 + P96                                  3 x 64 + 32
    256   128 + 128                                  4 x 64
    288   128 + 128 + 32                             4 x 64 + 32

`tiles()` below restates that rule, `atb_splits()` / `axb_splits()` the split-K plans (atb_plan / axb_plan of the same
header): they are used ONLY to choose shapes and to prove (tests/test_product_model_host.py, no GPU needed) that the shape
lists reach S == 1 and S > 1 on every launcher; tests/test_plans_cpu.py compares them with the header itself.
"""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-5, "bf16x6": 1e-5, "f16x3": 1e-5, "bf16x3": 4e-5, "f64": 2e-7}
WIDTHS = [32, 64, 96, 128, 160, 192, 224, 256, 288]
EXPECTED_TILES_F16 = {32: [32], 64: [64], 96: ["P96"], 128: [128], 160: [128, 32], 192: [128, 64], 224: [128, "P96"],
                      256: [128, 128], 288: [128, 128, 32]}
EXPECTED_TILES_NARROW = {32: [32], 64: [64], 96: [64, 32], 128: [64, 64], 160: [64, 64, 32], 192: [64] * 3,
                         224: [64] * 3 + [32], 256: [64] * 4, 288: [64] * 4 + [32]}

# (n, p): rows and columns off every tile size (512, 256, 64, 16) / so small that padding dominates / long and thin /
# one sample slab (K = 32) under many feature tiles
TMUL_SHAPES = [(1037, 2331), (29, 45), (20011, 301), (23, 40010)]
MUL_SHAPES = [(1037, 2331), (29, 45), (301, 20011), (40010, 23)]
ALL_PREC_SHAPE = (1037, 2331)
# in-place X·Y (launch_axb): fewer than 16 feature pairs -> S == 1; a long feature axis under few row tiles -> S > 1
# (a field stays in place when its feature count is a multiple of 4; a masked one when the valid features are at least 0.6
# of all and outnumber the samples)
AXB_SHAPES = [(301, 900), (333, 5000)]

ATB_BM, ATB_KG, AXB_BM, AXB_KG = 512, 32, 256, 64


def _up(a, b):
    return (a + b - 1) // b * b


def tiles(L, prec="f16x3"):
    """column tiles of launch_atb for a panel of L columns (launch_axb: the narrow rule, whatever the precision)"""
    wide = prec == "f16x3" and L >= 96
    out = [128] * (L // 128) if wide else []
    if wide and L - 128 * len(out) == 96:
        out.append("P96")
    rest = L - sum(96 if t == "P96" else t for t in out)
    return out + [64] * (rest // 64) + ([32] if rest % 64 else [])


def atb_splits(M, K, L, wide):
    """S of atb_plan(M, K, L, wide): C [M x L] = A[K x M]^T B[K x L], M a multiple of 512, K of 32"""
    bx, bz = M // ATB_BM, (L + 127) // 128 if wide else (L + 63) // 64
    resident = 256.0 if wide else 512.0
    best, best_t = 1, 1e30
    for S in range(1, 129):
        kps = _up((K + S - 1) // S, ATB_KG)
        if (K + kps - 1) // kps != S:
            continue
        t = math.ceil(bx * bz * S / resident) * kps * 2048.0 / 1.0e10
        if S > 1:
            t += (2.0 * S + 1.0) * M * L * 4.0 / 4.0e12
        if t < best_t * 0.98:
            best, best_t = S, t
    return best


def axb_splits(rows_pad, K):
    """S of axb_plan(rows_pad, K): the in-place X·Y, rows_pad a multiple of 256, K of 64"""
    rt, units = rows_pad // AXB_BM, K // AXB_KG
    if rt >= 1024 or units < 16:
        return 1
    best, best_t = 1, 1e30
    for s8 in range(1, 33):
        S = 8 * s8
        if S > units:
            break
        kps = (units + S - 1) // S * AXB_KG
        s_eff = (K + kps - 1) // kps
        if s_eff > S or s_eff <= S - 8:
            continue
        t = math.ceil(rt * s8 / 64.0) * kps * 1024.0 / 1.25e10 + (2.0 * s_eff + 1.0) * rows_pad * 64.0 * 4.0 / 4.0e12
        if t < best_t * 0.98:
            best, best_t = s_eff, t
    return best


def tmul_splits(n, p, L, prec="f16x3"):
    return atb_splits(_up(p, ATB_BM), _up(n, ATB_KG), L, prec == "f16x3" and L >= 96)


def mul_splits(n, p, L, prec="f16x3"):
    return atb_splits(_up(n, ATB_BM), _up(p, ATB_KG), L, prec == "f16x3" and L >= 96)


def in_place_mul_splits(n, p):
    return axb_splits(_up(n, ATB_BM), _up(p, AXB_KG))


SPREADS = ("panel", "a_cols", "a_rows")


def spread_operands(K, M, L, d, which, seed=0):
    """A [K x M], B [K x L] float32 of N(0,1) entries with magnitudes spread over d decades: `which` == "panel": column j of
    B times 10^(-d j / (L - 1)); "a_cols": column i of A times 10^(-d i / (M - 1)) (the features of X in X^T Z); "a_rows":
    row k of A times 10^(-d k / (K - 1)) (the features of X in X Y, where they are the summation index).
    The generator of the host model test and of the GPU test."""
    rng = np.random.default_rng(1000 * seed + 10 * d + SPREADS.index(which))
    A = rng.standard_normal((K, M))
    B = rng.standard_normal((K, L))
    if which == "panel":
        B *= 10.0 ** (-d * np.arange(L) / (L - 1))
    elif which == "a_cols":
        A *= 10.0 ** (-d * np.arange(M) / (M - 1))
    else:
        A *= 10.0 ** (-d * np.arange(K) / (K - 1))[:, None]
    return A.astype(np.float32), B.astype(np.float32)


def product_bounds(A, B, tol):
    """(float64 A^T B, tol * sum |a||b|, the absolute term of the split-fp16 model) for A [K x M], B [K x L].
    Absolute term (the header of atb_f16 in csrc/eofx_kernels.hpp): the scaled maximum lies in (2^13, 2^14] and the fp16
    subnormal spacing is 2^-24, so an element of A carries an error of at most 2^-25 * 2^-13 * max|A| = 2^-38 max|A|
    (likewise B): |err| <= 2^-38 (max|A| sum_k |b_k| + max|B| sum_k |a_k|)."""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = A64.T @ B64
    rel = tol * (np.abs(A64).T @ np.abs(B64))
    absb = 2.0 ** -38 * (np.abs(A64).max() * np.abs(B64).sum(0)[None, :] + np.abs(B64).max() * np.abs(A64).sum(0)[:, None])
    return ref, rel, absb


# ----------------------------------------------------------------------------------------------------------------------
def _nan_out(rows, L):
    import torch

    return torch.full((rows, L), float("nan"), dtype=torch.float32, device="cuda")


def _panel(ctx, H, rows_pad):
    """zero-padded device panel of the host array H"""
    from xeofs_amd import engine

    return engine.panel_import(ctx, H, rows_pad, H.shape[1])


def _check(got, ref, bound, rows, what):
    """got [rows_pad x L] (device) against ref [rows x L] within bound, padding rows exact zeros, nothing left unwritten"""
    import torch

    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.isfinite(g).all(), f"{what}: {np.count_nonzero(~np.isfinite(g))} elements unwritten or not finite"
    err = np.abs(g[:rows].astype(np.float64) - ref)
    ratio = float((err / (bound + 1e-300)).max())
    print(f"{what}: worst error / bound = {ratio:.3g}")
    bad = np.argwhere(err > bound + 1e-300)
    assert bad.size == 0, f"{what}: {len(bad)} elements outside the bound, first at {bad[0]}, worst ratio {ratio:.3g}"
    assert not g[rows:].any(), f"{what}: padding rows are not exact zeros"


def _both_products(ctx, mat, Xh, Z, Y, prec, what, tol=None, abs_term=False):
    """X^T Z and X Y of the resident matrix against the float64 products of Xh (what the engine holds)"""
    from xeofs_amd import engine

    tol = TOL[prec] if tol is None else tol
    n, p = Xh.shape
    if Z is not None:
        ref, rel, absb = product_bounds(Xh, Z, tol)
        got = engine.panel_tmul(ctx, mat, _panel(ctx, Z, mat.n_pad), out=_nan_out(mat.p_pad, Z.shape[1]), prec=prec)
        _check(got, ref, rel + absb if abs_term else rel, p, f"{what} XtZ L={Z.shape[1]} {prec}")
    if Y is not None:
        ref, rel, absb = product_bounds(np.ascontiguousarray(Xh.T), Y, tol)
        got = engine.panel_mul(ctx, mat, _panel(ctx, Y, mat.p_pad), out=_nan_out(mat.n_pad, Y.shape[1]), prec=prec)
        _check(got, ref, rel + absb if abs_term else rel, n, f"{what} XY L={Y.shape[1]} {prec}")


_CASES = ([("tmul",) + ALL_PREC_SHAPE + (pr,) for pr in TOL] + [("tmul",) + s + ("f16x3",) for s in TMUL_SHAPES[1:]]
          + [("mul",) + ALL_PREC_SHAPE + (pr,) for pr in TOL] + [("mul",) + s + ("f16x3",) for s in MUL_SHAPES[1:]])


@pytest.mark.parametrize("L", WIDTHS)
@pytest.mark.parametrize("product,n,p,prec", _CASES)
def test_every_tile_decomposition(ctx, product, n, p, prec, L):
    """a written matrix at every panel width of the table in the module docstring, every precision on one shape and the
    default precision on all of them (the shapes reach S == 1 and S > 1: tests/test_product_model_host.py)"""
    from xeofs_amd import engine

    assert tiles(L, "f16x3") == EXPECTED_TILES_F16[L] and tiles(L, "f32") == EXPECTED_TILES_NARROW[L]
    rng = np.random.default_rng(n + p + L)
    X = rng.standard_normal((n, p)).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    assert (mat.n_pad, mat.p_pad) == (_up(n, ATB_BM), _up(p, ATB_BM))
    Z = rng.standard_normal((n, L)).astype(np.float32) if product == "tmul" else None
    Y = rng.standard_normal((p, L)).astype(np.float32) if product == "mul" else None
    _both_products(ctx, mat, X, Z, Y, prec, f"written {n}x{p}")
    mat.free()


# ----------------------------------------------------------------------------------------------------------------------
def _layout_field(n, P, masked, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, P)) * (1.0 + 3.0 * rng.random(P)) + np.linspace(-40.0, 250.0, P)).astype(np.float32)
    if masked:      # whole 64-feature pairs without a valid feature, ragged edges, isolated points
        land = np.zeros(P, bool)
        land[130:330] = True
        land[P - 70:P - 3] = True
        land[rng.integers(0, P, 30)] = True
        X[:, land] = np.nan
    return X, np.linspace(0.2, 1.7, P)


@pytest.mark.parametrize("n,P", AXB_SHAPES)
@pytest.mark.parametrize("layout", ["written", "raw", "in_place", "in_place_dma", "masked", "masked_dma"])
def test_every_layout(monkeypatch, layout, n, P):
    """the same matrix held as a written two-layout matrix, a raw one (X^T Z by the AFF kernel), in place (X^T Z by AFF,
    X Y by axb_f16_kernel or the LDS-DMA kernel) and masked in place (AFF + MASK, the active-pair list): every element of
    both products against float64.  Widths 32, 64 and 96 stay on the in-place kernels (EOFX_NO_WIDE_XT), 160 columns take the
    default rule afterwards (an unmasked in-place matrix then builds its sample-contiguous layout).
    Masked matrix: the rows of X^T Z at masked features are exact zeros; X Y does not pick up what the panel holds at the
    masked rows -- a second call with N(0,1) values there stays inside the same bound against the same reference.  Equal
    bits are NOT required of that second call: the panel maximum that sets the fp16 scale is taken over all rows."""
    import torch
    from xeofs_amd import engine

    masked, dma = layout.startswith("masked"), layout.endswith("_dma")
    monkeypatch.setenv("EOFX_AXB_DMA", "1" if dma else "0")
    monkeypatch.setenv("EOFX_NO_WIDE_XT", "1")
    c = engine.Context(0)                 # the switches are read by a context at its first in-place product
    X, w = _layout_field(n, P, masked, seed=n + P)
    opts = dict(keep_raw=layout == "raw", in_place=layout not in ("written", "raw"), allow_masked=masked)
    m2, st2 = engine.preprocess(c, X, True, True, w)
    mat, st = engine.preprocess(c, X, True, True, w, **opts)
    assert mat.masked == masked
    if layout != "written":
        assert mat.layout() == (False, True)
    valid = st2["valid_feature"]
    Xh = np.zeros((n, P), np.float32)     # the engine's matrix over the PHYSICAL columns: zeros at the masked features
    Xh[:, valid] = m2.download()
    if not masked:
        assert valid.all()
    rng = np.random.default_rng(7)
    for L in (32, 64, 96, 160):
        if L == 160:
            monkeypatch.delenv("EOFX_NO_WIDE_XT")
        Z = rng.standard_normal((n, L)).astype(np.float32)
        Y = rng.standard_normal((P, L)).astype(np.float32)
        Y[~valid] = 0.0
        if masked:
            _both_products(c, mat, Xh, Z, Y, "f16x3", layout)
            got = engine.panel_tmul(c, mat, _panel(c, Z, mat.n_pad), out=_nan_out(mat.p_pad, L), prec="f16x3")
            torch.cuda.synchronize()
            assert not got.cpu().numpy()[:P][~valid].any(), "X^T Z is not an exact zero at a masked feature"
            Y2 = Y.copy()
            Y2[~valid] = rng.standard_normal((int((~valid).sum()), L)).astype(np.float32)
            ref, rel, _ = product_bounds(np.ascontiguousarray(Xh.T), Y, TOL["f16x3"])
            got = engine.panel_mul(c, mat, _panel(c, Y2, mat.p_pad), out=_nan_out(mat.n_pad, L), prec="f16x3")
            _check(got, ref, rel, n, f"{layout} XY L={L} with values at the masked rows")
        else:
            _both_products(c, mat, Xh, Z, Y, "f16x3", layout)
        if L < 160 and layout not in ("written", "raw"):
            assert not mat.has_sample_layout()          # still streaming the field where it lies
    mat.free()
    m2.free()


# ----------------------------------------------------------------------------------------------------------------------
_POW = [-40, -12, 0, 12, 40]


def _bits(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("layout,L", [("written", 96), ("written", 160), ("in_place", 64), ("in_place", 32)])
def test_power_of_two_covariance(monkeypatch, layout, L):
    """f16x3: the scales are exact powers of two and the split works on the scaled value, so X * 2^a and a panel * 2^b give
    the SAME BITS times 2^(a + b), on both products -- written matrices and an in-place matrix whose map is the identity
    (center=False, no standardisation, no weights).  Inputs of order 1: nothing leaves the float32 normal range."""
    from xeofs_amd import engine

    monkeypatch.setenv("EOFX_NO_WIDE_XT", "1")
    monkeypatch.setenv("EOFX_AXB_DMA", "0")
    c = engine.Context(0)
    n, p = 333, 2100
    rng = np.random.default_rng(L)
    X = rng.uniform(0.25, 2.0, (n, p)).astype(np.float32) * rng.choice([-1.0, 1.0], (n, p)).astype(np.float32)
    Z = rng.uniform(0.25, 2.0, (n, L)).astype(np.float32) * rng.choice([-1.0, 1.0], (n, L)).astype(np.float32)
    Y = rng.uniform(0.25, 2.0, (p, L)).astype(np.float32) * rng.choice([-1.0, 1.0], (p, L)).astype(np.float32)
    base = {}
    for a in [0] + [e for e in _POW if e]:
        Xa = (X * np.float32(2.0 ** a)).astype(np.float32)
        if layout == "written":
            mat = engine.from_dense(c, Xa)
        else:
            mat, _ = engine.preprocess(c, Xa, False, False, None, in_place=True)
            assert mat.layout() == (False, True)
        if layout == "written":
            assert np.array_equal(mat.download(), Xa)
        for b in [0] + [e for e in _POW if e]:
            s = np.float32(2.0 ** b)
            T = _bits(engine.panel_tmul(c, mat, _panel(c, Z * s, mat.n_pad), out=_nan_out(mat.p_pad, L), prec="f16x3"))
            W = _bits(engine.panel_mul(c, mat, _panel(c, Y * s, mat.p_pad), out=_nan_out(mat.n_pad, L), prec="f16x3"))
            if (a, b) == (0, 0):
                base = dict(T=T, W=W)
                assert np.isfinite(T).all() and np.isfinite(W).all() and T[:p].any() and W[:n].any()
                continue
            f = np.float32(2.0 ** (a + b))
            assert np.array_equal(T, base["T"] * f), (layout, "XtZ", a, b)
            assert np.array_equal(W, base["W"] * f), (layout, "XY", a, b)
        if layout != "written":
            assert not mat.has_sample_layout()
        mat.free()


# ----------------------------------------------------------------------------------------------------------------------
SPREAD_SHAPE = (700, 1100)      # (n, p)
SPREAD_L = 64


@pytest.mark.parametrize("which", ["panel", "field"])
@pytest.mark.parametrize("product", ["tmul", "mul"])
@pytest.mark.parametrize("d,prec", [(0, "f16x3"), (2, "f16x3"), (4, "f16x3"), (8, "f16x3"), (8, "f32"), (8, "f64")])
def test_dynamic_range_inside_one_operand(ctx, d, prec, product, which):
    """magnitudes spread over d decades across the panel's columns ("panel") or across the features of X ("field").
    d <= 4: the plain relative bound holds unchanged.  d = 8 under f16x3: elements far below the operand maximum carry an
    ABSOLUTE error, so the bound gains the term of `product_bounds` (tests/test_product_model_host.py shows that the
    split alone needs it at d = 8 and not at d <= 4).  The f32 and f64 kernels have no such limit: plain bound at d = 8."""
    from xeofs_amd import engine

    n, p = SPREAD_SHAPE
    K, M = (n, p) if product == "tmul" else (p, n)
    spread = "panel" if which == "panel" else "a_cols" if product == "tmul" else "a_rows"     # "field": the features of X
    A, B = spread_operands(K, M, SPREAD_L, d, spread, seed=1 + (product == "mul"))
    X = A if product == "tmul" else np.ascontiguousarray(A.T)
    mat = engine.from_dense(ctx, X)
    assert np.array_equal(mat.download(), X)
    _both_products(ctx, mat, X, B if product == "tmul" else None, B if product == "mul" else None, prec,
                   f"spread d={d} {which}", abs_term=(prec == "f16x3" and d == 8))
    mat.free()
