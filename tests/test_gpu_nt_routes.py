"""Every route through the fp16 NT matrix-core kernel (xeofs_amd/csrc/eofx_gram.hpp: planes_split_kernel / planes_split_t_kernel
-> gram_nt_kernel -> gram_finish_kernel / nt_finish_kernel) against float64, per element:

  fast Gram    G = X' X'^T                 ResidentMatrix.gram(0)    (eofx_mat_gram_f32 -> mat_gram_fast, p >= n)
  wide XᵀZ     Yp = X'^T Zn, L >= 512      engine.panel_tmul         (eofx_panel_tmul_f32 -> mat_tmul_nt, n >= 512)
  wide P·M     out = P M, L >= 512         engine.panel_matmul       (eofx_panel_matmul_f32 -> launch_matmul_nt, rows >= 1024)

The rules are those of tests/test_gpu_product_routes.py, whose helpers this module imports:

  reference     the float64 product of the float32 matrix the engine holds: the download of a written matrix; for a raw, in-place
                or masked matrix the download of the two-layout matrix preprocessed with the same arguments, zeros at the masked
                features; for P·M the float64 matrix rounded to float32 first, as the engine rounds it
  bound         per element, TOL["f16x3"] * sum_k |a_k| |b_k|, plus the 2^-38 absolute term of `product_bounds` when magnitudes
                spread over 8 decades across rows or columns
  dirty output  the output is full of NaN before the call; nothing may stay unwritten, padding rows and columns are exact zeros
  exact cases   integer operands in [-16, 16]: the scaled hi plane is exact, the lo plane zero and every float32 partial sum an
                integer below 2^24 times a power of two, so the result equals the integer product bit for bit whatever the split

`gram_plan()` restates gram_plan_build of csrc/eofx_plans.hpp (split-K rule, per-XCD deal): it is used ONLY to choose shapes
and to prove (tests/test_nt_model_host.py, no GPU needed) that the shape lists reach the plan edges named next to them;
tests/test_gram_plan_cpu.py compares it with the header itself.

What the routes' predicates leave unreachable: a field that is off a 16-byte boundary or whose feature count is no multiple of
four is never read where it lies (apply_plan writes the layouts instead), so planes_split_kernel and planes_split_t_kernel see an
unaligned source or leading dimension only through a probe; their scalar path is reached at the ragged last group of 8 (4)
features of a row -- with the Scaler map on an in-place field of 1100 features, without it on a written one of 1037 or 1100.
"""

import numpy as np
import pytest

import test_gpu_product_routes as routes
from test_gpu_product_routes import TOL, _check, _layout_field, _nan_out, _panel, _up, product_bounds, spread_operands

pytestmark = pytest.mark.gpu

GR_BM, GR_BK = 256, 32

# (n, p), p >= n (the fast route's condition)                    T   S   edge
GRAM_SHAPES = [(29, 45), (40, 64),      # 3   1   nst = 2, the shortest legal loop; 5 of the 8 XCD lanes hold empty items
               (40, 65),                # 3   1   nst = 4
               (300, 1037),             # 3   3   last split 10 of 12; p off 4, 8 and 32
               (513, 1100),             # 10  3   cmax = 2, T % 8 != 0
               (1100, 1440),            # 21  4   last split 10 of 12
               (1537, 1600),            # 36  5   cmax = 5
               (300, 4100)]             # 3   5   26-stage splits
# (n, p, L), n >= 512, L >= 512 a multiple of 32
TMUL_SHAPES = [(512, 300, 512),         # S = 2: the smallest legal shape
               (513, 1037, 544),
               (700, 3000, 512),        # S = 3, last split 6 of 8
               (577, 257, 768),         # Lp == L
               (1037, 2331, 544)]       # Lp = 768: nt_finish_kernel discards a partial column tile
# (rows, L, Lo), rows >= 1024 a multiple of 256, L >= 512, Lo >= 256, both multiples of 4
MATMUL_SHAPES = [(1024, 512, 256),      # S = 2: the smallest legal shape
                 (1024, 516, 260),      # S = 3; kpad = 576: the last 8-feature group leaves the vector path; Lo off 256
                 (1280, 1536, 1504),
                 (1024, 580, 772)]
LAYOUT_SHAPE = (577, 1100, 512)         # one field for the Gram matrix and the wide XᵀZ of test_every_source
ODD_SHAPE = (577, 1037, 512)            # ... and one whose feature count is off 4
LAYOUTS = ["written", "raw", "in_place", "masked", "misaligned", "odd"]
EXACT_GRAM = [(300, 1037), (513, 1100)]
EXACT_TMUL = (700, 3000, 512)
EXACT_MATMUL = (1024, 516, 260)
SPLITS = [None, 1, 2, 5, 16]            # EOFX_GRAM_SPLITS
POW = [-40, -12, 12, 40]
SPREAD_D = [0, 4, 8]
SPREAD_GRAM = (1100, 300)               # (K, M) of spread_operands: X = A^T is 300 x 1100
SPREAD_TMUL = (600, 700, 512)           # (K, M, L): X is 600 x 700, the panel 600 x 512
SPREAD_MATMUL = (512, 1024, 256)        # (K, M, L): P = A^T is 1024 x 512, the matrix 512 x 256
SPREAD_SEED = 3


def gram_plan(nti, ntj, sym, nst_total, S=0):
    """gram_plan_build (csrc/eofx_plans.hpp) without the lists: tiles T, largest per-XCD patch cmax, splits S of st_per_split
    stages (the last one `last`), workgroups grid.  S <= 0: the plan's own choice."""
    T = sum(max(0, ntj - i) for i in range(nti)) if sym else nti * ntj
    lo = [T * x // 8 for x in range(9)]
    cmax = max(lo[x + 1] - lo[x] for x in range(8))
    if S <= 0:
        best = 1e300
        for s in range(1, min(16, nst_total) + 1):
            sps = ((nst_total + s - 1) // s + 1) // 2 * 2
            if (nst_total + sps - 1) // sps != s:
                continue
            cost = float((cmax * s + 31) // 32) * (sps + 40.0) + 2.0 * s
            if cost < best * 0.97:
                best, S = cost, s
    sps = ((nst_total + S - 1) // S + 1) // 2 * 2
    S = (nst_total + sps - 1) // sps
    return dict(T=T, cmax=cmax, S=S, st_per_split=sps, last=nst_total - (S - 1) * sps, grid=8 * cmax * S, nst_total=nst_total)


def gram_shape_plan(n, p, S=0):
    nt = _up(n, routes.ATB_BM) // GR_BM
    return gram_plan(nt, nt, True, _up(p, 2 * GR_BK) // GR_BK, S)


def tmul_shape_plan(n, p, L, S=0):
    return gram_plan(_up(p, routes.ATB_BM) // GR_BM, _up(L, GR_BM) // GR_BM, False, _up(n, 2 * GR_BK) // GR_BK, S)


def matmul_shape_plan(rows, L, Lo, S=0):
    return gram_plan(rows // GR_BM, _up(Lo, GR_BM) // GR_BM, False, _up(L, 2 * GR_BK) // GR_BK, S)


def layout_inputs(layout):
    """(field, weights) of test_every_source: the generator of the host test and of the GPU test"""
    n, P, _ = ODD_SHAPE if layout == "odd" else LAYOUT_SHAPE
    return _layout_field(n, P, layout == "masked", seed=n + P)


def int_operands(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-16, 17, shape).astype(np.float32)


def census_field(n, p):
    """feature k is 1 in row k mod n and 0 elsewhere: G = diag(number of features of row i)"""
    X = np.zeros((n, p), np.float32)
    X[np.arange(p) % n, np.arange(p)] = 1.0
    return X


def position_coded(n, p):
    """integers in [-16, 16] that tell the position: X[r, k] = (7 r + 13 k) mod 33 - 16"""
    return ((7 * np.arange(n)[:, None] + 13 * np.arange(p)[None, :]) % 33 - 16).astype(np.float32)


def corner_rows(n):
    """first and last rows of the 64-row sub-blocks, of the 256-row tiles and of the matrix"""
    return sorted({0, 63, 64, 127, 128, 255, 256, 511, n - 1})


def spread_inputs(route, d, which):
    K, M, L = {"gram": SPREAD_GRAM + (32,), "tmul": SPREAD_TMUL, "matmul": SPREAD_MATMUL}[route]
    A, B = spread_operands(K, M, L, d, which, seed=SPREAD_SEED)
    return (A, A) if route == "gram" else (A, B)


# ----------------------------------------------------------------------------------------------------------------------
RATIOS = {}


def _note(route, got, ref, bound, rows):
    """largest error / bound seen per route (printed with every case, summed up by test_print_worst_ratios)"""
    g = got[:rows, :ref.shape[1]].double().cpu().numpy()
    r = float((np.abs(g - ref) / (bound + 1e-300)).max())
    RATIOS[route] = max(RATIOS.get(route, 0.0), r)


def _check2(got, ref, bound, what, route=None):
    """got [rows_pad x cols_pad] against ref [rows x cols]: `_check` on the leading columns, then the padding columns"""
    import torch

    rows, cols = ref.shape
    _check(got[:, :cols], ref, bound, rows, what)
    torch.cuda.synchronize()
    assert not got[:, cols:].cpu().numpy().any(), f"{what}: padding columns are not exact zeros"
    if route:
        _note(route, got, ref, bound, rows)


def _gram(mat):
    return mat.gram(0, out=_nan_out(mat.n_pad, mat.n_pad))


def _check_gram(mat, Xh, what, abs_term=False, route="gram"):
    """G of the resident matrix against the float64 Gram matrix of Xh [n x p]; -> G as a host array"""
    A = np.ascontiguousarray(Xh.T)
    ref, rel, absb = product_bounds(A, A, TOL["f16x3"])
    G = _gram(mat)
    _check2(G, ref, rel + absb if abs_term else rel, what, route)
    return G.cpu().numpy()


def _check_tmul(ctx, mat, Xh, Z, what, abs_term=False, route="tmul"):
    from xeofs_amd import engine

    ref, rel, absb = product_bounds(Xh, Z, TOL["f16x3"])
    got = engine.panel_tmul(ctx, mat, _panel(ctx, Z, mat.n_pad), out=_nan_out(mat.p_pad, Z.shape[1]), prec="f16x3")
    _check2(got, ref, rel + absb if abs_term else rel, what, route)
    return got


def _matmul(ctx, P, M64):
    """P [rows x L] float32, M64 [L x Lo] float64 (host) -> the device result over a NaN-filled output"""
    import torch
    from xeofs_amd import engine

    Pd, Md = torch.from_numpy(np.ascontiguousarray(P)).cuda(), torch.from_numpy(np.ascontiguousarray(M64)).cuda()
    return engine.panel_matmul(ctx, Pd, Md, out=_nan_out(P.shape[0], M64.shape[1]))


def _check_matmul(ctx, P, M64, what, abs_term=False, route="matmul"):
    ref, rel, absb = product_bounds(np.ascontiguousarray(P.T), M64.astype(np.float32), TOL["f16x3"])
    got = _matmul(ctx, P, M64)
    _check2(got, ref, rel + absb if abs_term else rel, what, route)
    return got


def _bits(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# 1. every shape, per element
@pytest.mark.parametrize("n,p", GRAM_SHAPES)
def test_gram_every_shape(ctx, n, p):
    """N(0, 1) field, written matrix: every element inside the bound, G == G^T bit for bit, a second call gives the same bits"""
    from xeofs_amd import engine

    X = np.random.default_rng(n + p).standard_normal((n, p)).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    assert mat.n_pad == _up(n, routes.ATB_BM) and np.array_equal(mat.download(), X)
    G = _check_gram(mat, X, f"gram {n}x{p}")
    assert np.array_equal(G, G.T), "G is not symmetric bit for bit"
    assert np.array_equal(_bits(_gram(mat)), G), "a second call gives other bits"
    mat.free()


@pytest.mark.parametrize("n,p,L", TMUL_SHAPES)
def test_wide_tmul_every_shape(ctx, n, p, L):
    from xeofs_amd import engine

    rng = np.random.default_rng(n + p + L)
    X = rng.standard_normal((n, p)).astype(np.float32)
    Z = (rng.standard_normal((n, L)) * (1.0 + rng.random(L))).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    assert mat.p_pad == _up(p, routes.ATB_BM) and np.array_equal(mat.download(), X)
    _check_tmul(ctx, mat, X, Z, f"tmul {n}x{p} L={L}")
    mat.free()


@pytest.mark.parametrize("rows,L,Lo", MATMUL_SHAPES)
def test_wide_matmul_every_shape(ctx, rows, L, Lo):
    rng = np.random.default_rng(rows + L + Lo)
    P = rng.standard_normal((rows, L)).astype(np.float32)
    M = rng.standard_normal((L, Lo))
    _check_matmul(ctx, P, M, f"matmul {rows}x{L} Lo={Lo}")


# ----------------------------------------------------------------------------------------------------------------------
# 2. every source of planes_split_kernel and planes_split_t_kernel
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_source(ctx, layout):
    """the same centred, standardised and weighted field held as written layouts, raw, in place, masked in place (NaN at whole
    64-feature runs, ragged ends and isolated points), handed in 4 bytes off a 16-byte boundary, and with a feature count off 4
    (the engine writes the layouts of the last two: see the module docstring).  Gram matrix and wide XᵀZ against float64 of the
    two-layout matrix with zeros at the masked features; there the rows of XᵀZ are exact zeros."""
    import torch
    from xeofs_amd import engine

    n, P, L = ODD_SHAPE if layout == "odd" else LAYOUT_SHAPE
    X, w = layout_inputs(layout)
    masked = layout == "masked"
    m2, st2 = engine.preprocess(ctx, X, True, True, w)
    valid = st2["valid_feature"]
    assert valid.all() != masked
    Xh = np.zeros((n, P), np.float32)
    Xh[:, valid] = m2.download()
    m2.free()
    src = X
    if layout == "misaligned":
        buf = torch.empty(X.size + 1, dtype=torch.float32, device="cuda")
        src = buf[1:].view(X.shape)
        src.copy_(torch.from_numpy(X))
        assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    mat, _ = engine.preprocess(ctx, src, True, True, w, keep_raw=layout == "raw", in_place=layout not in ("written", "raw"),
                               allow_masked=masked)
    assert mat.masked == masked
    assert mat.layout() == ((True, False) if layout in ("written", "misaligned", "odd") else (False, True))
    G = _check_gram(mat, Xh, f"{layout} gram", route="gram_layouts")
    assert np.array_equal(G, G.T)
    Z = np.random.default_rng(7).standard_normal((n, L)).astype(np.float32)
    got = _check_tmul(ctx, mat, Xh, Z, f"{layout} tmul", route="tmul_layouts")
    if masked:
        assert not _bits(got)[:P][~valid].any(), "X^T Z is not an exact zero at a masked feature"
    mat.free()


# ----------------------------------------------------------------------------------------------------------------------
# 3. exact operands, bit for bit, at every split count
def _exact_gram(mat, X, what):
    want = (X.astype(np.float64) @ X.astype(np.float64).T)
    assert np.abs(want).max() < 2 ** 24
    G = _bits(_gram(mat))
    n = X.shape[0]
    bad = np.argwhere(G[:n, :n] != want)          # (NaN compares unequal: an unwritten element counts)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ from the integer product, first at {bad[0]}"
    assert not G[n:].any() and not G[:, n:].any(), f"{what}: padding is not exact zeros"


@pytest.mark.parametrize("splits", SPLITS)
def test_exact_operands_at_every_split(monkeypatch, splits):
    """integers in [-16, 16] (see the module docstring) on written matrices and on an in-place matrix with the identity map;
    the stage census (a dropped, doubled or misplaced 32-feature stage, 16-byte chunk or k-step is a wrong integer on the
    diagonal) and the tile corners (rows 0, 63 | 64, ..., 255 | 256, 511, n - 1 of a position-coded field alone hold data, then the
    whole field: the first and last rows of the
    sub-blocks that straddle the diagonal of a diagonal tile, where only the upper triangle is used, land where they belong and
    nothing lands elsewhere).  A fresh context per split count: a context caches its work lists by shape."""
    from xeofs_amd import engine

    if splits is None:
        monkeypatch.delenv("EOFX_GRAM_SPLITS", raising=False)
    else:
        monkeypatch.setenv("EOFX_GRAM_SPLITS", str(splits))
    c = engine.Context(0)
    for n, p in EXACT_GRAM:
        X = int_operands((n, p), n + p)
        mat = engine.from_dense(c, X)
        _exact_gram(mat, X, f"S={splits} written gram {n}x{p}")
        mat.free()
        C = census_field(n, p)
        mat = engine.from_dense(c, C)
        assert np.array_equal(np.diag(np.bincount(np.arange(p) % n, minlength=n)).astype(np.float64), C.astype(np.float64) @ C.T)
        _exact_gram(mat, C, f"S={splits} census {n}x{p}")
        mat.free()
    n, p = EXACT_GRAM[1]
    X = int_operands((n, p), 5)
    mat, _ = engine.preprocess(c, X, False, False, None, in_place=True)
    assert mat.layout() == (False, True)
    _exact_gram(mat, X, f"S={splits} in-place gram {n}x{p}")
    mat.free()
    Xc = np.zeros((n, p), np.float32)
    Xc[corner_rows(n)] = position_coded(n, p)[corner_rows(n)]
    for what, Xe in (("tile corners", Xc), ("position-coded", position_coded(n, p))):
        mat = engine.from_dense(c, Xe)
        _exact_gram(mat, Xe, f"S={splits} {what} {n}x{p}")
        mat.free()

    n, p, L = EXACT_TMUL
    X, Z = int_operands((n, p), 11), int_operands((n, L), 12)
    want = X.astype(np.float64).T @ Z.astype(np.float64)
    assert np.abs(want).max() < 2 ** 24
    for layout in ("written", "in_place"):
        mat = engine.from_dense(c, X) if layout == "written" else engine.preprocess(c, X, False, False, None, in_place=True)[0]
        assert mat.layout() == ((True, False) if layout == "written" else (False, True))
        got = _bits(engine.panel_tmul(c, mat, _panel(c, Z, mat.n_pad), out=_nan_out(mat.p_pad, L), prec="f16x3"))
        assert np.array_equal(got[:p], want) and not got[p:].any(), f"S={splits} {layout} tmul"
        mat.free()

    rows, L, Lo = EXACT_MATMUL
    P, M = int_operands((rows, L), 13), int_operands((L, Lo), 14).astype(np.float64)
    want = P.astype(np.float64) @ M
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(_bits(_matmul(c, P, M)), want), f"S={splits} matmul"


# ----------------------------------------------------------------------------------------------------------------------
# 4. power-of-two covariance
def _signed_uniform(rng, shape):
    return rng.uniform(0.25, 2.0, shape).astype(np.float32) * rng.choice([-1.0, 1.0], shape).astype(np.float32)


@pytest.mark.parametrize("layout", ["written", "in_place"])
def test_power_of_two_covariance_field_routes(ctx, layout):
    """X * 2^a and a panel * 2^b give the SAME BITS times 2^(2a) (Gram matrix) and 2^(a + b) (wide XᵀZ): the scales are exact
    powers of two and the split works on the scaled value.  Inputs of order 1: nothing leaves the float32 normal range."""
    from xeofs_amd import engine

    n, p, L = LAYOUT_SHAPE
    rng = np.random.default_rng(L)
    X, Z = _signed_uniform(rng, (n, p)), _signed_uniform(rng, (n, L))
    base = {}
    for a in [0] + POW:
        Xa = (X * np.float32(2.0 ** a)).astype(np.float32)
        if layout == "written":
            mat = engine.from_dense(ctx, Xa)
            assert np.array_equal(mat.download(), Xa)
        else:
            mat, _ = engine.preprocess(ctx, Xa, False, False, None, in_place=True)
            assert mat.layout() == (False, True)
        G = _bits(_gram(mat))
        if a == 0:
            base["G"] = G
            assert np.isfinite(G).all() and G[:n, :n].all()
        else:
            assert np.array_equal(G, base["G"] * np.float32(2.0 ** (2 * a))), (layout, "gram", a)
        for b in [0] + POW:
            Zb = (Z * np.float32(2.0 ** b)).astype(np.float32)
            T = _bits(engine.panel_tmul(ctx, mat, _panel(ctx, Zb, mat.n_pad), out=_nan_out(mat.p_pad, L), prec="f16x3"))
            if (a, b) == (0, 0):
                base["T"] = T
                assert np.isfinite(T).all() and T[:p].all()
            else:
                assert np.array_equal(T, base["T"] * np.float32(2.0 ** (a + b))), (layout, "tmul", a, b)
        mat.free()


def test_power_of_two_covariance_matmul(ctx):
    rows, L, Lo = EXACT_MATMUL
    rng = np.random.default_rng(Lo)
    P, M = _signed_uniform(rng, (rows, L)), _signed_uniform(rng, (L, Lo)).astype(np.float64)
    base = _bits(_matmul(ctx, P, M))
    assert np.isfinite(base).all() and base.all()
    for a in [0] + POW:
        for b in [0] + POW:
            if (a, b) != (0, 0):
                got = _bits(_matmul(ctx, (P * np.float32(2.0 ** a)).astype(np.float32), M * 2.0 ** b))
                assert np.array_equal(got, base * np.float32(2.0 ** (a + b))), (a, b)


# ----------------------------------------------------------------------------------------------------------------------
# 5. dynamic range inside one operand
@pytest.mark.parametrize("d", SPREAD_D)
@pytest.mark.parametrize("route,which", [("gram", "a_cols"), ("gram", "a_rows"), ("tmul", "panel"), ("matmul", "panel")])
def test_dynamic_range(ctx, route, which, d):
    """magnitudes spread over d decades across the samples of a Gram matrix ("a_cols": the rows and columns of G), along its
    features ("a_rows": the summation index), across the columns of a wide panel and of the matrix of P·M.  d <= 4: the plain
    relative bound; d = 8: the bound gains the absolute term of `product_bounds` (tests/test_nt_model_host.py shows on these
    very inputs that the split alone stays inside the asserted bound and that d = 8 across rows or columns needs the term)."""
    from xeofs_amd import engine

    A, B = spread_inputs(route, d, which)
    what = f"spread d={d} {route} {which}"
    if route == "matmul":
        _check_matmul(ctx, np.ascontiguousarray(A.T), B.astype(np.float64), what, abs_term=d == 8, route="matmul_spread")
        return
    X = np.ascontiguousarray(A.T) if route == "gram" else A
    mat = engine.from_dense(ctx, X)
    assert np.array_equal(mat.download(), X)
    if route == "gram":
        _check_gram(mat, X, what, abs_term=d == 8, route="gram_spread")
    else:
        _check_tmul(ctx, mat, X, B, what, abs_term=d == 8, route="tmul_spread")
    mat.free()


# ----------------------------------------------------------------------------------------------------------------------
# 6. dirty scratch
def test_small_products_after_large_values_in_the_arena(ctx):
    """a large-valued product of a larger shape first: the arena that becomes the planes and the partial tiles of the small
    case is then full of big numbers (as fp16 bit patterns: infinities and NaN among them).  Padding features, padding rows
    and idle work items must still give exact zeros."""
    from xeofs_amd import engine

    rng = np.random.default_rng(6)
    big = (rng.standard_normal((700, 3000)) * 1e12).astype(np.float32)
    mat = engine.from_dense(ctx, big)
    assert np.isfinite(_bits(_gram(mat))[:700, :700]).all()
    Zb = (rng.standard_normal((700, 512)) * 1e12).astype(np.float32)
    engine.panel_tmul(ctx, mat, _panel(ctx, Zb, mat.n_pad), out=_nan_out(mat.p_pad, 512), prec="f16x3")
    mat.free()
    for n, p in GRAM_SHAPES[:3]:
        X = rng.standard_normal((n, p)).astype(np.float32)
        mat = engine.from_dense(ctx, X)
        _check_gram(mat, X, f"dirty arena gram {n}x{p}")
        mat.free()
    n, p, L = TMUL_SHAPES[0]
    X, Z = rng.standard_normal((n, p)).astype(np.float32), rng.standard_normal((n, L)).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    _check_tmul(ctx, mat, X, Z, f"dirty arena tmul {n}x{p} L={L}")
    mat.free()
    _matmul(ctx, (rng.standard_normal((1280, 1536)) * 1e12).astype(np.float32), rng.standard_normal((1536, 1504)) * 1e12)
    rows, L, Lo = MATMUL_SHAPES[1]
    _check_matmul(ctx, rng.standard_normal((rows, L)).astype(np.float32), rng.standard_normal((L, Lo)), f"dirty arena matmul {rows}x{L} Lo={Lo}")


# ----------------------------------------------------------------------------------------------------------------------
# 7. route switches
def test_route_switches(ctx, monkeypatch):
    """each route and the streaming or VALU kernel it replaces (EOFX_NO_FAST_GRAM, EOFX_NO_TMUL_NT, EOFX_NO_MATMUL_NT): both
    inside the SAME per-element bound against float64 (they are not compared with each other)"""
    from xeofs_amd import engine

    rng = np.random.default_rng(70)
    n, p, L = TMUL_SHAPES[1]
    X = rng.standard_normal((n, p)).astype(np.float32)
    Z = (rng.standard_normal((n, L)) * (1.0 + rng.random(L))).astype(np.float32)
    rows, Lm, Lo = MATMUL_SHAPES[1]
    P, M = rng.standard_normal((rows, Lm)).astype(np.float32), rng.standard_normal((Lm, Lo))
    mat = engine.from_dense(ctx, X)
    for off in (False, True):
        tag = "replaced kernel" if off else "NT route"
        for var in ("EOFX_NO_FAST_GRAM", "EOFX_NO_TMUL_NT", "EOFX_NO_MATMUL_NT"):
            monkeypatch.setenv(var, "1") if off else monkeypatch.delenv(var, raising=False)
        route = "replaced" if off else None
        _check_gram(mat, X, f"{tag} gram {n}x{p}", route=route and "gram_" + route)
        _check_tmul(ctx, mat, X, Z, f"{tag} tmul {n}x{p} L={L}", route=route and "tmul_" + route)
        _check_matmul(ctx, P, M, f"{tag} matmul {rows}x{Lm} Lo={Lo}", route=route and "matmul_" + route)
    mat.free()


def test_print_worst_ratios():
    """(last in the module) the largest error / bound per route over the cases that ran, for docs/EXPERIMENTS.md"""
    for route in sorted(RATIOS):
        print(f"worst error / bound, {route}: {RATIOS[route]:.3g}")
