"""One pass of the complex operator Z = A + iB over a [Re | Im] panel, Z^H W and Z Y (eofx_cmat_mul_f32,
eofx_hilbert_cmat_mul_f32: CplxOps::zh_mul / z_mul of csrc/eofx_abi.hip), route by route against float64.

The complex product is a real product of stacked operands:

    Z^H W = [A; B]^T [W; R],      R  = [Wi | -Wr]        (A, B stacked along the samples)
    Z Y   = [A^T; B^T]^T [Y; R'], R' = [-Yi | Yr]        (A^T, B^T stacked along the features)

so every case follows the rules of tests/test_gpu_product_routes.py, whose helpers it imports:

  reference     the float64 product of the stacked float32 matrices the engine holds: `download()` of a written part; for an
                in-place or masked part the download of the two-layout matrix preprocessed with the same arguments
  bound         product_bounds(stacked A, stacked panel, TOL[prec]): tol * sum_k |a_k| |b_k| per element, the relative term
                alone; the absolute term of the split-fp16 model only where one part is 2^-10 of the other (the two parts of
                a two-matrix launch share ONE fp16 scale, so the small part is quantised against the large part's maximum)
  dirty output  the output is full of NaN before the call
  padding       the padding rows of the output are exact zeros afterwards
  rerun         a second call returns the same bits; the panel and the operands' download() are unchanged
  size          every matrix is at most 64 MB

Routes (tests/test_complex_routes_host.py proves, without a GPU, that the shapes reach s_half == 1 and s_half > 1 of the
two-matrix launch in both directions and at both widths, and S == 1 and S > 1 of the in-place X Y plan):

  two-matrix    a written pair under f16x3: one launch, splits [0, s_half) stream A against the panel, [s_half, 2 s_half) stream
                B against the companion panel of cpanel_rot; the reduction always runs (at s_half == 1 over exactly two partials)
  two launches  a written pair under f32 / bf16x3 / bf16x6 / f64: one launch per part + cpanel_combine
  lean          64 columns, f16x3, some part not held in both written layouts: every part is streamed in a layout it has
                (raw field through the Scaler map: atb AFF (+ MASK) / axb; a sample-contiguous-only part: axb with the identity
                map / atb), the two products meet in cpanel_combine in place
  operator      Z = (I + i Hc) A with the resident Hilbert operator: two chained products and a combine in between
"""

import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_product_routes as routes
from test_gpu_product_routes import TOL, _check, _nan_out, _panel, product_bounds

pytestmark = pytest.mark.gpu

EOFX_ERR_ARG, EOFX_ERR_SHAPE = -1, -8
HILBERT_OP_MAX_N = 16384

# (n, p), every p a multiple of 4 (the field can stay in place): the smallest / padding dominates, Z^H W has s_half == 1 /
# off 512, 256, 64 and 32 on both axes, several M tiles either way / one K group under many feature tiles, Z Y at
# s_half == 126 / its mirror / the in-place X Y plan at S == 1 / at S > 1
SHAPES = [(2, 4), (29, 44), (1037, 2332), (23, 40012), (40012, 24), (301, 900), (333, 5000)]
MAIN_SHAPE = (1037, 2332)
PREC_SHAPES = [(1037, 2332), (29, 44)]
OTHER_PRECISIONS = ["f32", "bf16x3", "bf16x6", "f64"]
LEAN_SHAPES = [(301, 900), (333, 5000), (1037, 2332), (29, 44)]
OPERATOR_SHAPES = [(29, 44), (301, 900), (1037, 2332)]
SPREAD_L = 64
SPREAD_FACTOR = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def written_pair(n, p):
    """two independent N(0,1) parts with feature-dependent magnitudes (B is NOT a Hilbert transform of A: a sign or a half
    that is mixed up cannot cancel)"""
    rng = np.random.default_rng(7919 * n + p)
    A = (rng.standard_normal((n, p)) * (1.0 + rng.random(p))).astype(np.float32)
    B = (rng.standard_normal((n, p)) * (0.5 + 2.0 * rng.random(p))).astype(np.float32)
    return A, B


def spread_pair(small):
    """the scale-spread inputs at MAIN_SHAPE (shared with the host emulation): part `small` ("A" | "B") is 2^-10 times
    unit-scale data, the other part is unit scale"""
    A, B = written_pair(*MAIN_SHAPE)
    f = np.float32(SPREAD_FACTOR)
    return (A * f, B) if small == "A" else (A, B * f)


def panel_for(rows, L, seed):
    return np.random.default_rng(seed).standard_normal((rows, L)).astype(np.float32)


def stacked(Am, Bm, P, conj_left):
    """(stacked field [K x M], stacked panel [K x L]) with Z^H P (conj_left) or Z P equal to field^T panel"""
    h = P.shape[1] // 2
    Pr, Pi = P[:, :h], P[:, h:]
    if conj_left:
        return np.vstack([Am, Bm]), np.vstack([P, np.hstack([Pi, -Pr])])
    return np.vstack([Am.T, Bm.T]), np.vstack([P, np.hstack([-Pi, Pr])])


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _one_pass(ctx, mul, P, rows_in_pad, rows_out, rows_out_pad, ref, bound, what):
    """`mul(panel, out)` twice into NaN-filled outputs: the bound and the padding, the same bits, the panel untouched"""
    Pd = _panel(ctx, P, rows_in_pad)
    before = _host(Pd).copy()
    got = mul(Pd, _nan_out(rows_out_pad, P.shape[1]))
    _check(got, ref, bound, rows_out, what)
    again = mul(Pd, _nan_out(rows_out_pad, P.shape[1]))
    g = _host(got)
    assert _same_bits(g, _host(again)), f"{what}: a second call returns other bits"
    assert _same_bits(before, _host(Pd)), f"{what}: the input panel was modified"
    return g


def _both_directions(ctx, A, B, Am, Bm, L, prec, what, finals=(False, True), abs_term=False, seed=0):
    """Z^H W and Z Y of the resident pair against the float64 products of the stacked (Am, Bm), what the engine holds over
    the physical feature axis"""
    from xeofs_amd import engine

    n, p = Am.shape
    for conj_left in (True, False):
        P = panel_for(n if conj_left else p, L, 100 * L + 2 * seed + conj_left)
        ref, rel, absb = product_bounds(*stacked(Am, Bm, P, conj_left), TOL[prec])
        for final in finals:
            _one_pass(ctx, lambda Pd, out: engine.cmat_mul(ctx, A, B, Pd, conj_left, final, out=out), P,
                      A.n_pad if conj_left else A.p_pad, p if conj_left else n, A.p_pad if conj_left else A.n_pad, ref,
                      rel + absb if abs_term else rel, f"{what} {'ZhW' if conj_left else 'ZY'} L={L} {prec} final={int(final)}")


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 128])
@pytest.mark.parametrize("n,p", SHAPES)
def test_written_pair_two_matrix_form(ctx, n, p, L):
    """a written pair under the default precision: ONE launch over both parts (64 columns: the 64-column tile, 128: the wide
    one), both directions, power and final pass"""
    from xeofs_amd import engine

    assert ctx.precision == ("f16x3", "f16x3")
    Ah, Bh = written_pair(n, p)
    A, B = engine.from_dense(ctx, Ah), engine.from_dense(ctx, Bh)
    assert (A.n_pad, A.p_pad) == (routes._up(n, 512), routes._up(p, 512))
    _both_directions(ctx, A, B, Ah, Bh, L, "f16x3", f"two-matrix {n}x{p}")
    assert np.array_equal(A.download(), Ah) and np.array_equal(B.download(), Bh)
    A.free()
    B.free()


@pytest.mark.parametrize("small", ["A", "B"])
def test_written_pair_scale_spread(ctx, small):
    """one part 2^-10 of the other: the two-matrix launch scales BOTH with the larger maximum, so the small part carries the
    absolute error of the split-fp16 model -- the bound is the relative plus the absolute term of product_bounds on the
    stacked operands (tests/test_complex_routes_host.py: the split alone stays inside it on these inputs)"""
    from xeofs_amd import engine

    Ah, Bh = spread_pair(small)
    A, B = engine.from_dense(ctx, Ah), engine.from_dense(ctx, Bh)
    _both_directions(ctx, A, B, Ah, Bh, SPREAD_L, "f16x3", f"spread small={small}", abs_term=True)
    assert np.array_equal(A.download(), Ah) and np.array_equal(B.download(), Bh)
    A.free()
    B.free()


@pytest.mark.parametrize("n,p", PREC_SHAPES)
@pytest.mark.parametrize("prec", OTHER_PRECISIONS)
def test_written_pair_other_precisions(ctx, prec, n, p):
    """the native two-launch branch: one launch per part and cpanel_combine, under every other precision the context accepts
    (xeofs_amd/complex_svd.py composes this case in Python, so nothing else reaches it)"""
    from xeofs_amd import engine

    Ah, Bh = written_pair(n, p)
    A, B = engine.from_dense(ctx, Ah), engine.from_dense(ctx, Bh)
    try:
        ctx.set_precision(prec, prec)
        for L in (64, 128):
            _both_directions(ctx, A, B, Ah, Bh, L, prec, f"two-launch {n}x{p}")
    finally:
        ctx.set_precision("f16x3", "f16x3")
    assert np.array_equal(A.download(), Ah) and np.array_equal(B.download(), Bh)
    A.free()
    B.free()


# ----------------------------------------------------------------------------------------------------------------------
def lean_field(n, P, seed, masked=False):
    """an uncentred field with feature-dependent spread and weights (the Scaler map matters); masked: runs of all-NaN grid
    points and scattered ones, about a quarter of the features"""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, P)) * (1.0 + 3.0 * rng.random(P)) + np.linspace(-40.0, 250.0, P)).astype(np.float32)
    if masked:
        land = np.zeros(P, bool)
        land[P // 7:P // 7 + P // 6] = True
        land[P - 3 - P // 12:P - 3] = True
        land[rng.integers(0, P, P // 40 + 1)] = True
        X[:, land] = np.nan
    return X, np.linspace(0.2, 1.7, P)


def _held(ctx, X, w):
    """what the engine holds for the field over the PHYSICAL feature axis (zeros at the masked features): the download of the
    two-layout matrix preprocessed with the same arguments"""
    from xeofs_amd import engine

    m2, st = engine.preprocess(ctx, X, True, True, w)
    valid = st["valid_feature"]
    Xh = np.zeros(X.shape, np.float32)
    Xh[:, valid] = m2.download()
    m2.free()
    return Xh, valid


@pytest.mark.parametrize("n,p", LEAN_SHAPES)
@pytest.mark.parametrize("flavour", ["hilbert", "both_in_place", "masked_hilbert"])
def test_lean_routes(ctx, flavour, n, p):
    """64 columns over a pair that is not held in both written layouts: Re in place + Im as the Hilbert stage leaves it (sample
    layout only), both parts in place, a masked Re in place + its Hilbert Im.  Nothing is written for the passes; a 128-column
    pass on the same pair afterwards (which does write the layouts) meets the same bound.  The panel of a masked pair holds
    N(0,1) values at the masked features too: the reference has zeros there, nothing of them may reach the product."""
    from xeofs_amd import engine

    assert ctx.precision == ("f16x3", "f16x3")
    masked = flavour == "masked_hilbert"
    X, w = lean_field(n, p, seed=n + p, masked=masked)
    A, _ = engine.preprocess(ctx, X, True, True, w, in_place=True, allow_masked=masked)
    assert A.masked == masked and A.layout() == (False, True) and A.p_phys == p
    Am, valid = _held(ctx, X, w)
    if masked:
        assert valid.sum() >= 0.6 * p and valid.sum() > n and not valid.all() and A.p == valid.sum()
    if flavour == "both_in_place":
        X2, w2 = lean_field(n, p, seed=3 * n + p + 1)
        B, _ = engine.preprocess(ctx, X2, True, True, w2[::-1].copy(), in_place=True)
        Bm, _ = _held(ctx, X2, w2[::-1].copy())
        b_lean = lambda: B.layout() == (False, True)                            # noqa: E731
    else:
        B, _ = engine.hilbert(ctx, A, "exp", 0.2)
        assert B.p == p and not B.masked
        Bm = None                                                               # (download() writes B's other layout: afterwards)
        b_lean = lambda: B.layout()[0] is False and B.has_sample_layout()       # noqa: E731
    assert b_lean() and not A.has_sample_layout()
    # the 64-column passes first, checked once B may be downloaded
    results = []
    for conj_left in (True, False):
        P = panel_for(n if conj_left else p, 64, 64 + conj_left)
        rin, rout = (A.n_pad, A.p_pad) if conj_left else (A.p_pad, A.n_pad)
        Pd = _panel(ctx, P, rin)
        for final in (False, True):
            got = engine.cmat_mul(ctx, A, B, Pd, conj_left, final, out=_nan_out(rout, 64))
            again = engine.cmat_mul(ctx, A, B, Pd, conj_left, final, out=_nan_out(rout, 64))
            assert _same_bits(_host(got), _host(again)), (flavour, conj_left, final)
            results.append((conj_left, final, P, got))
        assert _same_bits(_host(Pd)[:P.shape[0]], P)
    assert A.layout() == (False, True) and not A.has_sample_layout() and b_lean()      # nothing was written for the passes
    late = []
    for conj_left in (True, False):     # 128 columns: not lean -- the layouts are written, one two-matrix launch
        P = panel_for(n if conj_left else p, 128, 128 + conj_left)
        rin, rout = (A.n_pad, A.p_pad) if conj_left else (A.p_pad, A.n_pad)
        late.append((conj_left, False, P, engine.cmat_mul(ctx, A, B, _panel(ctx, P, rin), conj_left, out=_nan_out(rout, 128))))
    if Bm is None:
        Bm = B.download()
        assert Bm.shape == (n, p) and not Bm[:, ~valid].any()
    for conj_left, final, P, got in results + late:
        ref, rel, _ = product_bounds(*stacked(Am, Bm, P, conj_left), TOL["f16x3"])
        what = f"lean {flavour} {n}x{p} {'ZhW' if conj_left else 'ZY'} L={P.shape[1]} final={int(final)}"
        _check(got, ref, rel, p if conj_left else n, what)
        if masked and conj_left:
            assert not _host(got)[:p][~valid].any(), f"{what}: not an exact zero at a masked feature"
    if not masked:
        assert _same_bits(A.download(), Am)
    assert _same_bits(B.download(), Bm)
    A.free()
    B.free()


# ----------------------------------------------------------------------------------------------------------------------
def _operator_bound(Am, Hc, P, conj_left, tol):
    """two chained products under the per-product model.  Z^H W = A^T (W - i Hc^T W): the first product errs by
    tol |Hc|^T |W|, which the second carries through |A|^T, and errs itself by tol |A|^T |W - i Hc^T W| --
    2 tol |A|^T (|W| + |Hc|^T |W~|) covers both.  Z Y = (I + i Hc)(A Y) likewise: 2 tol (|A||Y| + |Hc||A||Y~|).
    (~: the halves swapped -- the real part of the result takes the imaginary part of the operator term and the other
    way round.)"""
    h = P.shape[1] // 2
    A64, H64, P64 = np.abs(Am.astype(np.float64)), np.abs(Hc.astype(np.float64)), np.abs(P.astype(np.float64))
    Psw = np.hstack([P64[:, h:], P64[:, :h]])
    if conj_left:
        return 2.0 * tol * (A64.T @ (P64 + H64.T @ Psw))
    return 2.0 * tol * (A64 @ P64 + H64 @ (A64 @ Psw))


@pytest.mark.parametrize("n,p", OPERATOR_SHAPES)
@pytest.mark.parametrize("padding", ["exp", None])
@pytest.mark.parametrize("layout", ["in_place", "written"])
def test_operator_route(ctx, layout, padding, n, p):
    """eofx_hilbert_cmat_mul_f32 -- the products of eofx_rsvd_hilbert_c64 -- against complex128 of (I + i Hc) A with the
    float32 operator the engine hands out; and against the two-part pass over (A, hilbert(A)): the two differ by both bounds
    plus what the operator and the stage differ by, 2e-5 of each series' scale (test_hilbert_operator), carried through the
    product"""
    from xeofs_amd import engine

    assert ctx.precision == ("f16x3", "f16x3")
    X, w = lean_field(n, p, seed=5 * n + p)
    A, _ = engine.preprocess(ctx, X, True, True, w, in_place=layout == "in_place")
    if layout == "in_place":
        assert A.layout() == (False, True) and not A.has_sample_layout()
    else:
        assert A.layout()[0] and A.has_sample_layout()
    Am, _ = _held(ctx, X, w)
    Hc = engine.hilbert_operator(ctx, n, padding, 0.2)
    Z = Am.astype(np.float64) + 1j * (Hc.astype(np.float64) @ Am.astype(np.float64))
    kept = []
    for L in (64, 128):
        h = L // 2
        for conj_left in (True, False):
            P = panel_for(n if conj_left else p, L, 7 * L + conj_left)
            Pc = P[:, :h].astype(np.float64) + 1j * P[:, h:].astype(np.float64)
            rc = (Z.conj().T if conj_left else Z) @ Pc
            bound = _operator_bound(Am, Hc, P, conj_left, TOL["f16x3"])
            rin, rout = (A.n_pad, A.p_pad) if conj_left else (A.p_pad, A.n_pad)
            for final in (False, True):
                def mul(Pd, out):
                    return engine.hilbert_cmat_mul(ctx, A, Pd, conj_left, padding, 0.2, final, out=out)
                g = _one_pass(ctx, mul, P, rin, p if conj_left else n, rout, np.hstack([rc.real, rc.imag]), bound,
                              f"operator {layout} {padding} {n}x{p} {'ZhW' if conj_left else 'ZY'} L={L} final={int(final)}")
            kept.append((conj_left, P, g, bound))
    if layout == "in_place":
        assert A.layout() == (False, True) and not A.has_sample_layout()       # the operator passes wrote nothing
    # the two-part pass over the stage's own imaginary part
    B, _ = engine.hilbert(ctx, A, padding, 0.2)
    got2 = [engine.cmat_mul(ctx, A, B, _panel(ctx, P, A.n_pad if cl else A.p_pad), cl) for cl, P, _, _ in kept]
    Bm = B.download()
    scale = np.abs(Am.astype(np.float64)).max(0)                                 # per series (feature)
    for (conj_left, P, g, bound), g2 in zip(kept, got2):
        SA, SP = stacked(Am, Bm, P, conj_left)
        _, rel, _ = product_bounds(SA, SP, TOL["f16x3"])
        R = np.abs(SP[P.shape[0]:].astype(np.float64))                           # the companion panel meets the imaginary part
        stage = 2e-5 * (scale[:, None] * R.sum(0)[None, :] if conj_left else np.ones((n, 1)) * (scale @ R)[None, :])
        rows = p if conj_left else n
        diff = np.abs(g[:rows].astype(np.float64) - _host(g2)[:rows].astype(np.float64))
        ratio = float((diff / (bound + rel + stage)).max())
        print(f"operator against two-part {layout} {padding} {n}x{p} {'ZhW' if conj_left else 'ZY'} L={P.shape[1]}: "
              f"worst difference / allowance = {ratio:.3g}")
        assert ratio <= 1.0
    assert _same_bits(A.download(), Am)
    A.free()
    B.free()


# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """a width other than 64 / 128, parts of different shape, a non-positive decay with padding, more samples than the resident
    operator takes: the error code comes back before anything is launched (the NaN-filled output is untouched) and the context
    goes on working"""
    from xeofs_amd import engine
    from xeofs_amd._lib import ptr

    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(5)
    Ah, Bh = written_pair(29, 44)
    A, B = engine.from_dense(ctx, Ah), engine.from_dense(ctx, Bh)
    B_cols = engine.from_dense(ctx, rng.standard_normal((29, 48)).astype(np.float32))
    B_rows = engine.from_dense(ctx, rng.standard_normal((30, 44)).astype(np.float32))
    tall = engine.from_dense(ctx, rng.standard_normal((HILBERT_OP_MAX_N + 1, 4)).astype(np.float32))
    P = _panel(ctx, rng.standard_normal((29, 256)).astype(np.float32), tall.n_pad)
    out = _nan_out(tall.n_pad, 256)

    def cm(a, b, L, conj_left=1):
        return lib.eofx_cmat_mul_f32(h, a.handle, b.handle, conj_left, ptr(P), L, 0, ptr(out))

    def hm(a, padding, decay, L, conj_left=1):
        return lib.eofx_hilbert_cmat_mul_f32(h, a.handle, padding, C.c_double(decay), conj_left, ptr(P), L, 0, ptr(out))

    for L in (0, 32, 96, 160, 256, -64):
        assert cm(A, B, L) == EOFX_ERR_ARG, L
        assert hm(A, 1, 0.2, L) == EOFX_ERR_ARG, L
    for other in (B_cols, B_rows):
        for conj_left in (0, 1):
            assert cm(A, other, 64, conj_left) == EOFX_ERR_SHAPE
    for decay in (0.0, -0.2, float("nan")):
        assert hm(A, 1, decay, 64) == EOFX_ERR_ARG, decay
    for conj_left in (0, 1):
        assert hm(tall, 1, 0.2, 64, conj_left) == EOFX_ERR_ARG
        assert hm(tall, 0, 0.2, 128, conj_left) == EOFX_ERR_ARG
    with pytest.raises(ValueError):
        engine.cmat_mul(ctx, A, B_cols, P[:A.n_pad, :64].contiguous(), True)
    with pytest.raises(ValueError):
        engine.hilbert_cmat_mul(ctx, A, P[:A.n_pad, :64].contiguous(), True, "exp", 0.0)
    assert np.isnan(_host(out)).all()                                            # nothing was launched
    assert hm(A, 0, 0.0, 64) == 0 and cm(A, B, 64) == 0                          # no padding: the decay is not looked at
    assert np.isfinite(_host(out)[:A.p_pad * 64 // 256]).all()                   # ([p_pad x 64] at the head of the buffer)
    for m in (A, B, B_cols, B_rows, tall):
        m.free()
