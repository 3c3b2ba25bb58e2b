"""Host-side checks behind tests/test_gpu_product_routes.py (no GPU needed).

1. The shape lists of the GPU tests reach S == 1 and S > 1 of the split-K plans on every launcher (launch_atb narrow and
   wide, launch_axb) and every column tile, by the restated plans of that module.
2. A numpy emulation of the f16x3 product -- power-of-two scaling from the operand maxima, the two-term round-to-nearest fp16
   split, the three cross products hi*hi + hi*lo + lo*hi, EXACT accumulation -- stays inside the bound the GPU test asserts,
   on the GPU test's own inputs.  The split alone therefore fits the model; what the kernels add is float32 accumulation,
   which the relative term covers.

Figures of the emulation on these inputs (worst over the five shapes, printed by the test): against the relative bound
1e-5 * sum|a||b| alone the split uses at most 0.008 at d <= 4 and 0.12 at d = 6; at d = 8 it exceeds that bound 3 to 19
times when the spread runs across output columns or rows ("panel", "a_cols") and uses 0.011 of it when the spread runs along
the summation index ("a_rows").  With the absolute term it uses at most 0.11 of the bound anywhere.
"""

import numpy as np
import pytest

import test_gpu_product_routes as routes


def test_shape_lists_reach_every_split_plan_and_tile():
    narrow = [routes.tmul_splits(n, p, L) for n, p in routes.TMUL_SHAPES for L in (32, 64)]
    wide = [routes.tmul_splits(n, p, L) for n, p in routes.TMUL_SHAPES for L in routes.WIDTHS if L >= 96]
    assert min(narrow) == 1 and max(narrow) > 1, narrow
    assert min(wide) == 1 and max(wide) > 1, wide
    narrow = [routes.mul_splits(n, p, L) for n, p in routes.MUL_SHAPES for L in (32, 64)]
    wide = [routes.mul_splits(n, p, L) for n, p in routes.MUL_SHAPES for L in routes.WIDTHS if L >= 96]
    assert min(narrow) == 1 and max(narrow) > 1, narrow
    assert min(wide) == 1 and max(wide) > 1, wide
    # the other precisions take the narrow plan at every width
    other = [routes.tmul_splits(*routes.ALL_PREC_SHAPE, L, "f32") for L in routes.WIDTHS]
    assert max(other) > 1, other
    axb = [routes.in_place_mul_splits(n, p) for n, p in routes.AXB_SHAPES]
    assert min(axb) == 1 and max(axb) > 1, axb
    # the in-place shape of the power-of-two test runs split, the spread shape too
    assert routes.in_place_mul_splits(333, 2100) > 1
    seen = set()
    for L in routes.WIDTHS:
        assert routes.tiles(L, "f16x3") == routes.EXPECTED_TILES_F16[L]
        assert routes.tiles(L, "f32") == routes.EXPECTED_TILES_NARROW[L]
        assert sum(96 if t == "P96" else t for t in routes.tiles(L, "f16x3")) == L
        seen.update(routes.tiles(L, "f16x3"))
    assert seen == {32, 64, 128, "P96"}
    for n, p in routes.TMUL_SHAPES + routes.MUL_SHAPES + routes.AXB_SHAPES + [routes.SPREAD_SHAPE]:
        assert n * p * 4 <= 64 << 20


def test_shapes_are_off_every_tile_size_or_dominated_by_padding():
    n, p = routes.ALL_PREC_SHAPE
    assert all(v % t for v in (n, p) for t in (512, 256, 64, 16))
    assert routes.TMUL_SHAPES[0] == routes.ALL_PREC_SHAPE == routes.MUL_SHAPES[0]
    n, p = routes.TMUL_SHAPES[1]
    assert n * p * 50 < 512 * 512 and routes.MUL_SHAPES[1] == (n, p)


def _scale_for(m):
    """f16_scale_for: 2^(14 - e) with m = f * 2^e, f in [0.5, 1): the scaled maximum lies in [2^13, 2^14)"""
    if not (m > 0 and np.isfinite(m)):
        return 1.0
    _, e = np.frexp(np.float32(m))
    return float(np.ldexp(1.0, 14 - int(e)))


def _split(x32):
    hi = x32.astype(np.float16)                       # round to nearest, subnormals kept
    lo = (x32 - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulate_f16x3(A, B):
    """C = A^T B, A [K x M], B [K x L] float32: three cross products of the scaled split, accumulated exactly (float64 holds
    every partial product of two fp16 numbers; the sums of a few thousand of them lose nothing that matters at 2^-38)"""
    sa, sb = _scale_for(np.abs(A).max()), _scale_for(np.abs(B).max())
    ah, al = _split(A * np.float32(sa))
    bh, bl = _split(B * np.float32(sb))
    return (ah.T @ bh + ah.T @ bl + al.T @ bh) / (sa * sb)


EMUL_SHAPES = [(700, 100, 32), (3000, 64, 96), (520, 1000, 64), routes.SPREAD_SHAPE + (routes.SPREAD_L,),
               routes.SPREAD_SHAPE[::-1] + (routes.SPREAD_L,)]


@pytest.mark.parametrize("which", routes.SPREADS)
@pytest.mark.parametrize("d", [0, 2, 4, 6, 8])
def test_split_emulation_stays_inside_the_asserted_bound(d, which):
    worst_model = worst_rel = 0.0
    least_rel = np.inf
    for K, M, L in EMUL_SHAPES:
        A, B = routes.spread_operands(K, M, L, d, which, seed=1)
        ref, rel, absb = routes.product_bounds(A, B, routes.TOL["f16x3"])
        err = np.abs(emulate_f16x3(A, B) - ref)
        r_model, r_rel = float((err / (rel + absb)).max()), float((err / rel).max())
        print(f"K={K} M={M} L={L} d={d} {which}: error / (rel + abs) = {r_model:.3g}, error / rel alone = {r_rel:.3g}")
        worst_model, worst_rel, least_rel = max(worst_model, r_model), max(worst_rel, r_rel), min(least_rel, r_rel)
    assert worst_model <= 1.0            # the model the GPU test asserts at d = 8 holds for the split at every d
    if d <= 4:
        assert worst_rel <= 1.0          # ... and d <= 4 does not need the absolute term
    if d == 8 and which != "a_rows":
        assert least_rel > 1.0           # ... while d = 8 cannot hold without it, on every shape
    # ("a_rows" spreads the SUMMATION index: every sum is dominated by its large terms and the relative bound holds alone)
