"""Host-side checks behind tests/test_gpu_complex_routes.py (no GPU needed).

1. The shape lists of the GPU tests reach s_half == 1 and s_half > 1 of the two-matrix launch in both directions, on the narrow
   plan (64 columns) and the wide one (128 columns), and S == 1 and S > 1 of the in-place X Y plan -- by the restated plans of
   tests/test_gpu_product_routes.py (tests/test_plans_cpu.py compares those with the header itself).  The two-matrix launch
   runs 2 * s_half splits: s_half of the plan for ONE matrix over Re, as many over Im.
2. The numpy emulation of the f16x3 product (tests/test_product_model_host.py) on the STACKED operands of the GPU test's
   scale-spread inputs -- one power-of-two scale for [A; B], as the two-matrix launch takes it from max(|A|, |B|) -- stays
   inside the bound the GPU test asserts there (relative + absolute term).

Figures of the emulation (printed by the test): with one part 2^-10 of the other the split uses 0.0011 to 0.0016 of the
relative bound alone, in either direction and whichever part is the small one -- the absolute term is the model's allowance
for the shared scale, not something these inputs need.
"""

import numpy as np
import pytest

import test_gpu_complex_routes as croutes
import test_gpu_product_routes as routes
from test_product_model_host import emulate_f16x3

# (n, p): s_half of Z^H W at 64 / 128 columns, of Z Y at 64 / 128 columns
EXPECTED_SPLITS = {(29, 44): (1, 1, 2, 2), (23, 40012): (1, 1, 126, 126), (40012, 24): (126, 126, 1, 1),
                   (1037, 2332): (33, 17, 37, 37)}
EXPECTED_IN_PLACE = {(301, 900): 1, (333, 5000): 40}


def _splits(n, p):
    return tuple(f(n, p, L) for f in (routes.tmul_splits, routes.mul_splits) for L in (64, 128))


def test_shape_list_reaches_every_split_plan():
    for shape, want in EXPECTED_SPLITS.items():
        assert shape in croutes.SHAPES and _splits(*shape) == want, (shape, _splits(*shape))
    for shape, want in EXPECTED_IN_PLACE.items():
        assert shape in croutes.LEAN_SHAPES and shape in croutes.SHAPES
        assert routes.in_place_mul_splits(*shape) == want, (shape, routes.in_place_mul_splits(*shape))
    assert _splits(2, 4)[:2] == (1, 1) and (2, 4) in croutes.SHAPES
    every = [_splits(n, p) for n, p in croutes.SHAPES]
    for i in range(4):       # Z^H W narrow, wide; Z Y narrow, wide
        s = [e[i] for e in every]
        assert min(s) == 1 and max(s) > 1, (i, s)
    lean = [routes.in_place_mul_splits(n, p) for n, p in croutes.LEAN_SHAPES]
    assert min(lean) == 1 and max(lean) > 1, lean
    # the precision and operator shapes run split and unsplit as well
    prec = [_splits(n, p) for n, p in croutes.PREC_SHAPES]
    assert min(min(e) for e in prec) == 1 and max(max(e) for e in prec) > 1


def test_shapes_fit_the_rules():
    shapes = set(croutes.SHAPES + croutes.PREC_SHAPES + croutes.LEAN_SHAPES + croutes.OPERATOR_SHAPES + [croutes.MAIN_SHAPE])
    assert shapes == set(croutes.SHAPES)
    for n, p in shapes:
        assert p % 4 == 0                                    # the field can stay in place
        assert n * p * 4 <= 64 << 20, (n, p)
    n, p = croutes.MAIN_SHAPE
    assert all(v % t for v in (n, p) for t in (512, 256, 64, 32))
    assert routes._up(n, 512) > 512 and routes._up(p, 512) > 512
    # the masked fields keep the matrix in place: a valid share of at least 0.6, more valid features than samples
    for n, p in croutes.LEAN_SHAPES:
        X, _ = croutes.lean_field(n, p, seed=n + p, masked=True)
        dead = np.isnan(X).all(0)
        assert np.array_equal(np.isnan(X).any(0), dead)
        runs = np.flatnonzero(np.diff(np.r_[0, dead.astype(int), 0]) == 1).size
        assert (~dead).sum() >= 0.6 * p and (~dead).sum() > n and dead.sum() > 0 and runs >= 2, (n, p)


@pytest.mark.parametrize("conj_left", [True, False])
@pytest.mark.parametrize("small", ["A", "B"])
def test_split_emulation_of_the_shared_scale(small, conj_left):
    A, B = croutes.spread_pair(small)
    n, p = A.shape
    assert np.abs(A if small == "A" else B).max() < 2.0 ** -7 * np.abs(B if small == "A" else A).max()
    P = croutes.panel_for(n if conj_left else p, croutes.SPREAD_L, 100 * croutes.SPREAD_L + conj_left)   # the GPU test's panel
    SA, SP = croutes.stacked(A, B, P, conj_left)
    ref, rel, absb = routes.product_bounds(SA, SP, routes.TOL["f16x3"])
    err = np.abs(emulate_f16x3(SA, SP) - ref)
    r_model, r_rel = float((err / (rel + absb)).max()), float((err / rel).max())
    print(f"small={small} {'ZhW' if conj_left else 'ZY'}: error / (rel + abs) = {r_model:.3g}, error / rel alone = {r_rel:.3g}")
    assert r_model <= 1.0
