"""Host-side checks behind tests/test_gpu_nt_routes.py (no GPU needed).

1. The shape lists of the GPU tests take the NT routes (the header's own predicates, through tests/plans_shim.cpp) and reach the
   plan edges named next to them, by the restated plan of that module (tests/test_gram_plan_cpu.py compares it with the header).
2. The numpy emulation of the f16x3 product (tests/test_product_model_host.py: emulate_f16x3 -- the split with EXACT
   accumulation) stays inside the bound the GPU test asserts, on the GPU test's own inputs: the split alone fits the model, what
   the kernels add is float32 accumulation, which the relative term covers.  On integer operands in [-16, 16] the emulation IS the
   integer product, so the GPU test may ask for equal bits.

Figures of the emulation on these inputs (printed by the tests): against the relative bound 1e-5 * sum|a||b| alone the split uses
at most 0.0081 at d <= 4; at d = 8 it exceeds that bound 6.8 times across the samples of the Gram matrix and 9.9 and 11.9 times
across the columns of the wide panel and of the matrix of P·M, and uses 0.012 of it when the spread runs along the summation
index.  With the absolute term it uses at most 0.071 of the bound anywhere.
"""

import numpy as np
import pytest

import plans_shim
import test_gpu_nt_routes as nt
from test_product_model_host import emulate_f16x3

routes = nt.routes


def test_shape_lists_take_the_nt_routes():
    lib = plans_shim.lib()
    for n, p in nt.GRAM_SHAPES + nt.EXACT_GRAM + [nt.LAYOUT_SHAPE[:2], nt.ODD_SHAPE[:2], nt.SPREAD_GRAM[::-1], nt.TMUL_SHAPES[1][:2]]:
        assert p >= n and lib.pl_gram_fast_ok(nt._up(n, 512), p, 1) == 1, (n, p)
    for n, p, L in nt.TMUL_SHAPES + [nt.LAYOUT_SHAPE, nt.ODD_SHAPE, nt.EXACT_TMUL, nt.SPREAD_TMUL]:
        assert L % 32 == 0 and lib.pl_tmul_nt_ok(n, nt._up(p, 512), 1, L) == 1, (n, p, L)
    for rows, L, Lo in nt.MATMUL_SHAPES + [nt.EXACT_MATMUL, (nt.SPREAD_MATMUL[1], nt.SPREAD_MATMUL[0], nt.SPREAD_MATMUL[2])]:
        assert lib.pl_matmul_nt_ok(rows, L, Lo) == 1, (rows, L, Lo)
    # ... and the shapes just below the thresholds do not
    assert lib.pl_tmul_nt_ok(511, 512, 1, 512) == 0 and lib.pl_tmul_nt_ok(512, 512, 1, 480) == 0
    assert lib.pl_matmul_nt_ok(768, 512, 256) == 0 and lib.pl_matmul_nt_ok(1024, 508, 256) == 0 and lib.pl_matmul_nt_ok(1024, 512, 252) == 0
    for shape in nt.GRAM_SHAPES + nt.TMUL_SHAPES + nt.MATMUL_SHAPES + [nt.LAYOUT_SHAPE, nt.ODD_SHAPE, nt.EXACT_TMUL, nt.SPREAD_TMUL]:
        assert max(shape) * sorted(shape)[-2] * 4 <= 64 << 20        # every matrix stays under 64 MB


def test_shape_lists_reach_the_plan_edges():
    g = {s: nt.gram_shape_plan(*s) for s in nt.GRAM_SHAPES}
    t = {s: nt.tmul_shape_plan(*s) for s in nt.TMUL_SHAPES}
    m = {s: nt.matmul_shape_plan(*s) for s in nt.MATMUL_SHAPES}
    TS = lambda pl: (pl["T"], pl["S"])
    # the table of the GPU module, row by row
    for s in [(29, 45), (40, 64)]:
        assert TS(g[s]) == (3, 1) and g[s]["nst_total"] == 2 and g[s]["grid"] == 8        # 3 real items among 8: 5 lanes idle
    assert TS(g[(40, 65)]) == (3, 1) and g[(40, 65)]["nst_total"] == 4
    assert TS(g[(300, 1037)]) == (3, 3) and (g[(300, 1037)]["st_per_split"], g[(300, 1037)]["last"]) == (12, 10)
    assert all(1037 % q for q in (4, 8, 32))
    assert TS(g[(513, 1100)]) == (10, 3) and g[(513, 1100)]["cmax"] == 2
    assert TS(g[(1100, 1440)]) == (21, 4) and (g[(1100, 1440)]["st_per_split"], g[(1100, 1440)]["last"]) == (12, 10)
    assert TS(g[(1537, 1600)]) == (36, 5) and g[(1537, 1600)]["cmax"] == 5
    assert TS(g[(300, 4100)]) == (3, 5) and g[(300, 4100)]["st_per_split"] == 26
    assert t[(512, 300, 512)]["S"] == 2
    assert t[(700, 3000, 512)]["S"] == 3 and (t[(700, 3000, 512)]["st_per_split"], t[(700, 3000, 512)]["last"]) == (8, 6)
    assert nt._up(768, 256) == 768 and nt._up(544, 256) == 768
    assert m[(1024, 512, 256)]["S"] == 2
    assert m[(1024, 516, 260)]["S"] == 3 and nt._up(516, 64) == 576 and 516 % 8 and 260 % 256
    # the edges, over the lists
    plans = list(g.values()) + list(t.values()) + list(m.values())
    for group in (g, t, m):
        S = [pl["S"] for pl in group.values()]
        assert max(S) > 1, S
    assert min(pl["S"] for pl in g.values()) == 1
    assert any(pl["last"] < pl["st_per_split"] for pl in plans)                         # a short last split
    assert any(pl["nst_total"] == 2 for pl in plans)                                    # the shortest legal loop
    assert any(pl["T"] % 8 and pl["cmax"] > 1 for pl in plans)
    assert any(nt._up(p, 64) > p for _, p in nt.GRAM_SHAPES) and any(nt._up(n, 64) > n for n, _, _ in nt.TMUL_SHAPES)      # kpad > K
    assert any(nt._up(L, 64) > L for _, L, _ in nt.MATMUL_SHAPES)
    assert any(nt._up(L, 256) > L for _, _, L in nt.TMUL_SHAPES) and any(nt._up(Lo, 256) > Lo for _, _, Lo in nt.MATMUL_SHAPES)     # Lp > L
    # the forced split counts of the exact test change the plan of every exact shape, and some leave a short last split
    for plan_of, shapes in ((nt.gram_shape_plan, nt.EXACT_GRAM), (nt.tmul_shape_plan, [nt.EXACT_TMUL]), (nt.matmul_shape_plan, [nt.EXACT_MATMUL])):
        for s in shapes:
            S = {plan_of(*s, S=f or 0)["S"] for f in nt.SPLITS}
            assert len(S) >= 4 and 1 in S, (s, S)
            assert any(plan_of(*s, S=f or 0)["last"] < plan_of(*s, S=f or 0)["st_per_split"] for f in nt.SPLITS), s
    # the ragged last group of 8 (4) features: with the map on the in-place field, without it on the written ones
    assert nt.LAYOUT_SHAPE[1] % 4 == 0 and nt.LAYOUT_SHAPE[1] % 8 and nt.ODD_SHAPE[1] % 4
    # the masked field stays in place: the valid features are at least 0.6 of all and outnumber the samples
    X, _ = nt.layout_inputs("masked")
    pv = int((~np.isnan(X[0])).sum())
    assert 10 * pv >= 6 * X.shape[1] and X.shape[0] < pv < X.shape[1]
    land = np.isnan(X[0])
    runs = np.diff(np.flatnonzero(np.diff(np.r_[0, land.astype(np.int8), 0])))[::2]
    assert runs.max() >= 128 and (runs == 1).any()              # whole 64-feature runs and isolated points
    # the tile corners of the exact test: both sides of a sub-block edge and of a tile edge, and the last row
    n = nt.EXACT_GRAM[1][0]
    rows = nt.corner_rows(n)
    assert {0, 255, 256, 511, n - 1} <= set(rows) and {63, 64} <= set(rows) and n > 512


def test_exact_operands_are_exact_in_the_emulation():
    """integers in [-16, 16]: hi is exact, lo zero, the emulated product the integer product bit for bit; every partial sum
    of the scaled products is an integer below 2^24 times a power of two, so float32 accumulation is exact too"""
    for n, p in nt.EXACT_GRAM:
        for X in (nt.int_operands((n, p), n + p), nt.census_field(n, p)):
            A = np.ascontiguousarray(X.T)
            assert np.array_equal(emulate_f16x3(A, A), X.astype(np.float64) @ X.astype(np.float64).T)
            assert (np.abs(A.astype(np.float64)).T @ np.abs(A.astype(np.float64))).max() < 2 ** 24
    n, p, L = nt.EXACT_TMUL
    X, Z = nt.int_operands((n, p), 11), nt.int_operands((n, L), 12)
    assert np.array_equal(emulate_f16x3(X, Z), X.astype(np.float64).T @ Z.astype(np.float64))
    assert 256 * max(n, nt.EXACT_MATMUL[1], max(p for _, p in nt.EXACT_GRAM)) < 2 ** 24
    C = nt.census_field(300, 1037)
    assert sorted(set(np.diag(C @ C.T).tolist())) == [3.0, 4.0] and np.count_nonzero(C @ C.T) == 300


@pytest.mark.parametrize("d", nt.SPREAD_D)
@pytest.mark.parametrize("route,which", [("gram", "a_cols"), ("gram", "a_rows"), ("tmul", "panel"), ("matmul", "panel")])
def test_split_emulation_stays_inside_the_asserted_bound(route, which, d):
    A, B = nt.spread_inputs(route, d, which)
    ref, rel, absb = routes.product_bounds(A, B, routes.TOL["f16x3"])
    err = np.abs(emulate_f16x3(A, B) - ref)
    r_model, r_rel = float((err / (rel + absb)).max()), float((err / rel).max())
    print(f"{route} {which} d={d}: error / (rel + abs) = {r_model:.3g}, error / rel alone = {r_rel:.3g}")
    assert r_model <= 1.0                # the model the GPU test asserts at d = 8 holds for the split at every d
    if d <= 4:
        assert r_rel <= 1.0              # ... and d <= 4 does not need the absolute term
    if d == 8 and which != "a_rows":
        assert r_rel > 1.0               # ... while d = 8 across rows or columns cannot hold without it
