"""Host-side checks behind tests/test_gpu_lag_routes.py (no GPU needed).

1. A restatement of the grouping rule of the lag operator (lag_groupsize in csrc/eofx_plans.hpp: EOFX_LAG_GROUP_COLS = 1024,
   G = max(1, min(E, 1024 // L))) and of n' / n'_pad proves that the GPU test's case list reaches every edge it is there
   for.  When a constant of the rule moves, this test says which case has to move with it.
2. The float64 reference of the uncentred field, recomputed in long double, stays far inside the bounds the GPU test
   asserts: those bounds judge the kernel, not the reference.
"""

import numpy as np

import plans_shim
import test_gpu_lag_routes as lag


def test_restated_constants_match_the_source():
    """the restated grouping rule against the header itself (csrc/eofx_plans.hpp through tests/plans_shim.cpp, compiled with the
    host compiler) -- the constant, the group size and the groups in launch order; tests/test_plans_cpu.py sweeps the rest"""
    lib = plans_shim.lib()
    assert plans_shim.constants(lib)["LAG_GROUP_COLS"] == lag.LAG_GROUP_COLS
    shapes = [(1, 32), (40, 32), (11, 96), (5, 256), (3, 544), (3, 2048)]
    assert [lib.pl_lag_groupsize(E, L) for E, L in shapes] == [lag.lag_groupsize(E, L) for E, L in shapes] == [1, 32, 10, 4, 1, 1]
    for E, L in shapes + [(21, 96)]:
        out = np.zeros(E, np.int32)
        assert out[:lib.pl_lag_groups(E, L, out.ctypes.data)].tolist() == lag.lag_groups(E, L)
    assert lag.lag_groups(11, 96) == [10, 1] and lag.lag_groups(40, 32) == [32, 8] and lag.lag_groups(3, 544) == [1, 1, 1]


def test_case_list_reaches_every_edge():
    cases = lag.CASES + lag.EXTRA_CASES
    assert len(lag.CASES) == 10 and len(set(cases)) == 12
    groups = {c: lag.lag_groups(c[2], c[4]) for c in cases}
    for (n, p, E, tau, L), g in groups.items():
        assert sum(g) == E and L % 32 == 0 and lag.n_emb(n, E, tau) >= 2
        assert max(g) * L <= max(lag.LAG_GROUP_COLS, L)
        assert n * lag._up(p, 4) * 4 <= 64 << 20
    # one group
    assert any(len(g) == 1 and c[2] > 1 for c, g in groups.items())
    assert groups[lag.CASES[5]] == [1]                                  # E = 1
    # one full group and a shorter last one; several full groups and a shorter last one
    assert groups[lag.CASES[6]] == [10, 1] and groups[lag.CASES[7]] == [4, 1]
    assert groups[lag.GROUPS_CASE] == [10, 10, 1]
    assert any(len(g) >= 3 and g[0] == g[1] > 1 and g[-1] < g[0] for g in groups.values())
    # G = 1 with several groups, at a panel above 512 columns
    assert groups[lag.CASES[8]] == [1, 1, 1] and lag.CASES[8][4] > 512
    # the widths of the wide products of CASES[7]: 1024 and 256 columns
    assert [g * lag.CASES[7][4] for g in groups[lag.CASES[7]]] == [1024, 256]
    ne = {c: lag.n_emb(c[0], c[2], c[3]) for c in cases}
    pads = {c: (lag._up(ne[c], 512), lag._up(c[0], 512)) for c in cases}
    # n'_pad < n_pad
    assert pads[lag.CASES[1]] == (512, 1536) and pads[lag.CASES[2]] == (1024, 1536)
    # n' on both sides of a 512 boundary
    assert {ne[c] % 512 for c in cases} >= {0, 1, 511}
    assert ne[lag.CASES[0]] == 1023 and ne[lag.CASES[1]] == 512 and ne[lag.CASES[2]] == 513
    # disjoint windows (tau >= n'): rows that lie in no window
    disjoint = [c for c in cases if c[2] > 1 and c[3] > ne[c]]
    assert lag.CASES[1] in disjoint and lag.CASES[4] in disjoint
    n, p, E, tau, L = lag.CASES[4]
    assert ne[lag.CASES[4]] == 9 and list(range(ne[lag.CASES[4]], tau)) == list(range(9, 20))
    # n' = 2
    assert ne[lag.CASES[3]] == 2
    # several row and feature tiles, p off a multiple of 4
    n, p = lag.CASES[0][:2]
    assert n > 512 and p > 512 and p % 4
    # both sides of the NT kernel of the f16x3 X^T W
    assert lag.tmul_nt_ok(lag.NT_CASE[0], groups[lag.NT_CASE][0] * lag.NT_CASE[4])
    assert not any(lag.tmul_nt_ok(c[0], g * c[4]) for c in lag.CASES for g in groups[c])
    # the plan runs every case, the two all-precision cases on an owned matrix, every source at least once
    planned = {c for c, _ in lag.PLAN}
    assert planned == set(cases)
    assert {s for _, s in lag.PLAN} == {"owned", "in_place", "raw", "sample_only"}
    assert all((c, "owned") in lag.PLAN for c in lag.ALL_PREC_CASES)
    assert lag.ALL_PREC_CASES == (lag.CASES[0], lag.CASES[6])
    assert all(lag.precisions(c, "owned") == list(lag.TOL) for c in lag.ALL_PREC_CASES)
    assert all({"f32", "f16x3"} <= set(lag.precisions(c, s)) for c, s in lag.PLAN)
    # the in-place X.Y of CASES[9] runs split along the features
    import test_gpu_product_routes as routes

    assert (lag.CASES[9], "in_place") in lag.PLAN and routes.in_place_mul_splits(*lag.CASES[9][:2]) > 1


def test_window_count_formula():
    """the number of windows that hold row t, as lag_stats_kernel counts it (with its guard for rows in no window),
    against the definition -- on every case of the list"""
    for n, p, E, tau, L in lag.CASES + lag.EXTRA_CASES:
        ne = lag.n_emb(n, E, tau)
        t = np.arange(n)
        hi = np.minimum(E - 1, t // tau)
        lo = np.where(t >= ne, (t - ne + tau) // tau, 0)
        cnt = np.where(hi >= lo, hi - lo + 1, 0)
        ref = sum(((t >= e * tau) & (t < e * tau + ne)).astype(int) for e in range(E))
        assert np.array_equal(cnt, ref)
        if (n, p, E, tau, L) in (lag.CASES[1], lag.CASES[4]):
            assert (ref == 0).any()                 # rows in no window (there hi - lo + 1 is 0, never negative)


def test_uncentred_reference_is_inside_its_bounds():
    """the float64 reference of test_uncentred_field against long double: it uses a small fraction of the bounds, which are
    about 1e-6 relative on the variance (the offset is 1000 standard deviations) -- an error of a window boundary is of
    order 1 / n'"""
    X = lag.uncentred_field()
    n, p = X.shape
    sd = X.astype(np.float64).std(axis=0)
    assert np.all(np.abs(X.astype(np.float64).mean(axis=0)) > 800 * sd)       # (the sample deviation of 301 values scatters by some per cent)
    for E, tau in [(5, 2), (2, 200), (3, 7)]:
        ne = lag.n_emb(n, E, tau)
        Xe, mu, tv, mu_bound, tv_bound = lag.stats_reference(X, tau, E)
        Xl = lag.embed(X.astype(np.longdouble), tau, E)
        mul = Xl.sum(axis=0) / ne
        tvl = ((Xl - mul) ** 2).sum() / (ne - 1)
        assert np.all(np.abs(mu - mul) <= 0.01 * mu_bound)
        assert abs(tv - tvl) <= 0.01 * tv_bound
        assert 1e-8 * tv < tv_bound < 2e-6 * tv, (tv_bound / tv)
        # one row counted in one window too many (an off-by-one in cnt(t) of lag_stats_kernel) is far outside the bound
        assert (X[n - 1].astype(np.float64) ** 2).sum() / (ne - 1) > 1e3 * tv_bound
