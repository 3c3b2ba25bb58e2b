"""Host-side checks behind tests/test_gpu_gw_kernels.py (no GPU needed).

1. A plain float64 numpy emulation of the covariance kernels' algorithm (csrc/eofx_gw.hpp) -- the shift r = the mean of a
   centre tile's rows, taken from the real centre tiling (eofx_gwplan.hpp through tests/plans_shim.cpp), gw_weight's formula on
   the plan's geo arrays, the augmented moments sum_j w [y; 1][y; 1]^T added location by location in the neighbours' sorted
   order as (w y_a) y_b, then gw_finalize_kernel's (S_ab - S_a S_b / W) / W -- stays under HALF of the bound the GPU test
   asserts against the longdouble reference, on every covariance case of that module.
2. Two deliberately broken variants exceed the bound: weights rounded to float32 (the six metric x kernel cases), and no
   shift (the two offset cases).  So the bound can tell a float32 intermediate or a missing shift from float64 rounding.
3. The case lists reach the pass counts 1, 2, 257 (exactly full) and 260 of gw_cov_kernel's grid and both plans, the bandwidth
   below the spacing visits one tile pair per centre tile, and the grid holds pairs at exactly d == bandwidth.

Figures of the emulation (the largest share of the bound per case group, printed by the test): features 0.042, locations
0.043, kernels 0.021, ranges 0.0081, geometry 0.010, shift 0.013.  Broken variants, as multiples of the bound: float32
weights 2.7e4 to 2.9e5, no shift 60 (field-1e3) and 1.3e6 (constant-1e4).  On an MI355X the kernels themselves used 0.035,
0.043, 0.014, 0.011, 0.0077 and 0.018 of it.
"""

import numpy as np
import pytest

import plans_shim
import test_gpu_gw_kernels as gk
from test_gwplan_cpu import Plan, weights


@pytest.fixture(scope="module")
def lib():
    return plans_shim.lib()


def emulate(lib, case, weight_dtype=np.float64, shift=True):
    """-> (cov [count, p, p], tv [count]) as gw_cov_kernel + gw_finalize_kernel compute them for engine.gw_cov (the unsorted
    plan).  Tile pairs the plan leaves out hold weights of exactly 0 (tests/test_gwplan_cpu.py), and adding 0 changes no sum, so
    every neighbour is visited here."""
    T = plans_shim.constants(lib)["GW_T"]
    pl = Plan(lib, case.xy, case.metric, case.kernel, case.bw, sorted_=False, first=case.first, count=case.count)
    X = case.X.astype(np.float64)
    n, p = X.shape
    cov, tv = np.zeros((case.count, p, p)), np.zeros(case.count)
    for c0 in range(0, case.count, T):
        rows = pl.c_perm[c0:c0 + T]
        tc = rows.size
        r = np.zeros(p)
        if shift:
            for i in rows:
                r = r + X[i]
            r = r / tc
        w = weights(pl.c_geo[c0:c0 + tc], pl.nb_geo, case.metric, case.kernel, case.bw).astype(weight_dtype).astype(np.float64)
        z = np.concatenate([X[pl.nb_perm] - r, np.ones((n, 1))], 1)
        S = np.zeros((tc, p + 1, p + 1))
        for j in range(n):
            S += (w[:, j, None, None] * z[j][None, :, None]) * z[j][None, None, :]
        S = np.triu(S) + np.triu(S, 1).transpose(0, 2, 1)         # the kernel holds a <= b only, the finalize mirrors it
        W = S[:, p, p][:, None, None]
        C = (S[:, :p, :p] - S[:, :p, p][:, :, None] * S[:, :p, p][:, None, :] / W) / W
        for s, i in enumerate(rows):
            cov[i - case.first] = C[s]
            t = 0.0
            for a in range(p):
                t += C[s, a, a]
            tv[i - case.first] = t
    return cov, tv


def share(case, cov, tv):
    ref = gk.reference(case)
    err = np.abs(cov.astype(gk.LD) - ref.C).astype(np.float64)
    terr = np.abs(tv.astype(gk.LD) - ref.tv).astype(np.float64)
    tb = np.einsum("iaa->i", ref.bound)
    assert np.all(err[ref.bound == 0] == 0) and np.all(terr[tb == 0] == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(np.where(ref.bound > 0, err / ref.bound, 0.0).max(), np.where(tb > 0, terr / tb, 0.0).max())


def test_emulation_uses_less_than_half_of_the_bound(lib):
    worst = {}
    for case in gk.CASES:
        cov, tv = emulate(lib, case)
        s = share(case, cov, tv)
        worst[case.group] = max(worst.get(case.group, 0.0), s)
        assert s < 0.5, (case.name, s)
        gk.check_covariance(case, cov, tv)          # the GPU test's own check passes on it, the exact zeros included
        gk.check_invariants(case, cov, tv)
    print("largest share of the bound per group:", {g: float(f"{s:.2g}") for g, s in worst.items()})
    assert set(worst) == {"features", "locations", "kernels", "ranges", "geometry", "shift"}


def test_broken_variants_exceed_the_bound(lib):
    seen = {}
    for case in gk.CASES:
        if case.group == "kernels":
            seen[case.name] = s = share(case, *emulate(lib, case, weight_dtype=np.float32))
            assert s > 10.0, (case.name, s)
        if case.group == "shift":
            seen[case.name] = s = share(case, *emulate(lib, case, shift=False))
            assert s > 10.0, (case.name, s)
    print("broken variants, multiples of the bound:", {k: float(f"{s:.2g}") for k, s in seen.items()})
    assert len(seen) == 9 + 2


def test_case_lists_reach_every_pass_count_plan_and_edge(lib):
    T = plans_shim.constants(lib)["GW_T"]
    assert T == gk.GW_T
    ps = {p: gk.passes(p) for p in gk.FEATURE_COUNTS}
    assert ps[1] == ps[2] == ps[3] == ps[14] == 1 and ps[15] == 2 and ps[255] == 257 and ps[256] == 260
    assert T * (256 * 257 // 2) == 257 * 2048                      # p = 255: every pass full
    assert T * (257 * 258 // 2) - 259 * 2048 == T                  # p = 256: one entry per location in the last pass
    assert {63, 64, 65} <= set(gk.FEATURE_COUNTS) and max(gk.FEATURE_COUNTS) == 256
    assert {1, 2, 15, 16, 17, 31, 33} <= set(gk.LOCATION_COUNTS)
    assert all(gk.CASE[f"features-p{p}"].n == 40 for p in gk.GWPCA_P + [65])
    # both plans: gw_cov tiles the range among itself (another order than the neighbours' when first > 0), gwpca cuts the
    # neighbours' order into chunks
    case = gk.CASE["ranges-7+93"]
    pu = Plan(lib, case.xy, "euclidean", "bisquare", case.bw, sorted_=False, first=7, count=93)
    assert len(pu.info) == 1 and pu.ctiles == 6 and np.array_equal(np.sort(pu.c_perm), np.arange(7, 100))
    first_count = {(c.first, c.count) for c in gk.CASES if c.group == "ranges"}
    assert first_count == set(gk.RANGES) and any(f % T and c % T for f, c in first_count)
    case = gk.CASE["features-p64"]
    ps_ = Plan(lib, case.xy, "euclidean", "bisquare", case.bw, chunk=16)
    assert [c[2] for c in ps_.chunks()] == [16, 16, 8] and np.array_equal(ps_.c_perm, ps_.nb_perm)
    # a bandwidth below the spacing: every centre tile lists its own tile alone
    case = gk.CASE["geometry-grid-alone"]
    pa = Plan(lib, case.xy, "euclidean", "bisquare", case.bw, sorted_=False, first=0, count=case.n)
    assert pa.visited == pa.ctiles == 4
    assert np.all(gk.reference(case).N == 1)
    # pairs at exactly d == bandwidth: weight exactly 0 with d <= bw; one ulp less and they are beyond it
    g = gk.CASE["geometry-grid-bw5"]
    w, d, _ = gk.ref_weights(g.xy, "euclidean", "bisquare", 5.0)
    at = d == 5
    assert at.sum() >= 2 * 40 and np.all(w[at] == 0) and np.all(weights(
        np.c_[g.xy, np.zeros(64)], np.c_[g.xy, np.zeros(64)], "euclidean", "bisquare", 5.0)[at] == 0.0)
    assert gk.CASE["geometry-grid-bw5-"].bw < 5.0
    assert np.array_equal(gk.reference(g).N, gk.reference(gk.CASE["geometry-grid-bw5-"]).N)
    # the antipodal case holds such pairs and the general haversine cases none (asserted inside the reference as well)
    assert gk.reference(gk.CASE["geometry-antipodal"]).near_antipodal >= 2 * (9 + 2)
    for name in ("kernels-haversine-gaussian", "kernels-haversine360-exponential"):
        assert gk.reference(gk.CASE[name]).near_antipodal == 0 and gk.reference(gk.CASE[name]).N.min() == 100
