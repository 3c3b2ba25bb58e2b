"""Host-side checks behind tests/test_gpu_preprocess_routes.py (no GPU needed).

1. The case lists of the GPU tests reach every route of the statistics stage, by the restated plans of that module: the three
   kernels of run_colstats with one row split and with several, a non-last split whose row count is not a multiple of 8, a short
   last split, the transposing kernel with a last split below 64 rows and P % 64 != 0, several workgroups of
   feature_summary_kernel (with missing features), both apply variants, every layout, the row map with both kernels and
   several splits, and the fused fit in both panel widths below and above one float64 flush per split with re-read rows.
   Removing a shape that alone reaches a route fails the test.
2. A numpy float64 emulation of the statistics with the association order of the kernels -- sums about the provisional shift c,
   sequential within a split, the splits in order, mu = c + s / k, M2 = max(q - s (s / k), 0), sd = max(sqrt(M2 / k), eps32) -- stays inside HALF the bound the GPU test
   asserts (its MARGIN of 2 is for the associations the emulation does not take), against the same two-pass np.longdouble
   reference, on every data family of the GPU file.  Likewise the fused form: values shifted by the nine-row probe mean in
   float32, float32 partial sums of squares over FIT_FLUSH slabs flushed into float64, the ones-column sum accumulated in
   float32 row by row, the re-read last row taken out with the kernel's own expression.
"""

import numpy as np
import pytest

import test_gpu_preprocess_routes as pr


def _plans():
    out = []
    for c in pr.CASES:
        aligned = c.inp != "misaligned"
        pv = c.P - pr.dead_features(c).size
        ns = c.n - pr.missing_rows(c).size
        out.append((c, pr.colstats_plan(c.n, c.P, aligned), pr.colstats_plan(c.n, c.P, aligned, sample_raw=c.hilbert and c.mode >= 2),
                    pr.apply_plan(c.n, c.P, pv, ns, c.mode, aligned), pv, ns))
    return out


def test_case_list_reaches_every_statistics_route():
    plans = _plans()
    first = [(c, p) for c, p, _, _, _, _ in plans]
    second = [(c, p) for c, _, p, _, _, _ in plans if c.hilbert]
    for kernel, runs in (("scalar", first), ("vec4", first), ("tr", second)):
        rs = [p["RS"] for c, p in runs if p["kernel"] == kernel]
        assert rs and min(rs) == 1 and max(rs) > 1, (kernel, rs)
    for kernel in ("scalar", "vec4"):
        mine = [p for c, p in first if p["kernel"] == kernel and p["RS"] > 1]
        assert any(p["rps"] % 8 for p in mine), kernel                # a tail inside a split other than the last
        assert any(p["last"] < p["rps"] for p in mine), kernel        # a short last split
        assert any(p["RS"] == 1 and c.n % 8 for c, p in first if p["kernel"] == kernel), kernel
    tr = [(c, p) for c, p in second if p["kernel"] == "tr"]
    assert len(tr) == len(second)
    assert all(p["rps"] % 64 == 0 for c, p in tr)
    assert any(p["last"] % 64 and p["RS"] > 1 for c, p in tr) and any(p["last"] % 64 and p["RS"] == 1 for c, p in tr)
    assert all(c.P % 64 for c, p in tr)
    # a misaligned field takes the scalar kernel although P % 4 == 0, and no raw layout
    mis = [(c, p, a) for c, p, _, a, _, _ in plans if c.inp == "misaligned"]
    assert mis and all(c.P % 4 == 0 and p["kernel"] == "scalar" and a == dict(layout="written", apply="scalar") for c, p, a in mis)
    # the summary kernel: several workgroups, with and without missing features
    assert any(pr.summary_blocks(c.P) > 1 and pv < c.P for c, _, _, _, pv, _ in plans)
    assert any(pr.summary_blocks(c.P) == 1 and pv < c.P for c, _, _, _, pv, _ in plans)
    layouts = {a["layout"] for _, _, _, a, _, _ in plans}
    assert layouts == {"written", "raw", "in_place", "masked"}, layouts
    assert {a["apply"] for _, _, _, a, _, _ in plans} == {"scalar", "vec", None}
    # masked in place with several summary blocks; a mask above 40 % falls back to compaction; missing samples leave the
    # in-place request for the written layouts
    assert any(a["layout"] == "masked" and pr.summary_blocks(c.P) > 1 for c, _, _, a, _, _ in plans)
    assert any(c.mode == 3 and c.family == "nan_hi" and a["layout"] == "written" and 10 * pv < 6 * c.P for c, _, _, a, pv, _ in plans)
    assert any(c.mode == 2 and ns < c.n and a["layout"] == "written" for c, _, _, a, _, ns in plans)
    assert any(c.mode == 1 and c.P % 4 and a["layout"] == "written" for c, _, _, a, _, _ in plans)
    # missing samples: the first row, the last row and one WHOLE row split, on both kernels, together with missing features
    for kernel in ("scalar", "vec4"):
        hit = [(c, p) for c, p in first if c.family == "missing" and p["kernel"] == kernel]
        assert hit, kernel
        for c, p in hit:
            rows = set(pr.missing_rows(c).tolist())
            assert {0, c.n - 1} <= rows and set(range(p["rps"], 2 * p["rps"])) <= rows and pr.dead_features(c).size
    # all-NaN features: the first and the last, and runs across the 4 / 64 / 256 / 512 boundaries
    for c in pr.CASES:
        if c.family in ("nan_lo", "nan_hi") and c.P > 600:
            dead = set(pr.dead_features(c).tolist())
            assert {0, c.P - 1} <= dead and all({b - 1, b} <= dead for b in (4, 64, 256, 512))
            assert (len(dead) < 0.4 * c.P) == (c.family == "nan_lo")
    # sizes: fewer than four features up to more than 4096; 1 or 2 samples, 63 / 64 / 65, several thousand
    assert min(c.P for c in pr.CASES) < 4 and max(c.P for c in pr.CASES) > 4096
    assert {2, 63, 64, 65} <= {c.n for c in pr.CASES} and max(c.n for c in pr.CASES) >= 5000
    assert {c.inp for c in pr.CASES} == {"host", "device", "misaligned"}
    assert {c.family for c in pr.CASES} == {"noise", "nan_lo", "nan_hi", "missing", "const", "weights"}
    assert all(c.n * c.P * 4 <= 64 << 20 for c in pr.CASES)


def test_fit_and_resample_lists_reach_their_routes():
    plans = [pr.fit_plan(c.n, c.P, c.k + c.over) for c in pr.FIT_CASES]
    for nb in (1, 2):
        mine = [p for p in plans if p["NB"] == nb]
        assert any(p["kps"] > pr.FLUSH_ROWS for p in mine), (nb, mine)         # the float64 flush happens more than once
        assert any(p["kps"] <= pr.FLUSH_ROWS for p in mine), (nb, mine)
    assert all(p["extra"] > 0 for p in plans)                                  # the correction for the re-read last row
    assert any(p["S"] > 1 for p in plans)
    res = [pr.colstats_plan(c.n_rows, c.P, ld=pr._up(c.P, 64), row_map=True) for c in pr.RESAMPLE_CASES]
    for kernel in ("scalar", "vec4"):
        rs = [p["RS"] for p in res if p["kernel"] == kernel]
        assert rs and min(rs) == 1 and max(rs) > 1, (kernel, rs)
    assert all(c.n_rows != c.n for c in pr.RESAMPLE_CASES)
    for n in pr.CANCEL_N:
        assert pr.colstats_plan(n, pr.CANCEL_P)["kernel"] == "vec4" and pr.colstats_plan(n, pr.CANCEL_P - 1)["kernel"] == "scalar"
    assert pr.CANCEL_RATIOS == (30.0, 1e3, 3e4, 1e6) and pr.CANCEL_N == (120, 5000, 60000)


# --------------------------------------------------------------------------- #
# the statistics, emulated                                                      #
# --------------------------------------------------------------------------- #
def emulate_two_step(X32, rps):
    """(k, mean, M2, std) of colstats*_kernel + colstats_finalize_kernel: float64, rows in order within a split, splits in order"""
    n, P = X32.shape
    k = np.zeros(P, np.int64)
    s, q = np.zeros(P), np.zeros(P)
    c = pr.stats_shift(X32).astype(np.float64)
    for r0 in range(0, n, rps):
        ks, ss, qs = np.zeros(P, np.int64), np.zeros(P), np.zeros(P)
        for r in range(r0, min(r0 + rps, n)):
            d = X32[r].astype(np.float64)
            ok = d == d
            d = np.where(ok, d - c, 0.0)
            ks += ok
            ss = ss + d
            qs = qs + d * d
        k, s, q = k + ks, s + ss, q + qs
    with np.errstate(invalid="ignore", divide="ignore"):
        ds = s / k
        mu = c + ds
        M2 = np.maximum(q - s * ds, 0.0)
        sd = np.maximum(np.sqrt(M2 / k), pr.EPS32)
    return k, mu, M2, sd


def emulate_fused(X32, kps):
    """(mean, M2, std) of the fused first pass + fit_finalize_kernel for a NaN-free field, a_scale = 1 (a power of two: exact)"""
    n, P = X32.shape
    f32 = np.float32
    c = pr.probe_shift(X32)
    K = pr._up(n, pr.ATB_KG)
    S1, q = np.zeros(P), np.zeros(P)
    for k0 in range(0, K, kps):
        acc = np.zeros(P, f32)                       # the matrix cores' float32 accumulator of this split (one rounding per row)
        qa = np.zeros((2, P), f32)                   # the two half-waves: rows 2t and 2t + 1
        q64 = np.zeros((2, P))
        for i, r in enumerate(range(k0, min(k0 + kps, K))):
            v = (X32[min(r, n - 1)].astype(np.float64) - c.astype(np.float64)).astype(f32)     # one fused multiply-add
            if r < n:                                # the ones column is zero beyond the field
                hi = v.astype(np.float16).astype(f32)
                lo = (v - hi).astype(np.float16).astype(f32)
                acc = (acc + hi).astype(f32)
                acc = (acc + lo).astype(f32)
            qa[r & 1] = (qa[r & 1] + (v * v).astype(f32)).astype(f32)
            if (i + 1) % pr.FLUSH_ROWS == 0:
                q64 += qa
                qa[:] = 0
        q64 += qa
        S1 = S1 + acc.astype(np.float64)
        q = q + (q64[0] + q64[1])
    extra = K - n
    if extra:
        v = (X32[n - 1].astype(np.float64) - c.astype(np.float64)).astype(f32).astype(np.float64)
        q = q - extra * (v * v)
    mu = c.astype(np.float64) + S1 / n
    M2 = np.maximum(q - S1 * S1 / n, 0.0)
    return mu, M2, np.maximum(np.sqrt(M2 / n), pr.EPS32)


def _inside_half(tag, ref, mu, M2, sd, dmean, dM2):
    """the emulated statistics of the valid features use at most half of MARGIN * bound"""
    half = pr.MARGIN / 2
    r_mean = float(np.max(np.abs(mu - ref["mean"]) / np.maximum(dmean, 1e-300)))
    r_m2 = float(np.max(np.where(dM2 > 0, np.abs(M2 - ref["M2"]) / np.where(dM2 > 0, dM2, 1.0), 0.0)))
    print(f"{tag}: |mean - ref| / bound = {r_mean:.3g}, |M2 - ref| / bound = {r_m2:.3g}")
    assert r_mean <= half and r_m2 <= half, (tag, r_mean, r_m2)
    assert np.all(M2[dM2 == 0] == ref["M2"][dM2 == 0])
    lo, hi = pr.std_interval(ref, dM2)
    assert np.all((sd >= lo) & (sd <= hi)), tag


@pytest.mark.parametrize("case", [c for c in pr.CASES if c.n * c.P <= 1_400_000], ids=lambda c: c.id)
def test_two_step_emulation_stays_inside_half_the_bound(case):
    X = pr.make_field(case)
    cols = np.unique(np.r_[np.arange(min(case.P, 96)), np.arange(max(case.P - 40, 0), case.P)])     # a slice keeps this fast
    plan = pr.colstats_plan(case.n, case.P, case.inp != "misaligned")
    Xs = X[:, cols]
    ref = pr.reference(Xs, True, True, None)
    k, mu, M2, sd = emulate_two_step(Xs, plan["rps"])
    vf = ref["vf"]
    assert np.array_equal(k > 0, vf) and np.all(k[vf] == ref["k"])
    _inside_half(case.id, ref, mu[vf], M2[vf], sd[vf], *pr.two_step_bounds(ref))


@pytest.mark.parametrize("n", pr.CANCEL_N)
def test_cancellation_emulation_two_step(n):
    X, R = pr.cancel_field(n, pr.CANCEL_P, seed=n + pr.CANCEL_P)
    ref = pr.reference(X, True, True, None)
    k, mu, M2, sd = emulate_two_step(X, pr.colstats_plan(n, pr.CANCEL_P)["rps"])
    dmean, dM2 = pr.two_step_bounds(ref)
    _inside_half(f"cancel n={n}", ref, mu, M2, sd, dmean, dM2)
    for ratio in pr.CANCEL_RATIOS:
        sel = R == ratio
        print(f"n={n} R={ratio:g}: emulated std error {np.max(np.abs(sd - ref['std'])[sel] / ref['std'][sel]):.3g}, "
              f"model {np.max((pr.MARGIN * dM2 / ref['M2'] / 2)[sel]):.3g}")


@pytest.mark.parametrize("case", pr.FIT_CASES, ids=lambda c: c.id)
def test_fused_emulation_stays_inside_half_the_bound(case):
    rng = pr._rng(case.id)
    n, P = case.n, case.P
    X = (rng.standard_normal((n, P)) * rng.uniform(0.5, 3.0, P) + rng.uniform(-50.0, 300.0, P)).astype(np.float32)[:, :48]
    kps = pr.fit_plan(n, P, case.k + case.over)["kps"]
    ref = pr.reference(X, True, True, None)
    mu, M2, sd = emulate_fused(X, kps)
    _inside_half(case.id, ref, mu, M2, sd, *pr.fused_bounds(ref, pr.probe_shift(X), kps))


@pytest.mark.parametrize("n", pr.CANCEL_FUSED_N)
def test_cancellation_emulation_fused(n):
    P = pr._up(n + 4, 4)
    X, R = pr.cancel_field(n, P, seed=n)
    X = X[:, :16]
    kps = pr.fit_plan(n, P, 16)["kps"]
    ref = pr.reference(X, True, False, None)
    mu, M2, sd = emulate_fused(X, kps)
    _inside_half(f"cancel fused n={n}", ref, mu, M2, sd, *pr.fused_bounds(ref, pr.probe_shift(X), kps))
