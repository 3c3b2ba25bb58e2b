"""The launch plans of xeofs_amd/csrc/eofx_plans.hpp without a GPU: the header is plain C++, so tests/plans_shim.cpp (extern "C"
wrappers and nothing else) is compiled with the host C++ compiler and loaded through ctypes (tests/plans_shim.py).

1. The Python restatements that the GPU route tests choose their shapes with (tests/test_gpu_product_routes.py,
   test_gpu_preprocess_routes.py, test_gpu_lag_routes.py) equal the header's functions -- on the GPU tests' own case lists and
   on a seeded sweep of a few thousand shapes per rule.  A changed constant in the header fails here instead of silently moving
   the GPU tests off the routes they exist to cover.
2. Invariants of the split plans; the block-covariance plan against a numpy brute force; the padded weight vectors of the filter
   plans against np.pad."""
import ctypes
import itertools

import numpy as np
import pytest

import plans_shim
import test_gpu_lag_routes as lag
import test_gpu_preprocess_routes as pr
import test_gpu_product_routes as routes

PREC_F16X3 = 3          # include/eofx.h


@pytest.fixture(scope="module")
def lib():
    return plans_shim.lib()


# --------------------------------------------------------------------------- #
# the header's functions as the restatements return them                        #
# --------------------------------------------------------------------------- #
def c_tiles(lib, L, wide):
    w = np.zeros(64, np.int32)
    k = lib.pl_tiles(L, int(wide), w.ctypes.data)
    assert k > 0, (L, wide)
    return ["P96" if t == 96 else t for t in w[:k].tolist()]


def c_atb(lib, M, K, L, wide):
    kps = ctypes.c_int64()
    return lib.pl_atb_plan(M, K, L, int(wide), ctypes.addressof(kps)), kps.value


def c_axb(lib, rows_pad, K):
    kps = ctypes.c_int64()
    return lib.pl_axb_plan(rows_pad, K, ctypes.addressof(kps)), kps.value


def c_colstats(lib, n, P, aligned=True, ld=None, sample_raw=False, row_map=False):
    out = np.zeros(5, np.int64)
    lib.pl_colstats_plan(n, P, ld or P, int(aligned), int(sample_raw), int(row_map), out.ctypes.data)
    kernel, RS, rps = ("scalar", "vec4", "tr")[out[0]], int(out[1]), int(out[2])
    return dict(kernel=kernel, RS=RS, rps=rps, last=n - (RS - 1) * rps)


def c_apply(lib, n, P, pv, ns, mode, aligned=True):
    out = np.zeros(5, np.int32)
    lib.pl_apply_plan(n, P, pv, ns, min(mode, 2), int(mode == 3), 1, int(aligned), out.ctypes.data)
    raw, masked, in_place, col_map, vec = (bool(x) for x in out)
    if in_place:
        return dict(layout="masked" if masked else "in_place", apply=None)
    return dict(layout="raw" if raw else "written", apply="vec" if vec else "scalar")


def c_fit(lib, n, P, l):
    assert lib.pl_fit_first_eligible(2, PREC_F16X3, 1, n, P, l) == 1
    L, K = pr._up(l, 32), pr._up(n, routes.ATB_KG)
    S, kps = c_atb(lib, pr._up(P, routes.ATB_BM), K, L, False)
    return dict(NB=L // 32, S=S, kps=kps, extra=K - n)


def c_lag_groups(lib, E, L):
    out = np.zeros(max(E, 1), np.int32)
    k = lib.pl_lag_groups(E, L, out.ctypes.data)
    return out[:k].tolist()


def c_wide(lib, L, prec):
    return prec == "f16x3" and bool(lib.pl_atb_wide(L))


# --------------------------------------------------------------------------- #
# 1. restatements against the header                                            #
# --------------------------------------------------------------------------- #
def test_restated_constants(lib):
    c = plans_shim.constants(lib)
    assert (c["ATB_BM"], c["ATB_KG"], c["AXB_BM"], c["AXB_KG"]) == (routes.ATB_BM, routes.ATB_KG, routes.AXB_BM, routes.AXB_KG)
    assert c["LAG_GROUP_COLS"] == lag.LAG_GROUP_COLS


def test_product_restatements_on_the_gpu_case_lists(lib):
    for L in routes.WIDTHS:
        for prec in routes.TOL:
            assert routes.tiles(L, prec) == c_tiles(lib, L, c_wide(lib, L, prec)), (L, prec)
        for n, p in routes.TMUL_SHAPES:
            for prec in ("f16x3", "f32"):
                assert routes.tmul_splits(n, p, L, prec) == c_atb(lib, routes._up(p, 512), routes._up(n, 32), L, c_wide(lib, L, prec))[0]
        for n, p in routes.MUL_SHAPES:
            for prec in ("f16x3", "f32"):
                assert routes.mul_splits(n, p, L, prec) == c_atb(lib, routes._up(n, 512), routes._up(p, 32), L, c_wide(lib, L, prec))[0]
    for n, p in routes.AXB_SHAPES + [c[:2] for c in lag.CASES + lag.EXTRA_CASES] + [(333, 2100)]:
        assert routes.in_place_mul_splits(n, p) == c_axb(lib, routes._up(n, 512), routes._up(p, 64))[0], (n, p)


def test_product_restatements_on_a_sweep(lib):
    rng = np.random.default_rng(2024)
    Ls = list(range(32, 545, 32))
    Ms = [512, 512 * 1024] + [512 * int(x) for x in rng.integers(1, 300, 40)]
    Ks = [32] + [32 * int(x) for x in rng.integers(1, 4000, 40)]
    count = 0
    for L in Ls:
        for wide in (False, True):
            assert routes.tiles(L, "f16x3" if wide else "f32") == c_tiles(lib, L, wide and L >= 96)
        for M, K in zip(rng.permutation(Ms * 3)[:100], rng.permutation(Ks * 3)[:100]):
            for wide in (False, True):
                assert routes.atb_splits(int(M), int(K), L, wide) == c_atb(lib, int(M), int(K), L, wide)[0], (M, K, L, wide)
                count += 1
    for M, K in itertools.product([512, 512 * 1024], [32, 64, 40032]):
        for L in Ls:
            assert routes.atb_splits(M, K, L, L >= 96) == c_atb(lib, M, K, L, L >= 96)[0]
    assert count >= 3000
    rts = [1, 2, 1023, 1024, 1025] + [int(x) for x in rng.integers(1, 1100, 60)]
    units = [1, 15, 16, 17, 255, 256, 257] + [int(x) for x in rng.integers(1, 20000, 60)]
    for rt, u in itertools.product(rts, units):
        assert routes.axb_splits(256 * rt, 64 * u) == c_axb(lib, 256 * rt, 64 * u)[0], (rt, u)
    assert len(rts) * len(units) >= 3000


def _preprocess_calls():
    """the arguments with which the GPU tests and their host model call the restated statistics plans"""
    for c in pr.CASES:
        aligned = c.inp != "misaligned"
        yield (c.n, c.P, aligned, None, False, False)
        yield (c.n, c.P, aligned, None, c.hilbert, False)
        yield (c.n, c.P, True, None, True, False)
    for c in pr.RESAMPLE_CASES:
        yield (c.n_rows, c.P, True, pr._up(c.P, 64), False, True)
    for n in pr.CANCEL_N:
        yield (n, pr.CANCEL_P, True, None, False, False)
        yield (n, pr.CANCEL_P - 1, True, None, False, False)


def test_statistics_restatements_on_the_gpu_case_lists(lib):
    for args in _preprocess_calls():
        assert pr.colstats_plan(*args) == c_colstats(lib, *args), args
    for c in pr.CASES:
        aligned = c.inp != "misaligned"
        pv, ns = c.P - pr.dead_features(c).size, c.n - pr.missing_rows(c).size
        assert pr.apply_plan(c.n, c.P, pv, ns, c.mode, aligned) == c_apply(lib, c.n, c.P, pv, ns, c.mode, aligned), c.id
        assert pr.summary_blocks(c.P) == lib.pl_summary_blocks(c.P)
    for route, n, P, family, mode, *_ in pr.APPLY_CASES:
        for pv in (P, P - 1, (6 * P + 9) // 10, P // 2):
            assert pr.apply_plan(n, P, pv, n, mode) == c_apply(lib, n, P, pv, n, mode), (route, pv)
    for c in pr.FIT_CASES:
        assert pr.fit_plan(c.n, c.P, c.k + c.over) == c_fit(lib, c.n, c.P, c.k + c.over), c.id
    for n, P in zip(pr.CANCEL_FUSED_N, (128, 5004)):
        assert pr.fit_plan(n, P, 16) == c_fit(lib, n, P, 16)


def test_statistics_restatements_on_a_sweep(lib):
    rng = np.random.default_rng(7)
    ns = [1, 2, 63, 64, 65, 127, 128, 8192, 8193] + [int(x) for x in rng.integers(1, 70000, 40)]
    Ps = [1, 3, 4, 5, 1023, 1024, 1025, 4096, 4097] + [int(x) for x in rng.integers(1, 600000, 40)]
    count = 0
    for n, P in itertools.product(ns, Ps):
        for aligned, pad, sample_raw, row_map in ((True, 0, False, False), (False, 0, False, False), (True, 0, True, False),
                                                  (True, 3, False, True), (True, 64, True, True)):
            args = (n, P, aligned, P + pad if pad else None, sample_raw, row_map)
            assert pr.colstats_plan(*args) == c_colstats(lib, *args), args
            count += 1
        assert pr.summary_blocks(P) == lib.pl_summary_blocks(P)
        for mode, aligned in itertools.product(range(4), (True, False)):
            for pv, ns_ in ((P, n), (P, max(n - 1, 1)), (max(P - 1, 1), n), ((6 * P + 9) // 10, n), (max((6 * P - 1) // 10, 1), n),
                            (min(n, P), n), (min(n + 1, P), n)):
                assert pr.apply_plan(n, P, pv, ns_, mode, aligned) == c_apply(lib, n, P, pv, ns_, mode, aligned), (n, P, pv, ns_, mode, aligned)
    assert count >= 3000
    fits = 0
    for n, P4, l in zip(rng.integers(3, 20000, 4000), rng.integers(1, 40000, 4000), rng.integers(1, 64, 4000)):
        n, P, l = int(n), 4 * int(P4), int(l)
        if n < P and l < n and l % 32:
            assert pr.fit_plan(n, P, l) == c_fit(lib, n, P, l), (n, P, l)
            fits += 1
    assert fits >= 1000


def test_lag_restatements(lib):
    """the grouping rule of the lag operator and the shape part of tmul_nt_ok, on the GPU case list and on a sweep (this is what
    test_lag_model_host.py::test_restated_constants_match_the_source stands on)"""
    for n, p, E, tau, L in lag.CASES + lag.EXTRA_CASES:
        assert lag.lag_groupsize(E, L) == lib.pl_lag_groupsize(E, L)
        assert lag.lag_groups(E, L) == c_lag_groups(lib, E, L)
        for g in lag.lag_groups(E, L):
            assert lag.tmul_nt_ok(n, g * L) == bool(lib.pl_tmul_nt_ok(n, lag._up(p, 512), 1, g * L))
    count = 0
    for E, L in itertools.product(list(range(1, 70)) + [100, 1000], list(range(32, 545, 32)) + [1024, 2048]):
        assert lag.lag_groupsize(E, L) == lib.pl_lag_groupsize(E, L) and lag.lag_groups(E, L) == c_lag_groups(lib, E, L), (E, L)
        count += 1
    rng = np.random.default_rng(3)
    for n, Lw in itertools.product([511, 512, 513] + [int(x) for x in rng.integers(2, 40000, 60)], [480, 511, 512, 513, 544, 1024]):
        assert lag.tmul_nt_ok(n, Lw) == bool(lib.pl_tmul_nt_ok(n, 2560, 1, Lw)), (n, Lw)
        count += 1
    assert count >= 1500
    assert not lib.pl_tmul_nt_ok(1037, 2560, 0, 512)            # (no layout the route can read)


# --------------------------------------------------------------------------- #
# 2. invariants, the block-covariance plan, the filter plans                    #
# --------------------------------------------------------------------------- #
def test_split_plan_invariants(lib):
    """S * kps >= K, (S - 1) * kps < K (no empty split) and kps a multiple of the granularity"""
    rng = np.random.default_rng(11)
    for L in range(32, 545, 32):
        for M, K in zip([512, 512 * 1024] + [512 * int(x) for x in rng.integers(1, 300, 30)],
                        [32, 32] + [32 * int(x) for x in rng.integers(1, 4000, 30)]):
            for wide in (False, True):
                S, kps = c_atb(lib, M, K, L, wide)
                assert 1 <= S <= 128 and S * kps >= K and (S - 1) * kps < K and kps % routes.ATB_KG == 0, (M, K, L, wide, S, kps)
    for rt, u in itertools.product([1, 2, 40, 1023, 1024], [1, 15, 16, 17, 100, 255, 256, 257, 5000, 16200]):
        S, kps = c_axb(lib, 256 * rt, 64 * u)
        assert S >= 1 and S * kps >= 64 * u and (S - 1) * kps < 64 * u and kps % routes.AXB_KG == 0, (rt, u, S, kps)
        assert S == 1 or (rt < 1024 and u >= 16)


def _viewcov(lib, n, p, off, keep_diag):
    view, tiles, out3 = np.zeros(p, np.int32), np.zeros((33 * 17, 2), np.int32), np.zeros(3, np.int64)
    off = np.asarray(off, np.int32)
    k = lib.pl_viewcov_plan(n, p, off.ctypes.data, len(off) - 1, int(keep_diag), view.ctypes.data, tiles.ctypes.data, len(tiles),
                            out3.ctypes.data)
    return k, view, tiles[:max(k, 0)], out3


def _view_offsets(p, m, T):
    """m views over p columns: one boundary exactly on a tile edge and one inside a tile where p and m leave room"""
    if m == 1:
        return [[0, p]]
    if m > p:
        return []
    rng = np.random.default_rng(p + m)
    outs = []
    for forced in ([T] if p > T else [], [T // 2 + 1] if p > T // 2 + 1 else [], [T, T + T // 2 + 1] if p > 2 * T else []):
        forced = forced[:m - 1]
        rest = [c for c in rng.permutation(np.arange(1, p)).tolist() if c not in forced][:m - 1 - len(forced)]
        outs.append([0] + sorted(forced + rest) + [p])
    return outs


@pytest.mark.parametrize("p", [1, 127, 128, 129, 300, 4096])
def test_block_covariance_plan(lib, p):
    """Against a numpy brute force over all p x p entries: a 128-tile (bi, bj), bi <= bj, is listed iff it holds an entry (i, j)
    with i <= j and (keep_diag or different views), in row-major order.  No split of the samples is empty, and the partial
    blocks of a split run stay within VIEWCOV_WGS: G * ntiles <= VIEWCOV_WGS wherever the samples are split at all (p = 4096 with
    every tile wanted has 528 tiles, more than VIEWCOV_WGS: there G = 1 and no partial block exists)."""
    c = plans_shim.constants(lib)
    T, WGS = c["VIEWCOV_T"], c["VIEWCOV_WGS"]
    nb = (p + T - 1) // T
    for m in (1, 2, 5, 64):
        for off in _view_offsets(p, m, T):
            v = np.repeat(np.arange(m), np.diff(off))
            differ = v[:, None] != v[None, :]
            for keep_diag in (False, True):
                wanted = np.triu(differ | keep_diag)
                brute = [(bi, bj) for bi in range(nb) for bj in range(bi, nb) if wanted[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T].any()]
                for n in (2, 4095, 4096, 100000):
                    k, view, tiles, (G, chunk, nslabs) = _viewcov(lib, n, p, off, keep_diag)
                    assert k >= 0 and np.array_equal(view, v)
                    assert [tuple(t) for t in tiles.tolist()] == brute, (p, off, keep_diag)
                    assert nslabs == (n + 15) // 16 and G >= 1 and chunk * G >= nslabs and chunk * (G - 1) < nslabs
                    assert G == 1 or G * k <= WGS
                    assert G > 1 or k == 0 or WGS // k < 2 or nslabs // 16 < 2      # (a split wherever the rule allows two)
    assert _viewcov(lib, 500, p, [0, p + 1], True)[0] == -1 and _viewcov(lib, 500, p, [1, p], True)[0] == -1       # the ends of off
    if p > 2:
        assert _viewcov(lib, 500, p, [0, 2, 2, p], True)[0] == -2 and _viewcov(lib, 500, p, [0, 2, 1, p], True)[0] == -2


@pytest.mark.parametrize("ntau", [1, 65, 66])
def test_lag_covariance_weights(lib, ntau):
    c = plans_shim.constants(lib)
    w = np.random.default_rng(ntau).standard_normal(ntau)
    out, nyG = np.full(ntau + 2 * c["LAGCOV_PADW"] + 3, 7.0), np.zeros(2, np.int32)
    k = lib.pl_lagcov_plan(700, 130, w.ctypes.data, ntau, out.ctypes.data, nyG.ctypes.data)
    assert c["LAGCOV_PADW"] == 15 and k == ntau + 30 and np.array_equal(out[:k], np.pad(w, 15)) and np.all(out[k:] == 7.0)
    assert nyG.tolist() == [3, 11]          # 3 column blocks of 64 in groups of 4: 3 tile pairs; min(11 row tiles, 512 // 3)


@pytest.mark.parametrize("h", [0, 1, 40])
def test_low_pass_weights(lib, h):
    c = plans_shim.constants(lib)
    w = np.random.default_rng(h).standard_normal(h + 1)
    out, nyG = np.full(2 * h + 1 + 2 * c["LOWPASS_PADW"] + 3, 7.0), np.zeros(2, np.int32)
    k = lib.pl_lowpass_plan(700, 130, w.ctypes.data, h, out.ctypes.data, nyG.ctypes.data)
    assert c["LOWPASS_PADW"] == 15 and k == 2 * h + 31 and np.array_equal(out[:k], np.pad(np.concatenate([w[:0:-1], w]), 15))
    assert np.all(out[k:] == 7.0) and nyG.tolist() == [6, 11]       # 3 (3 + 1) / 2 tile pairs; min(11 row tiles, 512 // 6)


# --------------------------------------------------------------------------- #
# 3. the plan of the complex driver (c64_plan)                                  #
# --------------------------------------------------------------------------- #
C64_FIELDS = ("status", "r", "l", "adaptive", "n_iter", "auto_count", "h", "LP", "ko", "Lo", "transposed", "small", "small_pad", "tall_pad",
              "big", "krylov", "nbmax", "ldk", "arena_bytes")
C64_OK, C64_SHARD_SIDE, C64_RANK, C64_WIDTH, C64_MASKED, C64_N_ITER = range(6)      # the order the driver reports the checks in


def c_c64(lib, n, p, k, n_oversamples=10, n_iter=-1, p_total=0, masked=False, p_valid=0, krylov_allowed=True):
    out = np.zeros(len(C64_FIELDS), np.int64)
    lib.pl_c64_plan(n, p, routes._up(n, 512), routes._up(p, 512), p_total, int(masked), p_valid, k, n_oversamples, n_iter,
                    int(krylov_allowed), out.ctypes.data)
    return dict(zip(C64_FIELDS, out.tolist()))


def _has(plan, **want):
    return {key: plan[key] for key in want} == want


def test_c64_plan_hand_cases(lib):
    """Values written out from the rules: r = min(n, features), l = min(k + oversamples, r), panels of 32 complex columns up to
    l = 32 and of 64 above, output panels of round_up(k, 16), scikit-learn's count 7 below k = 0.1 r and 4 from there,
    nb_fit = 384 // l blocks before a thick restart, nbmax = min(products + 1, nb_fit), block Krylov from one product and three
    blocks on.  A 300 x 900 field pads to 512 x 1024."""
    c = plans_shim.constants(lib)
    assert (c["KRYLOV_MAX_ORDER"], c["C64_IT_MIN"], c["C64_IT_CAP"]) == (384, 2, 20)
    # the panel width switches between l = 32 and l = 33 (k < 30: 7 products, 8 blocks of the 12 / 11 that fit)
    assert _has(c_c64(lib, 300, 900, 22), status=C64_OK, r=300, l=32, h=32, LP=64, ko=32, Lo=64, auto_count=7, n_iter=7, adaptive=0,
                transposed=1, small=300, small_pad=512, tall_pad=1024, big=1024, krylov=1, nbmax=8, ldk=512)
    assert _has(c_c64(lib, 300, 900, 23), status=C64_OK, l=33, h=64, LP=128, ko=32, Lo=64, n_iter=7, krylov=1, nbmax=8, ldk=1024)
    # scikit-learn's count on both sides of k < 0.1 r
    assert _has(c_c64(lib, 300, 900, 29), auto_count=7, n_iter=7, l=39, nbmax=8)
    assert _has(c_c64(lib, 300, 900, 30), auto_count=4, n_iter=4, l=40, nbmax=5, ldk=5 * 128)
    assert _has(c_c64(lib, 300, 900, 30, n_iter=9), auto_count=4, n_iter=9, nbmax=9)           # 384 // 40 = 9 < 10
    # the iteration codes
    assert _has(c_c64(lib, 300, 900, 6, n_iter=0), status=C64_OK, n_iter=0, krylov=0, nbmax=0, ldk=0, l=16, ko=16, Lo=32)
    assert _has(c_c64(lib, 300, 900, 6, n_iter=-2), status=C64_OK, adaptive=1, n_iter=20, auto_count=7, krylov=1, nbmax=21, ldk=21 * 64)
    assert c_c64(lib, 300, 900, 6, n_iter=-3)["status"] == C64_N_ITER
    # seven products: 8 blocks of 48 columns fit (no restart), of 49 columns only 7 (one restart)
    assert _has(c_c64(lib, 300, 900, 38, n_iter=7), status=C64_OK, l=48, krylov=1, nbmax=8)
    assert _has(c_c64(lib, 300, 900, 39, n_iter=7), status=C64_OK, l=49, krylov=1, nbmax=7)
    # the widest sketch
    assert _has(c_c64(lib, 300, 900, 54, n_iter=7), status=C64_OK, l=64, h=64, LP=128, ko=64, Lo=128, nbmax=6)
    assert _has(c_c64(lib, 300, 900, 55, n_iter=7), status=C64_WIDTH, l=65)
    assert _has(c_c64(lib, 300, 900, 60, n_oversamples=0), status=C64_OK, l=60)
    # more modes than rank; the sketch is cut to the rank
    assert _has(c_c64(lib, 20, 900, 21), status=C64_RANK, r=20)
    assert _has(c_c64(lib, 20, 900, 20), status=C64_OK, r=20, l=20, auto_count=4)
    # masked in place: the valid features count, and there must be more of them than samples
    assert _has(c_c64(lib, 300, 900, 6, masked=True, p_valid=301), status=C64_OK, r=300, transposed=1)
    assert c_c64(lib, 300, 900, 6, masked=True, p_valid=300)["status"] == C64_MASKED
    assert _has(c_c64(lib, 300, 900, 6, masked=True, p_valid=5), status=C64_RANK, r=5)
    # sharded: the features of all ranks count, the sketch sits on the sample side whatever the slice
    assert _has(c_c64(lib, 300, 100, 6, p_total=301), status=C64_OK, r=300, transposed=1, small=300, small_pad=512, tall_pad=512, big=512)
    assert c_c64(lib, 300, 100, 6, p_total=300)["status"] == C64_SHARD_SIDE
    assert _has(c_c64(lib, 300, 100, 6), status=C64_OK, r=100, transposed=0, small=100, small_pad=512, tall_pad=512)
    assert _has(c_c64(lib, 900, 300, 6), status=C64_OK, transposed=0, small=300, small_pad=512, tall_pad=1024, big=1024)
    # the subspace iteration on request
    assert _has(c_c64(lib, 300, 900, 6, krylov_allowed=False), status=C64_OK, n_iter=7, krylov=0, nbmax=0, ldk=0)


def test_c64_plan_on_a_sweep(lib):
    """Every accepted plan keeps the Rayleigh-Ritz problem within order 384, holds at least three blocks where the block Krylov
    recurrence runs (all of them, two, when one product is asked for), has panels of 64 or 128 real columns, and reserves what the formula restated here gives; the scratch of one
    pass of eofx_cmat_mul_f32 is its part of that formula."""
    rng = np.random.default_rng(384)
    up, scratch = routes._up, lib.pl_atb_scratch_bytes
    accepted = 0
    for _ in range(3000):
        n, p = (int(x) for x in rng.integers(1, 6000, 2))
        k, over, n_iter = int(rng.integers(1, 70)), int(rng.integers(0, 12)), int(rng.integers(-2, 22))
        pl = c_c64(lib, n, p, k, over, n_iter, krylov_allowed=bool(rng.integers(0, 4)))
        r = min(n, p)
        want = C64_RANK if k > r else C64_WIDTH if min(k + over, r) > 64 else C64_OK
        assert pl["status"] == want, (n, p, k, over, n_iter)
        if want != C64_OK:
            continue
        accepted += 1
        LP, Lo, nbmax, sp, tp, big = (pl[key] for key in ("LP", "Lo", "nbmax", "small_pad", "tall_pad", "big"))
        assert LP in (64, 128) and LP == 2 * pl["h"] and pl["l"] <= pl["h"] and nbmax * pl["l"] <= 384 and pl["ldk"] == nbmax * LP
        if pl["krylov"]:        # (a run of one product makes two blocks, Z_0 and Z_1, and is never short of room)
            assert 384 // pl["l"] >= 3 and (nbmax >= 3 or nbmax == pl["n_iter"] + 1 == 2), (n, p, k, over, n_iter)
        else:
            assert nbmax == 0
        n_pad, p_pad = up(n, 512), up(p, 512)
        passes = 2 * scratch(p_pad, up(n, 32), LP) + 2 * scratch(n_pad, up(p, 32), LP)
        need = (2 * sp + 2 * tp + 2 * big) * LP * 4 + (sp + tp) * Lo * 4 + passes
        need += (4 * lib.pl_gram_parts(big, LP) + 8) * LP * LP * 8 + big * (Lo + LP) * 4 + (8 << 20)
        if pl["krylov"]:
            need += nbmax * (2 * sp + tp) * LP * 4 + sp * LP * 4 + (3 + nbmax) * nbmax * LP * LP * 8 + (48 << 20)
        assert pl["arena_bytes"] == need, (n, p, k, over, n_iter)
        assert lib.pl_c64_mul_scratch_bytes(n, p, n_pad, p_pad, LP) == 4 * big * LP * 4 + (8 << 20) + passes
    assert accepted >= 1500


# --------------------------------------------------------------------------- #
# 4. the plans of the real drivers (rsvd_plan, cross_plan)                      #
# --------------------------------------------------------------------------- #
RSVD_FIELDS = ("status", "r", "l_req", "l", "L", "Lo", "n_iter", "transposed", "full_width")
CROSS_FIELDS = RSVD_FIELDS + ("tall", "small", "tall_pad", "small_pad", "gram_route", "arena_bytes")
RSVD_OK, RSVD_RANK, RSVD_WIDTH = range(3)       # the order the entries report the checks in
MAX_SKETCH = 256                                # EOFX_MAX_SKETCH (include/eofx.h)


def c_rsvd(lib, rows, cols, k, n_oversamples=10, n_iter=-1):
    out = np.zeros(len(RSVD_FIELDS), np.int64)
    lib.pl_rsvd_plan(rows, cols, k, n_oversamples, n_iter, out.ctypes.data)
    return dict(zip(RSVD_FIELDS, out.tolist()))


def c_cross(lib, n, p1, p2, k, n_oversamples=10, n_iter=-1, P1=None, P2=None, sharded=False, want_tsc=True, fast=(True, True),
            fast_scratch=(0, 0), no_gram=False):
    out = np.zeros(len(CROSS_FIELDS), np.int64)
    lib.pl_cross_plan(n, routes._up(n, 512), p1, routes._up(p1, 512), p2, routes._up(p2, 512), p1 if P1 is None else P1,
                      p2 if P2 is None else P2, int(sharded), int(want_tsc), int(fast[0]), int(fast[1]), fast_scratch[0], fast_scratch[1], k,
                      n_oversamples, n_iter, int(no_gram), out.ctypes.data)
    return dict(zip(CROSS_FIELDS, out.tolist()))


def null_repair(lib, rows_pad, Lo):
    """fix_null_columns' reservation as the drivers spelled it before null_repair_bytes"""
    return rows_pad * Lo * 4 + (lib.pl_gram_parts(rows_pad, Lo) + 4) * Lo * Lo * 8 + (64 << 10)


def rsvd_scratch(lib, tall_pad, small_pad, l, k):
    """rsvd_scratch_bytes as eofx_abi.hip spelled it before it moved into the header"""
    up, atb = routes._up, lib.pl_atb_scratch_bytes
    L, Lo, big = up(l, 32), up(k, 32), max(tall_pad, small_pad)
    b = 2 * small_pad * L * 4 + 2 * tall_pad * L * 4 + tall_pad * Lo * 4 + small_pad * Lo * 4
    b += atb(small_pad, tall_pad, L) + atb(tall_pad, small_pad, L) + atb(small_pad, tall_pad, Lo)
    b += (4 * lib.pl_gram_parts(big, L) + 8) * L * L * 8 + 2 * L * Lo * 8 + 4096 + big * (Lo + L) * 4
    if l > 64:
        Lb = up(l, 64)
        b += (2 * Lb * Lb + Lb * Lb // 2 + 64 * 64 + Lb) * 8 + 8192
    return b + (4 << 20)


def cross_arena(lib, n_pad, p1_pad, p2_pad, l, k, sharded, want_tsc, fast, fast_scratch, gram_route):
    """The arena of crosscov_impl as the driver sized it inline before cross_plan."""
    atb = lib.pl_atb_scratch_bytes
    L, pp = routes._up(l, 32), max(p1_pad, p2_pad)
    need = rsvd_scratch(lib, pp, pp, l, k) + n_pad * L * 4 * 2 + atb(n_pad, pp, L)
    if want_tsc:
        need += n_pad * n_pad * 4 * 2 + (1 << 20)
    need_gram = max(fast_scratch) + n_pad * L * 4 * 2 + atb(n_pad, n_pad, L) if all(fast) else 0
    need_plain = atb(n_pad, pp, n_pad) if want_tsc else 0
    if sharded:
        return need + null_repair(lib, pp, routes._up(k, 32)) + max(need_gram, need_plain)
    return need + (need_gram if gram_route else need_plain)


def test_rsvd_plan_hand_cases(lib):
    """r = min(rows, cols), l = min(k + oversamples, r), panels of round_up(l, 32) and round_up(k, 32) columns, scikit-learn's
    count 7 below k = 0.1 r and 4 from there, the transpose when there are fewer rows than columns."""
    assert c_rsvd(lib, 700, 60, 5) == dict(status=RSVD_OK, r=60, l_req=15, l=15, L=32, Lo=32, n_iter=7, transposed=0, full_width=0)
    assert c_rsvd(lib, 60, 700, 5) == dict(status=RSVD_OK, r=60, l_req=15, l=15, L=32, Lo=32, n_iter=7, transposed=1, full_width=0)
    # the sketch is cut to the rank and is then full width: l = r = 12
    assert c_rsvd(lib, 60, 12, 4) == dict(status=RSVD_OK, r=12, l_req=14, l=12, L=32, Lo=32, n_iter=4, transposed=0, full_width=1)
    assert _has(c_rsvd(lib, 60, 12, 2, n_oversamples=10), status=RSVD_OK, l_req=12, l=12, full_width=1)       # exactly the rank, unclamped
    assert _has(c_rsvd(lib, 60, 12, 1, n_oversamples=10), status=RSVD_OK, l=11, full_width=0)
    # more modes than rank; the rank is reported first
    assert _has(c_rsvd(lib, 60, 12, 13), status=RSVD_RANK, r=12)
    assert _has(c_rsvd(lib, 60, 12, 12), status=RSVD_OK, r=12, l=12)
    assert _has(c_rsvd(lib, 200, 300, 400, n_oversamples=0), status=RSVD_RANK, r=200)
    # the widest sketch
    assert _has(c_rsvd(lib, 900, 400, 246), status=RSVD_OK, l=256, L=256, Lo=256)
    assert _has(c_rsvd(lib, 900, 400, 247), status=RSVD_WIDTH, l=257)
    assert _has(c_rsvd(lib, 900, 256, 250), status=RSVD_OK, l=256, full_width=1)
    # an explicit count, zero included
    assert c_rsvd(lib, 700, 60, 5, n_iter=3)["n_iter"] == 3 and c_rsvd(lib, 700, 60, 5, n_iter=0)["n_iter"] == 0
    # the automatic count on both sides of k = 0.1 r (r = 60: k = 5 < 6 <= k = 6; r = 55: k = 5 < 5.5 < k = 6)
    assert [c_rsvd(lib, 700, 60, k)["n_iter"] for k in (5, 6, 7)] == [7, 4, 4]
    assert [c_rsvd(lib, 55, 700, k)["n_iter"] for k in (5, 6)] == [7, 4]
    # the sharded fit: (n, features over all ranks), so the sample count bounds the sketch
    assert _has(c_rsvd(lib, 120, 100000, 115), status=RSVD_OK, r=120, l_req=125, l=120, transposed=1, full_width=1, n_iter=4)


def test_rsvd_plan_on_a_sweep(lib):
    """l <= r; a clamped sketch is a full-width one (so eofx_rsvd_f32 needs no copy of the leading columns of omega: the identity
    replaces it); whole panels of 32 columns; and the two Python restatements of the rules (sharded.rsvd_auto_iters, the width
    sharded._resolve_sketch takes) agree with the header."""
    from xeofs_amd import sharded

    rng = np.random.default_rng(2275)
    seen = dict(clamped=0, full=0, rank=0, width=0)
    for _ in range(2500):
        rows, cols = (int(x) for x in rng.integers(1, 3000, 2))
        if rng.integers(0, 3) == 0:                 # small matrices: clamped sketches are common there
            rows, cols = (int(x) for x in rng.integers(1, 80, 2))
        k, over, n_iter = int(rng.integers(1, 300)), int(rng.integers(0, 12)), int(rng.integers(-1, 9))
        if rng.integers(0, 2):
            k = int(rng.integers(1, 40))
        pl = c_rsvd(lib, rows, cols, k, over, n_iter)
        r = min(rows, cols)
        want = RSVD_RANK if k > r else RSVD_WIDTH if min(k + over, r) > MAX_SKETCH else RSVD_OK
        assert pl["status"] == want and pl["r"] == r and pl["l_req"] == k + over, (rows, cols, k, over, n_iter)
        seen["rank"] += want == RSVD_RANK
        seen["width"] += want == RSVD_WIDTH
        assert pl["l"] <= r
        assert pl["l"] == pl["l_req"] or pl["full_width"], (rows, cols, k, over)
        assert pl["full_width"] == (pl["l"] == r) and pl["transposed"] == (rows < cols)
        assert pl["L"] % 32 == 0 and pl["L"] >= pl["l"] and pl["L"] - pl["l"] < 32 and pl["Lo"] == routes._up(k, 32)
        assert pl["n_iter"] == (sharded.rsvd_auto_iters(k, rows, cols) if n_iter < 0 else n_iter)
        seen["clamped"] += pl["l"] != pl["l_req"]
        seen["full"] += pl["full_width"]
        if want != RSVD_RANK:
            omega, l = sharded._resolve_sketch(k, r, over, np.zeros((r, k + over), np.float32), None)
            assert l == pl["l"] and omega.shape == (r, l)
    assert min(seen.values()) >= 50, seen


def test_null_repair_and_scratch_bytes(lib):
    rng = np.random.default_rng(2192)
    for _ in range(2000):
        rows_pad, Lo = 512 * int(rng.integers(1, 600)), 32 * int(rng.integers(1, 9))
        assert lib.pl_null_repair_bytes(rows_pad, Lo) == null_repair(lib, rows_pad, Lo)
    for _ in range(500):
        tp, sp = (512 * int(x) for x in rng.integers(1, 300, 2))
        l, k = int(rng.integers(1, 257)), int(rng.integers(1, 200))
        assert lib.pl_rsvd_scratch_bytes(tp, sp, l, k) == rsvd_scratch(lib, tp, sp, l, k), (tp, sp, l, k)


def test_cross_plan_hand_cases(lib):
    """300 samples pad to 512; 1300 and 900 features to 1536 and 1024.  The operator is C = X^T Y (p1 x p2), transposed when
    p1 < p2; the Gram route is this rank's wish when the total squared covariance is asked for, both fields are wider than long,
    both pass gram_fast_ok and the switch is off."""
    fs = (5 << 20, 3 << 20)
    pl = c_cross(lib, 300, 1300, 900, 6, fast_scratch=fs)
    assert _has(pl, status=RSVD_OK, r=900, l=16, L=32, Lo=32, n_iter=7, transposed=0, tall=1300, small=900, tall_pad=1536, small_pad=1024,
                gram_route=1)
    assert pl["arena_bytes"] == cross_arena(lib, 512, 1536, 1024, 16, 6, False, True, (True, True), fs, True)
    pl = c_cross(lib, 300, 900, 1300, 6, fast_scratch=fs)
    assert _has(pl, transposed=1, tall=1300, small=900, tall_pad=1536, small_pad=1024, gram_route=1)
    # every reason against the route
    assert c_cross(lib, 300, 1300, 900, 6, fast_scratch=fs, want_tsc=False)["gram_route"] == 0
    assert c_cross(lib, 300, 1300, 900, 6, fast_scratch=fs, no_gram=True)["gram_route"] == 0
    assert c_cross(lib, 300, 1300, 900, 6, fast=(True, False))["gram_route"] == 0
    assert c_cross(lib, 300, 1300, 900, 6, fast=(False, True))["gram_route"] == 0
    assert c_cross(lib, 300, 1300, 300, 6, fast_scratch=fs)["gram_route"] == 0 and c_cross(lib, 300, 1300, 301, 6, fast_scratch=fs)["gram_route"] == 1
    assert c_cross(lib, 300, 300, 1300, 6, fast_scratch=fs)["gram_route"] == 0
    assert c_cross(lib, 700, 50, 40, 6, fast_scratch=fs)["gram_route"] == 0
    # the valid (or global) counts rule: a masked first field with fewer valid features than the second turns the operator round
    assert _has(c_cross(lib, 300, 1300, 900, 6, P1=800), r=800, transposed=1, tall=900, small=1300, tall_pad=1024, small_pad=1536)
    assert _has(c_cross(lib, 300, 1300, 900, 6, P1=250), r=250, gram_route=0)
    # the checks, and the full-width sketch the driver answers with the identity
    assert _has(c_cross(lib, 80, 50, 40, 41), status=RSVD_RANK, r=40, arena_bytes=0)
    assert _has(c_cross(lib, 700, 400, 300, 250), status=RSVD_WIDTH, l=260, arena_bytes=0)
    assert _has(c_cross(lib, 80, 50, 40, 30), status=RSVD_OK, l=40, l_req=40, full_width=1)
    assert _has(c_cross(lib, 80, 50, 40, 31), status=RSVD_OK, l=40, l_req=41)       # the driver refuses a clamped sketch itself


def test_cross_plan_on_a_sweep(lib):
    """The reservation equals the formula the driver carried inline, the sharded one holds either route, and the Gram route is never
    wished for without the total squared covariance or with a field that is not wider than long."""
    rng = np.random.default_rng(3501)
    accepted = 0
    for _ in range(1500):
        n, p1, p2 = int(rng.integers(2, 3000)), int(rng.integers(1, 6000)), int(rng.integers(1, 6000))
        P1, P2 = (p if rng.integers(0, 3) else int(rng.integers(1, p + 1)) for p in (p1, p2))
        k, over, n_iter = int(rng.integers(1, 70)), int(rng.integers(0, 12)), int(rng.integers(-1, 9))
        fast = (bool(rng.integers(0, 4)), bool(rng.integers(0, 4)))
        fs = tuple(int(rng.integers(1, 1 << 28)) if all(fast) else 0 for _ in range(2))
        want_tsc, no_gram = bool(rng.integers(0, 3)), not rng.integers(0, 5)
        kw = dict(n_oversamples=over, n_iter=n_iter, P1=P1, P2=P2, want_tsc=want_tsc, fast=fast, fast_scratch=fs, no_gram=no_gram)
        loc, shd = c_cross(lib, n, p1, p2, k, sharded=False, **kw), c_cross(lib, n, p1, p2, k, sharded=True, **kw)
        assert {key: loc[key] for key in RSVD_FIELDS} == c_rsvd(lib, P1, P2, k, over, n_iter)
        assert loc["gram_route"] == shd["gram_route"] == int(want_tsc and n < P1 and n < P2 and all(fast) and not no_gram)
        if not want_tsc or n >= P1 or n >= P2:
            assert loc["gram_route"] == 0
        if loc["status"] != RSVD_OK:
            assert loc["arena_bytes"] == shd["arena_bytes"] == 0
            continue
        accepted += 1
        n_pad, pads = routes._up(n, 512), (routes._up(p1, 512), routes._up(p2, 512))
        assert (loc["tall_pad"], loc["small_pad"]) == (pads[::-1] if loc["transposed"] else pads)
        for pl, sharded in ((loc, False), (shd, True)):
            assert pl["arena_bytes"] == cross_arena(lib, n_pad, *pads, pl["l"], k, sharded, want_tsc, fast, fs, bool(pl["gram_route"]))
        # whichever route the vote of a sharded fit ends on, its arena holds what a local fit on that route reserves
        for route in (False, True):
            if route and not all(fast):
                continue
            assert shd["arena_bytes"] >= cross_arena(lib, n_pad, *pads, loc["l"], k, False, want_tsc, fast, fs, route)
    assert accepted >= 700


def test_fused_fit_eligible(lib):
    """fit_first_eligible plus: no more modes than samples, an unclamped sketch, a row of omega per sample, omega on the host."""
    ok = lambda **kw: lib.pl_fused_fit_eligible(*[{**dict(keep_raw=2, prec=PREC_F16X3, aligned=1, n=120, P=132, k=6, over=10, rows=120, dev=0),
                                                   **kw}[key] for key in ("keep_raw", "prec", "aligned", "n", "P", "k", "over", "rows", "dev")])
    assert ok() == 1 and ok(rows=500) == 1
    assert ok(rows=119) == 0 and ok(dev=1) == 0 and ok(keep_raw=1) == 0 and ok(aligned=0) == 0
    assert ok(over=26) == 0                 # l = 32: no spare column for the ones (fit_first_eligible)
    assert ok(k=115, over=10) == 0          # clamped to the 120 samples
    assert lib.pl_fit_first_eligible(2, PREC_F16X3, 1, 120, 132, 16) == 1
