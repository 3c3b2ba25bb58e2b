"""GPU tests of the low-pass covariance kernels (csrc/eofx_lowpass.hpp, engine.lowpass_cov, engine.lowpass).

The checker is a float64 numpy restatement that does not use the kernel's form (a sliding window over mirrored indices):
the detrended panel is padded with numpy.pad(mode="reflect"), the taps are added one shifted slice at a time, the trend is
added back and R = Y^T Y is one matmul.

Tolerances are derived, not measured (U53 = 2^-53, the unit roundoff of float64).  Every Y[t, j] is 2 h + 1 fused
multiply-adds plus two operations with the trend on either side of the filter, every R[i, j] a sum of n products of such
values, so with Ybar[t, j] = sum_k |w_k| (|S[refl]| + |trend at refl|) + |trend at t| and B = Ybar^T Ybar

    |Y - ref| <= 2 (2 h + 4) U53 Ybar,        |R - ref| <= 2 (n + 2 (2 h + 4)) U53 B,

the margin 2 (the restatement rounds too) being the one the lag-covariance test uses.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the restatement
def restate(S, w, trend=None):
    """-> (Y, R, Ybar, B) in float64"""
    S = np.asarray(S, np.float64)
    n, p = S.shape
    h = len(w) - 1
    T = np.zeros((n, p))
    if trend is not None:
        # the line evaluated in extended precision and rounded once, as a fused multiply-add does: a float64 product b t
        # rounds relative to |b t|, which near a zero crossing of the line exceeds the |a + b t| the bounds are stated in
        ext = np.longdouble
        T = np.asarray(trend[0].astype(ext)[None, :] + trend[1].astype(ext)[None, :] * np.arange(n).astype(ext)[:, None], np.float64)
    Dp = np.pad(S - T, ((h, h), (0, 0)), mode="reflect")
    Ap = np.pad(np.abs(S) + np.abs(T), ((h, h), (0, 0)), mode="reflect")
    Y, Ybar = np.zeros((n, p)), np.zeros((n, p))
    for k in range(-h, h + 1):
        Y += w[abs(k)] * Dp[h + k:h + k + n]
        Ybar += abs(w[abs(k)]) * Ap[h + k:h + k + n]
    Y += T
    Ybar += np.abs(T)
    return Y, Y.T @ Y, Ybar, Ybar.T @ Ybar


def panel(rng, n, p, pad):
    """float32 device panel [n x p] with row stride p + pad, and a trend near (not at) its least-squares lines"""
    import torch

    from xeofs_amd.single.lfca import linear_trend

    slope = 0.02 * rng.standard_normal(p + pad)
    host = (rng.standard_normal((n, p + pad)) + slope * np.arange(n)[:, None] + rng.standard_normal(p + pad)).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    lo = pad // 2
    host = host[:, lo:lo + p]
    trend = linear_trend(host) * (1.0 + 0.3 * rng.standard_normal((2, p)))
    return host, dev[:, lo:lo + p], trend


def mixed_weights(rng, h):
    return rng.standard_normal(h + 1) * rng.choice([1e-3, 1.0, 10.0], h + 1)         # mixed sign and size, not only Lanczos


def check(ctx, rng, n, p, h, with_trend, pad=0, filtered=True):
    from xeofs_amd import engine

    host, dev, trend = panel(rng, n, p, pad)
    if pad:
        assert dev.stride(0) == p + pad
    if not with_trend:
        trend = None
    w = mixed_weights(rng, h)
    Yref, Rref, Ybar, B = restate(host, w, trend)
    tol_r = 2.0 * (n + 2 * (2 * h + 4)) * U53 * B
    tol_y = 2.0 * (2 * h + 4) * U53 * Ybar
    tag = f"lowpass n={n} p={p} h={h} trend={with_trend} pad={pad}"

    def check_r(R, what):
        assert R.dtype.is_floating_point and R.element_size() == 8 and tuple(R.shape) == (p, p) and R.is_cuda
        R = R.cpu().numpy()
        err = np.abs(R - Rref)
        worst = float((err / np.maximum(tol_r, 1e-300)).max())
        print(f"{tag} R ({what}): max err / bound = {worst:.3f}")
        assert np.all(err <= tol_r), (tag, what, worst)
        assert np.array_equal(R, R.T), (tag, what)                                 # symmetric bit for bit
        return R

    def check_y(Y, what):
        assert Y.element_size() == 8 and tuple(Y.shape) == (n, p) and Y.is_cuda and Y.is_contiguous()
        Y = Y.cpu().numpy()
        err = np.abs(Y - Yref)
        worst = float((err / np.maximum(tol_y, 1e-300)).max())
        print(f"{tag} Y ({what}): max err / bound = {worst:.3f}")
        assert np.all(err <= tol_y), (tag, what, worst)
        return Y

    R = check_r(engine.lowpass_cov(ctx, dev, w, trend), "alone")
    assert np.array_equal(engine.lowpass_cov(ctx, dev, w, trend).cpu().numpy(), R)  # bit-reproducible
    if filtered:
        R2, Y2 = engine.lowpass_cov(ctx, dev, w, trend, return_filtered=True)       # Y together with R
        R2, Y2 = check_r(R2, "with Y"), check_y(Y2, "with R")
        Y = check_y(engine.lowpass(ctx, dev, w, trend), "alone")
        assert np.array_equal(Y, Y2) and np.array_equal(R, R2)                       # one route: the same bits either way
        assert np.array_equal(engine.lowpass(ctx, dev, w, trend).cpu().numpy(), Y)
    return host, dev, R


# ------------------------------------------------------------------------------------------------ 1. route edges
@pytest.mark.parametrize("p", [1, 15, 16, 17, 64, 65, 100, 257])
def test_route_edges(ctx, p):
    """n = 203 is no multiple of the 64-row tile or the 16-row window; the engine exports no route switch (there is one
    route), so h takes 0 and 1, a window shorter and one longer than the 16 outputs of a thread (2 h + 1 = 15 | 17), one
    that spans a row tile (h = 40) and h = n - 1, the largest half-width one reflection covers"""
    rng = np.random.default_rng(200 + p)
    n = 203
    for h in (0, 1, 7, 8, 40, n - 1):
        for with_trend in (False, True):
            check(ctx, rng, n, p, h, with_trend)
    check(ctx, rng, n, p, 3, True, pad=7)                                            # ld > p, odd padding
    check(ctx, rng, n, p, 33, False, pad=5)


@pytest.mark.parametrize("h", [1, 40])
def test_smallest_sample_count(ctx, h):
    """n = h + 1: every output reads mirrored samples on both sides"""
    rng = np.random.default_rng(300 + h)
    for p in (1, 17, 65):
        for with_trend in (False, True):
            check(ctx, rng, h + 1, p, h, with_trend)


def test_many_tiles_per_workgroup(ctx):
    """p = 257 has 15 pairs of column blocks, so 34 row groups walk the 104 row tiles of n = 6605, three or four each;
    40000 x 20: 625 tiles over 512 row groups"""
    rng = np.random.default_rng(7)
    for h, with_trend in ((3, True), (33, False), (120, True)):
        check(ctx, rng, 6605, 257, h, with_trend, pad=3, filtered=(h == 3))
    check(ctx, rng, 40000, 20, 21, True)


def test_host_input(ctx):
    """a host panel (float64 here) is staged by the engine as float32"""
    from xeofs_amd import engine
    from xeofs_amd.single.lfca import lanczos_weights, linear_trend

    rng = np.random.default_rng(3)
    S = rng.standard_normal((300, 70)).astype(np.float32)
    w = lanczos_weights(24, 30)
    trend = linear_trend(S)
    Yref, Rref, Ybar, B = restate(S, w, trend)
    R = engine.lowpass_cov(ctx, S.astype(np.float64), w, trend).cpu().numpy()
    Y = engine.lowpass(ctx, S, w, trend).cpu().numpy()
    assert np.all(np.abs(R - Rref) <= 2.0 * (300 + 2 * 64) * U53 * B)
    assert np.all(np.abs(Y - Yref) <= 2.0 * 64 * U53 * Ybar)
    # weights and trend as device tensors
    import torch

    R2 = engine.lowpass_cov(ctx, S, torch.from_numpy(w).cuda(), torch.from_numpy(trend).cuda()).cpu().numpy()
    assert np.array_equal(R2, R)


def test_identity_filter(ctx):
    """h = 0, w = [1]: Y = S exactly, and R agrees with the lag covariance of lag 0 within the sum of the two bounds"""
    from xeofs_amd import engine

    rng = np.random.default_rng(11)
    for n, p in ((203, 100), (1000, 257)):
        host, dev, _ = panel(rng, n, p, 3)
        Y = engine.lowpass(ctx, dev, np.array([1.0])).cpu().numpy()
        assert np.array_equal(Y, host.astype(np.float64))
        R = engine.lowpass_cov(ctx, dev, np.array([1.0])).cpu().numpy()
        M = engine.lagcov(ctx, dev, np.array([1.0])).cpu().numpy()
        A = np.abs(host.astype(np.float64))
        B = A.T @ A
        tol = 2.0 * (n + 2 * 4) * U53 * B + 2.0 * (n + 1 + 2) * U53 * B
        worst = float((np.abs(R - M) / tol).max())
        print(f"identity n={n} p={p}: max |R - lagcov| / bound = {worst:.3f}")
        assert np.all(np.abs(R - M) <= tol)


def test_bad_arguments(ctx):
    import torch

    from xeofs_amd import engine

    S = torch.zeros((50, 8), dtype=torch.float32, device="cuda")
    for fn in (engine.lowpass_cov, engine.lowpass):
        for w in (np.ones(51), np.ones(0), np.ones((2, 2))):                         # h > n - 1, no weight, not a vector
            with pytest.raises(ValueError):
                fn(ctx, S, w)
        fn(ctx, S, np.ones(50))                                                      # h = n - 1 is the last valid one
        with pytest.raises(ValueError):
            fn(ctx, torch.zeros((50, engine.LAGCOV_PMAX + 1), dtype=torch.float32, device="cuda"), np.ones(2))
        with pytest.raises(ValueError):
            fn(ctx, torch.zeros(50, dtype=torch.float32, device="cuda"), np.ones(2))   # wrong rank
        with pytest.raises(ValueError):
            fn(ctx, torch.zeros((1, 8), dtype=torch.float32, device="cuda"), np.ones(1))    # n < 2
        for trend in (np.zeros((2, 7)), np.zeros(8), np.zeros((3, 8))):
            with pytest.raises(ValueError):
                fn(ctx, S, np.ones(3), trend)
