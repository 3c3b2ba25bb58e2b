"""GPU tests of the block cross-covariance of multi-view CCA (csrc/eofx_viewcov.hpp, engine.viewcov).

The checker is numpy float64: Zc = Z - mean(Z), ref = Zc^T Zc / (n - 1) with the diagonal blocks zeroed.  Every output is a
float64 sum of n products of two float64 differences, so elementwise

    |err| <= (n + 6) 2^-53 (|Zc|^T |Zc|) / (n - 1)  +  n delta_i delta_j / (n - 1),    delta = n 2^-53 max|Z| per column:

a mean that is off by delta adds only the second term, because the first-order terms cancel.  (A split of the samples over G
workgroups sums at most n / 2 + 16 products per partial and G - 1 <= n / 256 partials: inside the same n + 6.)  Every case
runs twice and must be equal bit for bit, C == C^T bit for bit, and without keep_diag every entry of a diagonal block is
exactly 0.0.

Shapes against the kernel's tiles: slabs of 16 samples, tiles of 128 x 128 outputs, 64 x 64 per wave, 16 x 16 per
accumulator; the samples are split over workgroups from 32 slabs on (n >= 497) while the tiles are few.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
NS = [2, 3, 15, 16, 17, 63, 64, 65, 203]
OFFSETS = [[0, 1, 2], [0, 5, 70, 135], [0, 64, 128], [0, 63, 65, 130], [0, 200, 257], [0, 70, 71, 150], [0, 128, 256, 300]]


def panel(rng, n, p, shift=None):
    """columns of scales spread over [1e-3, 1, 30]; `shift`: unit-variance columns about that offset instead"""
    if shift is not None:
        return (rng.standard_normal((n, p)) + shift).astype(np.float32)
    return (rng.standard_normal((n, p)) * rng.choice([1e-3, 1.0, 30.0], (1, p)) + rng.standard_normal((1, p))).astype(np.float32)


def view_of(off):
    off = np.asarray(off)
    return np.repeat(np.arange(off.size - 1), np.diff(off))


def reference(Z, off, center=True, keep_diag=False):
    """-> (ref, bound, same-view mask)"""
    n = Z.shape[0]
    Z64 = Z.astype(np.float64)
    Zc = Z64 - Z64.mean(axis=0) if center else Z64
    ref = Zc.T @ Zc / (n - 1)
    bound = (n + 6) * U53 * (np.abs(Zc).T @ np.abs(Zc)) / (n - 1)
    if center:
        delta = n * U53 * np.abs(Z64).max(axis=0)
        bound = bound + n * np.outer(delta, delta) / (n - 1)
    v = view_of(off)
    same = v[:, None] == v[None, :]
    if not keep_diag:
        ref[same] = 0.0
        bound[same] = 0.0
    return ref, bound, same


def check(got, Z, off, center, keep_diag, what):
    ref, bound, same = reference(Z, off, center, keep_diag)
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert not np.isnan(got).any(), what
    assert np.array_equal(got, got.T), f"{what}: C != C^T"
    if not keep_diag:
        assert np.all(got[same] == 0.0) and not np.signbit(got[same]).any(), f"{what}: a diagonal block is not +0.0"
    err = np.abs(got - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"viewcov {what}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def run(ctx, Z, off, center=True, keep_diag=False, what=""):
    import torch

    from xeofs_amd import engine

    Zd = torch.from_numpy(Z).cuda()
    C = engine.viewcov(ctx, Zd, off, center=center, keep_diag=keep_diag)
    assert C.is_cuda and C.dtype == torch.float64
    got = C.cpu().numpy()
    check(got, Z, off, center, keep_diag, f"n={Z.shape[0]} off={off if len(off) < 8 else f'[{len(off) - 1} views]'} "
                                          f"center={center} keep_diag={keep_diag} {what}")
    assert np.array_equal(engine.viewcov(ctx, Zd, off, center=center, keep_diag=keep_diag).cpu().numpy(), got)      # bit-reproducible
    return got


@pytest.mark.parametrize("off", OFFSETS, ids=lambda o: "-".join(map(str, o)))
def test_viewcov_edges(ctx, off):
    """samples around the 16-sample slab and 64, view boundaries on and off the 16 / 64 / 128 column tiles, a tile and a
    wave's block wholly inside one view ([0, 200, 257]), a view one column wide between two wide ones; keep_diag and
    center alternate over the cases"""
    rng = np.random.default_rng(700 + sum(off))
    for i, n in enumerate(NS):
        Z = panel(rng, n, off[-1])
        run(ctx, Z, off, center=True, keep_diag=bool(i % 2))
    run(ctx, panel(rng, 65, off[-1]), off, center=False, keep_diag=False)
    run(ctx, panel(rng, 17, off[-1]), off, center=False, keep_diag=True)


def test_viewcov_centres_in_float64(ctx):
    """unit-variance columns about 1e4: a kernel that centred in float32, or not at all, is off by orders"""
    rng = np.random.default_rng(21)
    for off in ([0, 63, 65, 130], [0, 200, 257]):
        Z = panel(rng, 203, off[-1], shift=1e4)
        got = run(ctx, Z, off, what="offset 1e4")
        assert np.abs(got).max() < 2.0                                             # covariances of unit-variance columns


def test_viewcov_one_view_and_many_views(ctx):
    from xeofs_amd import engine

    rng = np.random.default_rng(22)
    Z = panel(rng, 65, 150)
    got = run(ctx, Z, [0, 150])                                                    # m = 1: nothing is wanted
    assert np.all(got == 0.0)
    full = run(ctx, Z, [0, 150], keep_diag=True)                                   # ... and the full covariance with keep_diag
    assert np.all(np.diag(full) > 0.0)
    assert engine.VIEWCOV_MMAX == 64
    widths = rng.integers(1, 4, engine.VIEWCOV_MMAX)
    off = np.concatenate([[0], np.cumsum(widths)]).tolist()
    for keep in (False, True):
        run(ctx, panel(rng, 64, off[-1]), off, keep_diag=keep)


def test_viewcov_either_side_of_the_sample_split(ctx):
    """31 slabs are one workgroup per tile, 32 slabs (n = 497) are split in two; 1100 samples in four; with three tiles and
    with fifteen"""
    rng = np.random.default_rng(23)
    for n in (496, 497, 1100):
        for off in ([0, 63, 65, 130], [0, 200, 450, 600]):
            for keep in (False, True):
                run(ctx, panel(rng, n, off[-1]), off, keep_diag=keep, what="split" if n >= 497 else "one workgroup per tile")


@pytest.mark.parametrize("keep_diag", [False, True])
def test_viewcov_at_the_limit(ctx, keep_diag):
    from xeofs_amd import engine

    assert engine.VIEWCOV_PMAX == 4096
    rng = np.random.default_rng(24)
    run(ctx, panel(rng, 130, 4096), [0, 1301, 1400, 4096], keep_diag=keep_diag, what="p = 4096")


@pytest.mark.parametrize("keep_diag", [False, True])
def test_viewcov_strided_views(ctx, keep_diag):
    """Z and `out` are windows of wider buffers whose padding holds NaN: a stray read poisons an output, a stray store
    overwrites a NaN"""
    import torch

    from xeofs_amd import engine

    rng = np.random.default_rng(25)
    for n, off, zoff, zpad, coff, cpad in [(203, [0, 63, 65, 130], 3, 7, 5, 9), (65, [0, 5, 17], 1, 2, 0, 1),
                                           (64, [0, 64, 128], 0, 1, 1, 1), (600, [0, 200, 257], 2, 5, 3, 4)]:
        p = off[-1]
        Z = panel(rng, n, p)
        Zw = np.full((n + 2, p + zpad), np.nan, dtype=np.float32)
        Zw[1:n + 1, zoff:zoff + p] = Z
        Zd = torch.from_numpy(Zw).cuda()[1:n + 1, zoff:zoff + p]
        assert Zd.stride(0) == p + zpad and not Zd.is_contiguous()
        Cw = torch.full((p + 2, p + cpad), float("nan"), dtype=torch.float64, device="cuda")
        out = Cw[1:p + 1, coff:coff + p]
        for rep in range(2):
            ret = engine.viewcov(ctx, Zd, off, keep_diag=keep_diag, out=out)
            assert ret.data_ptr() == out.data_ptr()
            host = Cw.cpu().numpy()
            got = host[1:p + 1, coff:coff + p]
            check(got, Z, off, True, keep_diag, f"views n={n} off={off} keep_diag={keep_diag}")
            mask = np.ones(host.shape, bool)
            mask[1:p + 1, coff:coff + p] = False
            assert np.all(np.isnan(host[mask])), "a store outside the output view"
            if rep == 0:
                first = got.copy()
        assert np.array_equal(first, got)


def test_viewcov_host_panel(ctx):
    from xeofs_amd import engine

    rng = np.random.default_rng(26)
    Z = panel(rng, 70, 29)
    got = engine.viewcov(ctx, Z, [0, 9, 29]).cpu().numpy()                         # a host panel is staged by the engine
    check(got, Z, [0, 9, 29], True, False, "host panel")


def test_viewcov_bad_arguments(ctx):
    import ctypes as C

    import torch

    from xeofs_amd import _lib, engine

    z = lambda r, c: torch.zeros((r, c), dtype=torch.float32, device="cuda")      # noqa: E731
    with pytest.raises(ValueError, match="n >= 2"):
        engine.viewcov(ctx, z(1, 4), [0, 2, 4])
    with pytest.raises(ValueError, match="p <= 4096"):
        engine.viewcov(ctx, z(4, 4097), [0, 2, 4097])
    with pytest.raises(ValueError, match="m <= 64"):
        engine.viewcov(ctx, z(4, 65), list(range(66)))
    for off in ([0, 2, 2, 4], [1, 2, 4], [0, 2, 3], [0, 3, 2, 4], [0]):
        with pytest.raises(ValueError, match="strictly increasing from 0 to p"):
            engine.viewcov(ctx, z(4, 4), off)
    with pytest.raises(ValueError, match="matrix"):
        engine.viewcov(ctx, torch.zeros((2, 3, 4), device="cuda"), [0, 4])
    with pytest.raises(ValueError, match="matrix"):
        engine.viewcov(ctx, np.zeros(5, np.float32), [0, 5])
    with pytest.raises(ValueError):
        engine.viewcov(ctx, z(4, 4), [0, 2, 4], out=torch.zeros((4, 5), dtype=torch.float64, device="cuda"))
    # the entry itself
    Z, Cm = z(8, 4), torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    off = np.array([0, 2, 4], dtype=np.int32)
    vp = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731

    def call(**kw):
        o = np.asarray(kw.get("off", off), dtype=np.int32)
        return ctx.lib.eofx_viewcov_f64(ctx.handle, vp(Z), kw.get("n", 8), kw.get("p", 4), kw.get("ld", 4), None,
                                        o.ctypes.data_as(C.c_void_p), kw.get("m", 2), 0, vp(Cm), kw.get("ldc", 4))

    assert call() == 0
    for kw in (dict(n=1), dict(ld=3), dict(ldc=3), dict(m=0), dict(p=0, ld=0, ldc=0), dict(off=[0, 2, 3]), dict(off=[0, 0, 4]),
               dict(off=[1, 2, 4])):
        assert call(**kw) == _lib.ERR_ARG, kw
    assert call(p=4097, ld=4097, ldc=4097) == _lib.ERR_SHAPE
    assert call(m=65, off=list(range(66))) == _lib.ERR_SHAPE
    with pytest.raises(ValueError, match="strictly increasing"):
        _lib.raise_for(call(off=[0, 0, 4]), ctx.handle)
