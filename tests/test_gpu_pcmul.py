"""GPU tests of the PC-space product (csrc/eofx_pcmul.hpp, engine.pcmul): Y = X M on the fp64 matrix cores.

The checker is X.astype(float64) @ M in numpy.  Every output is a chain of a fused multiply-adds in float64, so
|err| <= (a + 2) 2^-53 (|X| @ |M|) elementwise (the checker's own blocked sum is inside the + 2), plus 2^-24 |Y| where the
output is rounded to float32.  Every case runs twice and must be equal bit for bit.
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53, U24 = 2.0 ** -53, 2.0 ** -24
ROWS = [1, 63, 64, 65, 203]
A = [1, 3, 4, 5, 63, 64, 65, 257]
B = [1, 15, 16, 17, 64, 65, 257]


def operands(rng, rows, a, b, xdt):
    X = (rng.standard_normal((rows, a)) * rng.choice([1e-3, 1.0, 30.0], (1, a))).astype(xdt)
    M = rng.standard_normal((a, b)) * rng.choice([1e-2, 1.0, 10.0], (a, 1))
    return X, M


def check(ctx, X, M, got, ydt, what):
    ref = X.astype(np.float64) @ M
    bound = (X.shape[1] + 2) * U53 * (np.abs(X).astype(np.float64) @ np.abs(M))
    if ydt == np.float32:
        bound = bound + U24 * np.abs(ref)
    assert got.shape == ref.shape and got.dtype == ydt, what
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"pcmul {what}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def run(ctx, rng, rows, a, b, xdt, ydt, m_on_device=False):
    import torch

    from xeofs_amd import engine

    X, M = operands(rng, rows, a, b, xdt)
    Xd = torch.from_numpy(X).cuda()
    Md = torch.from_numpy(M).cuda() if m_on_device else M
    tdt = torch.float32 if ydt == np.float32 else torch.float64
    Y = engine.pcmul(ctx, Xd, Md, tdt)
    assert Y.is_cuda and Y.dtype == tdt
    got = Y.cpu().numpy()
    check(ctx, X, M, got, ydt, f"rows={rows} a={a} b={b} {np.dtype(xdt).name}->{np.dtype(ydt).name} M on {'device' if m_on_device else 'host'}")
    assert np.array_equal(engine.pcmul(ctx, Xd, Md, tdt).cpu().numpy(), got)      # bit-reproducible


@pytest.mark.parametrize("a", A)
def test_pcmul_edges(ctx, a):
    """rows around the 64-row tile, a around the 4-wide matrix-core step and the 16-wide slab, b around the 16-column block,
    the 64-column wave block and the 256-column workgroup; both input and both output types, M on either side"""
    rng = np.random.default_rng(500 + a)
    i = 0
    for rows in ROWS:
        for b in B:
            xdt = (np.float32, np.float64)[i % 2]
            ydt = (np.float64, np.float32)[(i // 2) % 2]
            run(ctx, rng, rows, a, b, xdt, ydt, m_on_device=bool((i // 4) % 2))
            i += 1


@pytest.mark.parametrize("xdt", [np.float32, np.float64])
@pytest.mark.parametrize("ydt", [np.float32, np.float64])
def test_pcmul_every_type_pair(ctx, xdt, ydt):
    rng = np.random.default_rng(11)
    for m_on_device in (False, True):
        run(ctx, rng, 203, 65, 257, xdt, ydt, m_on_device)
        run(ctx, rng, 65, 5, 17, xdt, ydt, m_on_device)


def test_pcmul_at_the_limits(ctx):
    from xeofs_amd import engine

    assert (engine.PCMUL_AMAX, engine.PCMUL_BMAX) == (1024, 2048)
    rng = np.random.default_rng(12)
    run(ctx, rng, 130, 1024, 2048, np.float32, np.float64)
    run(ctx, rng, 130, 1024, 2048, np.float64, np.float32, m_on_device=True)


@pytest.mark.parametrize("xdt,ydt", [(np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32),
                                     (np.float64, np.float64)])
def test_pcmul_strided_views(ctx, xdt, ydt):
    """ldx > a, ldy > b and column-offset views of wider buffers whose padding holds NaN: a stray read poisons an output,
    a stray store overwrites a NaN"""
    import torch

    from xeofs_amd import engine

    rng = np.random.default_rng(13)
    for rows, a, b, xoff, xpad, yoff, ypad in [(203, 65, 257, 3, 7, 5, 9), (65, 17, 15, 1, 2, 0, 1), (64, 64, 64, 0, 1, 1, 1)]:
        X, M = operands(rng, rows, a, b, xdt)
        Xw = np.full((rows + 2, a + xpad), np.nan, dtype=xdt)
        Xw[1:rows + 1, xoff:xoff + a] = X
        Xd = torch.from_numpy(Xw).cuda()[1:rows + 1, xoff:xoff + a]
        assert Xd.stride(0) == a + xpad and not Xd.is_contiguous()
        Yw = torch.full((rows + 2, b + ypad), float("nan"), dtype=torch.float32 if ydt == np.float32 else torch.float64,
                        device="cuda")
        out = Yw[1:rows + 1, yoff:yoff + b]
        for _ in range(2):
            ret = engine.pcmul(ctx, Xd, M, out=out)
            assert ret.data_ptr() == out.data_ptr()
            host = Yw.cpu().numpy()
            got = host[1:rows + 1, yoff:yoff + b]
            check(ctx, X, M, got, ydt, f"views rows={rows} a={a} b={b} {np.dtype(xdt).name}->{np.dtype(ydt).name}")
            mask = np.ones(host.shape, bool)
            mask[1:rows + 1, yoff:yoff + b] = False
            assert np.all(np.isnan(host[mask])), "a store outside the output view"
            if _ == 0:
                first = got.copy()
        assert np.array_equal(first, got)


def test_pcmul_host_panel_and_zero_rows(ctx):
    import torch

    from xeofs_amd import engine

    rng = np.random.default_rng(14)
    X, M = operands(rng, 70, 9, 20, np.float32)
    got = engine.pcmul(ctx, X, M).cpu().numpy()                                   # a host panel is staged by the engine
    check(ctx, X, M, got, np.float64, "host panel")
    for tdt in (torch.float32, torch.float64):
        Y = engine.pcmul(ctx, torch.empty((0, 9), dtype=torch.float32, device="cuda"), M, tdt)
        assert tuple(Y.shape) == (0, 20) and Y.dtype == tdt
    # zero rows with a live output buffer: nothing is written
    Yw = torch.full((4, 20), float("nan"), dtype=torch.float64, device="cuda")
    Xd = torch.zeros((4, 9), dtype=torch.float32, device="cuda")
    rc = ctx.lib.eofx_pcmul_f64(ctx.handle, C.c_void_p(Xd.data_ptr()), 0, 0, 9, 9, M.ctypes.data_as(C.c_void_p), 20,
                                C.c_void_p(Yw.data_ptr()), 1, 20)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(Yw).all())


def test_pcmul_bad_arguments(ctx):
    import torch

    from xeofs_amd import _lib, engine

    z = lambda r, c, dt=torch.float32: torch.zeros((r, c), dtype=dt, device="cuda")      # noqa: E731
    with pytest.raises(ValueError, match="a <= 1024"):
        engine.pcmul(ctx, z(8, 1025), np.zeros((1025, 4)))
    with pytest.raises(ValueError, match="b <= 2048"):
        engine.pcmul(ctx, z(8, 4), np.zeros((4, 2049)))
    with pytest.raises(ValueError):
        engine.pcmul(ctx, z(8, 4), np.zeros((5, 4)))                              # inner lengths differ
    with pytest.raises(ValueError):
        engine.pcmul(ctx, z(8, 4), np.zeros((4, 4)), out=z(8, 5))                  # out of another shape
    with pytest.raises(ValueError):
        engine.pcmul(ctx, z(8, 4), np.zeros((4, 4)), torch.float16)
    # the entry itself: ldx < a, ldy < b, unknown type codes, a < 1, rows < 0
    X, Y, M = z(8, 4), z(8, 4, torch.float64), np.zeros((4, 4))
    vp = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    mp = M.ctypes.data_as(C.c_void_p)
    call = lambda **kw: ctx.lib.eofx_pcmul_f64(ctx.handle, vp(X), kw.get("xd", 0), kw.get("rows", 8), kw.get("a", 4),  # noqa: E731
                                               kw.get("ldx", 4), mp, kw.get("b", 4), vp(Y), kw.get("yd", 1), kw.get("ldy", 4))
    assert call() == 0
    for kw in (dict(ldx=3), dict(ldy=3), dict(xd=2), dict(yd=-1), dict(a=0), dict(b=0), dict(rows=-1)):
        assert call(**kw) == _lib.ERR_ARG, kw
    assert call(a=1025, ldx=1025) == _lib.ERR_SHAPE and call(b=2049, ldy=2049) == _lib.ERR_SHAPE
    with pytest.raises(ValueError, match="ldx >= a"):
        _lib.raise_for(call(ldx=3), ctx.handle)
