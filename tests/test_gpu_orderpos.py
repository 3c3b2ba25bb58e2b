"""GPU tests of the rank-order kernel (engine.order_positions, eofx_orderpos_f32, csrc/eofx_orderpos.hpp).

The outputs are integers, or one float64 product of an integer rounded once, so every comparison is EXACT: Qi equals the
restatement of tests/trend_reference.py (numpy's stable argsort after the -0.0 / NaN normalisation; itself checked against a
brute-force rank count in tests/test_trend_reference_cpu.py), and Zt equals np.float32((q - (n - 1) / 2) * scale), the
product formed in float64, bit for bit -- the sign of a zero included.

Lengths: each tier of the kernel (threads per series m / 8 up to m = 2048, 512 threads at m = 4096, 1024 threads at m = 8192
and 16384), its power-of-two edge and one past it.  Every output is a view with a row stride above n into a buffer filled
with a sentinel, which must survive past column n of every row and past row p.
"""

import ctypes as C

import numpy as np
import pytest

import trend_reference as tr

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 8192, 10000, 16383, 16384]
Q_SENTINEL, Z_SENTINEL = -7, 12345.0
NAN_POS = np.frombuffer(np.uint32(0x7fc00001).tobytes(), np.float32)[0]
NAN_NEG = np.frombuffer(np.uint32(0xffc00000).tobytes(), np.float32)[0]


def series(kind, n, rng):
    """one float32 series of n samples of the kind `kind` (0 .. 9)"""
    t = np.arange(n, dtype=np.float32)
    if kind == 0:
        return rng.standard_normal(n).astype(np.float32)
    if kind == 1:
        return np.full(n, 2.5, np.float32)                                  # constant: Q is the identity
    if kind == 2:
        return rng.integers(0, 2, n).astype(np.float32)                     # two values
    if kind == 3:
        return -t                                                           # strictly descending
    if kind == 4:
        return t * np.float32(0.25) - 3.0                                   # already sorted
    if kind == 5:
        return np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)  # +0 and -0 mixed: all equal
    if kind == 6:
        return np.float32(rng.integers(-3, 4, n) * 1.401298464324817e-45)   # denormals, with ties and zeros
    if kind == 7:
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.2] = np.inf
        x[rng.random(n) < 0.2] = -np.inf
        return x
    if kind == 8:
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.1] = np.inf
        x[rng.random(n) < 0.15] = NAN_POS
        x[rng.random(n) < 0.15] = NAN_NEG
        x[rng.random(n) < 0.1] = -0.0
        return x
    x = np.full(n, -1.0, np.float32)                                        # every value equal except one
    x[n // 2] = -7.0
    return x


def panel(p, n, seed, first_kind=0):
    rng = np.random.default_rng(seed)
    return np.stack([series((first_kind + j) % 10, n, rng) for j in range(p)])


def scales(p, seed):
    """(name, scale) pairs: NULL, ones, non-powers of two, and zeros among them"""
    rng = np.random.default_rng(seed)
    odd = rng.random(p) * 2.7 + 1.0 / 3.0
    zero = odd.copy()
    zero[::2] = 0.0
    return [("null", None), ("ones", np.ones(p)), ("odd", odd), ("zero", zero)]


def sentinel_views(torch, p, n, pad_q, pad_z, device):
    qbuf = torch.full((p + 2, n + pad_q), Q_SENTINEL, dtype=torch.int32, device=device)
    zbuf = torch.full((p + 2, n + pad_z), Z_SENTINEL, dtype=torch.float32, device=device)
    return qbuf, zbuf, qbuf[:p, :n], zbuf[:p, :n]


def assert_canaries(qbuf, zbuf, p, n):
    assert bool((qbuf[:p, n:] == Q_SENTINEL).all()) and bool((qbuf[p:] == Q_SENTINEL).all()), "Qi written outside [p x n]"
    assert bool((zbuf[:p, n:] == Z_SENTINEL).all()) and bool((zbuf[p:] == Z_SENTINEL).all()), "Zt written outside [p x n]"


def assert_exact(q, z, T, scale):
    """q, z: device outputs (or None); T the host panel"""
    p, n = T.shape
    Qref = tr.order_positions(T)
    if q is not None:
        got = q.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (p, n)
        bad = np.argwhere(got != Qref)
        assert bad.size == 0, f"Qi differs at {len(bad)} places, first (series, position) = {bad[0]}"
    if z is not None:
        got = z.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (p, n)
        want = tr.rank_values(Qref, scale)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"Zt differs in bits at {len(bad)} places, first = {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.parametrize("p", [1, 7])
@pytest.mark.parametrize("n", LENGTHS)
def test_every_tier_strided_with_canaries(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T = panel(p, n, 1000 * p + n, first_kind=n % 10)
    Tbuf = torch.full((p, n + 5), float("nan"), dtype=torch.float32, device=dev)          # ld > n; NaNs past column n
    Tbuf[:, :n] = torch.from_numpy(T)
    name, scale = scales(p, n)[(n + p) % 4]
    qbuf, zbuf, qv, zv = sentinel_views(torch, p, n, 3, 9, dev)
    q, z = engine.order_positions(ctx, Tbuf[:, :n], scale, want="both", out=(qv, zv))
    assert q.data_ptr() == qv.data_ptr() and z.data_ptr() == zv.data_ptr()
    assert_exact(q, z, T, scale)
    assert_canaries(qbuf, zbuf, p, n)
    assert bool(torch.isnan(Tbuf[:, n:]).all())                                            # the input is read only


@pytest.mark.parametrize("n", [3, 65, 257, 1025, 4097, 10000])
def test_every_kind_of_series_and_every_scale(ctx, n):
    import torch
    from xeofs_amd import engine

    T = panel(10, n, 77 + n)
    Td = torch.from_numpy(T).to(f"cuda:{ctx.device}")
    Qref = tr.order_positions(T)
    assert np.array_equal(Qref[1], np.arange(n)) and np.array_equal(Qref[5], np.arange(n))           # constant, +-0: identity
    assert np.array_equal(Qref[3], np.arange(n)[::-1]) and np.array_equal(Qref[4], np.arange(n))
    for name, scale in scales(10, n):
        q, z = engine.order_positions(ctx, Td, scale, want="both")
        assert_exact(q, z, T, scale)
    sd = torch.from_numpy(scales(10, n)[2][1]).to(Td.device)                                          # a device scale vector
    assert_exact(None, engine.order_positions(ctx, Td, sd), T, scales(10, n)[2][1])


def test_want_combinations_host_input_and_two_runs(ctx):
    import torch
    from xeofs_amd import engine

    p, n = 7, 300
    T = panel(p, n, 5, first_kind=6)
    scale = scales(p, 1)[2][1]
    z = engine.order_positions(ctx, T, scale)                        # a host panel, want="z" by default
    q = engine.order_positions(ctx, T, want="q")
    both = engine.order_positions(ctx, T, scale, want="both")
    assert isinstance(z, torch.Tensor) and z.dtype == torch.float32 and q.dtype == torch.int32 and len(both) == 2
    assert_exact(q, z, T, scale)
    assert_exact(both[0], both[1], T, scale)
    dev = f"cuda:{ctx.device}"
    for want in ("q", "z"):                                          # one output into a caller's strided view, the other absent
        qbuf, zbuf, qv, zv = sentinel_views(torch, p, n, 4, 4, dev)
        r = engine.order_positions(ctx, T, scale, want=want, out=qv if want == "q" else zv)
        assert_exact(r if want == "q" else None, r if want == "z" else None, T, scale)
        if want == "q":
            assert bool((zbuf == Z_SENTINEL).all())
        else:
            assert bool((qbuf == Q_SENTINEL).all())
        assert_canaries(qbuf, zbuf, p, n)
    again = engine.order_positions(ctx, T, scale, want="both")
    assert torch.equal(again[0], both[0]) and torch.equal(again[1].view(torch.int32), both[1].view(torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        engine.order_positions(ctx, T, want="q", out=torch.empty((p, n), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        engine.order_positions(ctx, T, want="z", out=torch.empty((n, p), dtype=torch.float32, device=dev).t())
    with pytest.raises(ValueError, match="one entry per series"):
        engine.order_positions(ctx, T, np.ones(p + 1))
    with pytest.raises(ValueError, match="matrix"):
        engine.order_positions(ctx, T[0])


@pytest.mark.parametrize("n,per_cu,spb", [(5, 8, 256), (1025, 8, 1)])
def test_more_series_than_the_grid_holds(ctx, n, per_cu, spb):
    """a workgroup loops over its groups of series: p above (CUs x workgroups per CU x series per workgroup)"""
    import torch
    from xeofs_amd import engine

    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    p = cus * per_cu * spb + 2 * spb + 3
    rng = np.random.default_rng(n)
    T = rng.integers(-4, 5, (p, n)).astype(np.float32)               # many ties
    T[rng.random((p, n)) < 0.05] = np.nan
    scale = rng.random(p) + 0.25
    q, z = engine.order_positions(ctx, T, scale, want="both")
    assert_exact(q, z, T, scale)


def test_refusals_before_any_launch(ctx):
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    dev = f"cuda:{ctx.device}"
    T = torch.zeros((2, 16385), dtype=torch.float32, device=dev)
    qbuf = torch.full((2, 16385), Q_SENTINEL, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="16384"):
        engine.order_positions(ctx, T, want="q", out=qbuf)
    assert bool((qbuf == Q_SENTINEL).all())
    lib, h = ctx.lib, ctx.handle
    T = torch.zeros((3, 40), dtype=torch.float32, device=dev)
    q = torch.full((3, 40), Q_SENTINEL, dtype=torch.int32, device=dev)
    z = torch.full((3, 40), Z_SENTINEL, dtype=torch.float32, device=dev)
    call = lambda n, ld, qp, ldq, zp, ldz, p=3: lib.eofx_orderpos_f32(h, ptr(T), p, n, ld, None, qp, ldq, zp, ldz)
    assert call(40, 39, ptr(q), 40, ptr(z), 40) == _lib.ERR_ARG                     # ld < n
    assert call(40, 40, ptr(q), 39, ptr(z), 40) == _lib.ERR_ARG                     # ldq < n
    assert call(40, 40, ptr(q), 40, ptr(z), 39) == _lib.ERR_ARG                     # ldz < n
    assert call(40, 40, None, 0, None, 0) == _lib.ERR_ARG                           # both outputs NULL
    assert call(0, 40, ptr(q), 40, ptr(z), 40) == _lib.ERR_ARG                      # n < 1
    assert call(16385, 16385, ptr(q), 16385, ptr(z), 16385) == _lib.ERR_SHAPE       # past the LDS of a CU
    assert b"16384" in lib.eofx_last_error(h)
    assert call(40, 40, ptr(q), 40, ptr(z), 40, p=0) == _lib.EOFX_OK                # p == 0: a no-op
    assert call(40, 40, None, 0, ptr(z), 0, p=0) == _lib.ERR_ARG                    # ... after the argument checks
    ctx.synchronize()
    assert bool((q == Q_SENTINEL).all()) and bool((z == Z_SENTINEL).all())
    empty = engine.order_positions(ctx, torch.zeros((0, 12), dtype=torch.float32, device=dev), want="both")
    assert tuple(empty[0].shape) == (0, 12) and tuple(empty[1].shape) == (0, 12)
