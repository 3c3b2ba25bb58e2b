"""GPU tests of the slab-product operator of spectral EOF analysis (engine.slabmul; csrc/eofx_spectral.hpp):
out[f] = W[f] R[f] in float32 of the batches W [nb x q x r] and R [nb x r x p], against float64.

The bound is the fma-chain bound of a float32 chain of r terms, per element:

    |out[f, m, j] - out64[f, m, j]| <= r 2^-24 sum_i |W[f, m, i]| |R[f, i, j]|

Shapes: the two kernels (8 accumulators for q <= 8, 16 beyond: q 1, 6, 8, 9, 16), the block of 512 features with two per thread
(p 1, 255, 256, 257, 511, 512, 513, 1100), rows 1 .. 130.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q_LIST = [1, 6, 8, 9, 16]
R_LIST = [1, 2, 28, 65, 130]
P_LIST = [1, 255, 256, 257, 511, 512, 513, 1100]
SENTINEL = -12345.678


def operands(torch, dev, nb, q, r, p, seed=0):
    g = torch.Generator(device="cpu").manual_seed(10000 * q + 100 * r + p + seed)
    W = torch.randn((nb, q, r), generator=g, dtype=torch.float32)
    R = torch.randn((nb, r, p), generator=g, dtype=torch.float32)
    return W.to(dev), R.to(dev)


def reference(torch, W, R):
    return W.double() @ R.double(), W.shape[2] * 2.0 ** -24 * (W.double().abs() @ R.double().abs())


def assert_within(torch, out, ref, bound, what=""):
    assert out.dtype == torch.float32 and out.shape == ref.shape
    err = (out.double() - ref).abs()
    bad = torch.nonzero(~(err <= bound))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert len(bad) == 0, f"{what}: {len(bad)} elements outside the bound, first {bad[0].tolist()}"


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("r", R_LIST)
def test_random_operands_at_every_edge(ctx, r):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    W, R = operands(torch, dev, 3, max(Q_LIST), r, max(P_LIST))
    for p in P_LIST:
        Rp = R[:, :, :p].contiguous()
        for q in Q_LIST:
            Wq = W[:, :q].contiguous()
            ref, bound = reference(torch, Wq, Rp)
            out = engine.slabmul(ctx, Wq, Rp)
            assert tuple(out.shape) == (3, q, p) and out.is_cuda
            assert_within(torch, out, ref, bound, f"r={r} p={p} q={q}")


def test_the_largest_slab_and_a_chain_in_order(ctx):
    """r = SLABMUL_RMAX fills the LDS image; every element is the fmaf chain over the rows ascending, bit for bit"""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    W, R = operands(torch, dev, 2, 16, engine.ROWGRAM_RMAX, 700)
    ref, bound = reference(torch, W, R)
    out = engine.slabmul(ctx, W, R)
    assert_within(torch, out, ref, bound, "r = 512")
    Wh, Rh = W.cpu().numpy(), R.cpu().numpy()
    for f, m, j in [(0, 0, 0), (1, 15, 699), (0, 7, 256), (1, 8, 511)]:
        acc = np.float32(0.0)
        for i in range(Wh.shape[2]):
            acc = np.float32(np.float64(Wh[f, m, i]) * np.float64(Rh[f, i, j]) + np.float64(acc))     # one rounding: an fma
        assert acc == out[f, m, j].item(), (f, m, j)


@pytest.mark.parametrize("q,r,p", [(1, 1, 1), (6, 28, 513), (16, 130, 257), (9, 65, 1100)])
def test_small_integers_bit_for_bit(ctx, q, r, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    g = torch.Generator(device="cpu").manual_seed(q + r + p)
    W = torch.randint(-8, 9, (3, q, r), generator=g).float().to(dev)
    R = torch.randint(-8, 9, (3, r, p), generator=g).float().to(dev)
    ref, _ = reference(torch, W, R)
    assert torch.equal(engine.slabmul(ctx, W, R).double(), ref)


@pytest.mark.parametrize("q,r,p,nb", [(1, 1, 1, 1), (6, 28, 513, 3), (9, 3, 255, 2)])
def test_canaries_reruns_and_read_only_operands(ctx, q, r, p, nb):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    W, R = operands(torch, dev, nb, q, r, p)
    Wc, Rc = W.clone(), R.clone()
    pad, m = 2048, nb * q * p
    buf = torch.full((2 * pad + m,), SENTINEL, dtype=torch.float32, device=dev)
    o = buf[pad:pad + m].view(nb, q, p)
    out = engine.slabmul(ctx, W, R, out=o)
    assert out.data_ptr() == o.data_ptr()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + m:] == SENTINEL).all())
    assert torch.equal(bits(out), bits(engine.slabmul(ctx, W, R)))
    assert torch.equal(W, Wc) and torch.equal(R, Rc)
    assert torch.equal(bits(out), bits(engine.slabmul(ctx, W.cpu().numpy(), R.cpu().numpy())))      # host arrays are staged
    for f in range(nb):                                                     # a slab does not depend on its batch
        assert torch.equal(bits(out[f]), bits(engine.slabmul(ctx, W[f:f + 1], R[f:f + 1])[0]))


def test_a_bad_column_stays_in_its_column(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    W, R = operands(torch, dev, 2, 6, 28, 600)
    clean = engine.slabmul(ctx, W, R)
    Rb = R.clone()
    Rb[0, 3, 17] = float("nan")
    Rb[1, 27, 599] = float("inf")
    out = engine.slabmul(ctx, W, Rb)
    keep = torch.ones((2, 600), dtype=torch.bool, device=dev)
    keep[0, 17] = keep[1, 599] = False
    same = bits(out) == bits(clean)
    assert bool(same.permute(0, 2, 1)[keep].all())
    assert bool(torch.isnan(out[0, :, 17]).all()) and bool((~torch.isfinite(out[1, :, 599])).all())


def test_refusals(ctx):
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    dev = f"cuda:{ctx.device}"
    lib, h = ctx.lib, ctx.handle
    W = torch.zeros((2, 4, 3), dtype=torch.float32, device=dev)
    R = torch.zeros((2, 3, 10), dtype=torch.float32, device=dev)
    o = torch.full((2, 4, 10), SENTINEL, dtype=torch.float32, device=dev)
    call = lambda nb=2, q=4, r=3, p=10: lib.eofx_slabmul_f32(h, ptr(W), ptr(R), nb, q, r, p, ptr(o))
    assert call(q=engine.SLABMUL_QMAX + 1) == _lib.ERR_SHAPE and b"rows of W" in lib.eofx_last_error(h)
    assert call(r=engine.ROWGRAM_RMAX + 1) == _lib.ERR_SHAPE and b"slabs of at most" in lib.eofx_last_error(h)
    assert call(nb=engine.SPECTRAL_NBMAX + 1) == _lib.ERR_SHAPE
    assert call(q=0) == _lib.ERR_ARG and call(r=0) == _lib.ERR_ARG and call(nb=-1) == _lib.ERR_ARG and call(p=-1) == _lib.ERR_ARG
    assert call(nb=0) == _lib.EOFX_OK and call(p=0) == _lib.EOFX_OK
    assert lib.eofx_slabmul_f32(h, None, ptr(R), 2, 4, 3, 10, ptr(o)) == _lib.ERR_ARG
    assert lib.eofx_slabmul_f32(h, ptr(W), None, 2, 4, 3, 10, ptr(o)) == _lib.ERR_ARG
    assert lib.eofx_slabmul_f32(h, ptr(W), ptr(R), 2, 4, 3, 10, None) == _lib.ERR_ARG
    assert lib.eofx_slabmul_f32(None, ptr(W), ptr(R), 2, 4, 3, 10, ptr(o)) == _lib.ERR_ARG
    ctx.synchronize()
    assert bool((o == SENTINEL).all())
    with pytest.raises(ValueError, match="W must have shape"):
        engine.slabmul(ctx, W[:, :, :2], R)
    with pytest.raises(ValueError, match="W must have shape"):
        engine.slabmul(ctx, W[:1], R)
    with pytest.raises(ValueError, match="rows of W"):
        engine.slabmul(ctx, torch.zeros((2, 17, 3), dtype=torch.float32, device=dev), R)
    with pytest.raises(ValueError, match="batch of matrices"):
        engine.slabmul(ctx, W[0], R)
    with pytest.raises(ValueError, match="out must be"):
        engine.slabmul(ctx, W, R, out=torch.empty((2, 4, 11), dtype=torch.float32, device=dev))
    assert tuple(engine.slabmul(ctx, W, R[:, :, :0]).shape) == (2, 4, 0)
    assert tuple(engine.slabmul(ctx, W[:0], R[:0]).shape) == (0, 4, 10)
