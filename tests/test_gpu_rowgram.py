"""GPU tests of the row-Gram operator of spectral EOF analysis (engine.rowgram; csrc/eofx_spectral.hpp):
G[f] = R[f] R[f]^T in float64 of a batch of float32 slabs R [nb x r x p], against float64.

The bound: float32 fma chains over spans of ROWGRAM_SPAN = 2048 features, float64 beyond (whose rounding adds nothing
visible), per element

    |G[f, a, b] - G64[f, a, b]| <= ROWGRAM_SPAN 2^-24 sum_j |R[f, a, j]| |R[f, b, j]|

Shapes: the tile of 128 rows (r 63 .. 65, 130), one span and its edges (p 2047, 2048, 2049), and the split of the spans over
workgroups, min(spans, 16 / tile pairs): 16 for r <= 128 (edges at p = 16 spans and one feature more), 5 for r = 130.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_LIST = [1, 2, 63, 64, 65, 130]
SPAN = 2048
P_LIST = [1, 33, SPAN - 1, SPAN, SPAN + 1, 5 * SPAN + 1, 16 * SPAN, 16 * SPAN + 1, 33 * SPAN + 7]
SENTINEL = -12345.678


def slabs(torch, dev, nb, r, p, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * r + p + seed)
    return torch.randn((nb, r, p), generator=g, dtype=torch.float32).to(dev)


def reference(torch, R):
    R64 = R.double()
    return R64 @ R64.transpose(1, 2), SPAN * 2.0 ** -24 * (R64.abs() @ R64.abs().transpose(1, 2))


def assert_within(torch, G, ref, bound, what=""):
    assert G.dtype == torch.float64 and G.shape == ref.shape
    err = (G - ref).abs()
    bad = torch.nonzero(~(err <= bound))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert len(bad) == 0, f"{what}: {len(bad)} elements outside the bound, first {bad[0].tolist()}"


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def test_the_span_is_the_documented_one():
    from xeofs_amd import engine

    assert engine.ROWGRAM_SPAN == SPAN and engine.ROWGRAM_RMAX >= 512


@pytest.mark.parametrize("p", P_LIST)
def test_random_slabs_at_every_edge(ctx, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    for nb in (1, 3):
        R = slabs(torch, dev, nb, max(R_LIST), p, seed=nb)
        for r in R_LIST:
            Rr = R[:, :r].contiguous()
            ref, bound = reference(torch, Rr)
            G = engine.rowgram(ctx, Rr)
            assert tuple(G.shape) == (nb, r, r) and G.is_cuda
            assert_within(torch, G, ref, bound, f"p={p} nb={nb} r={r}")
            assert torch.equal(bits(G), bits(G.transpose(1, 2)))            # symmetric bit for bit
            assert torch.equal(bits(G), bits(engine.rowgram(ctx, Rr)))      # two runs are equal bit for bit


def test_the_largest_slab(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    R = slabs(torch, dev, 2, engine.ROWGRAM_RMAX, 2 * SPAN + 5)
    ref, bound = reference(torch, R)
    G = engine.rowgram(ctx, R)
    assert_within(torch, G, ref, bound, "r = ROWGRAM_RMAX")
    assert torch.equal(bits(G), bits(G.transpose(1, 2)))


@pytest.mark.parametrize("r,p", [(1, 1), (65, SPAN + 1), (130, 5 * SPAN + 1), (64, 17 * SPAN)])
def test_integer_slabs_are_exact(ctx, r, p):
    """entries in {-2 .. 2}: a chain of 2048 products stays below 2^24, float64 carries the rest exactly"""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    g = torch.Generator(device="cpu").manual_seed(r + p)
    R = torch.randint(-2, 3, (3, r, p), generator=g).float().to(dev)
    ref, _ = reference(torch, R)
    assert torch.equal(engine.rowgram(ctx, R), ref)


def test_a_slab_does_not_depend_on_its_batch(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    R = slabs(torch, dev, 5, 22, 7 * SPAN + 3)
    G = engine.rowgram(ctx, R)
    for f in range(5):
        assert torch.equal(bits(G[f]), bits(engine.rowgram(ctx, R[f:f + 1])[0]))
    assert torch.equal(bits(G[1:4]), bits(engine.rowgram(ctx, R[1:4])))


@pytest.mark.parametrize("r,p,nb", [(1, 1, 1), (65, SPAN + 1, 3), (130, 33, 2)])
def test_canaries_and_read_only_operands(ctx, r, p, nb):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    R = slabs(torch, dev, nb, r, p)
    Rc = R.clone()
    pad, m = 1024, nb * r * r
    buf = torch.full((2 * pad + m,), SENTINEL, dtype=torch.float64, device=dev)
    out = buf[pad:pad + m].view(nb, r, r)
    G = engine.rowgram(ctx, R, out=out)
    assert G.data_ptr() == out.data_ptr()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + m:] == SENTINEL).all())
    ref, bound = reference(torch, R)
    assert_within(torch, G, ref, bound, f"canaries r={r} p={p}")
    assert torch.equal(R, Rc)
    G2 = engine.rowgram(ctx, R.cpu().numpy())                               # a host array is staged
    assert torch.equal(bits(G2), bits(G))


def test_refusals(ctx):
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    dev = f"cuda:{ctx.device}"
    lib, h = ctx.lib, ctx.handle
    R = torch.zeros((2, 3, 10), dtype=torch.float32, device=dev)
    G = torch.full((2, 3, 3), SENTINEL, dtype=torch.float64, device=dev)
    call = lambda nb=2, r=3, p=10: lib.eofx_rowgram_f32(h, ptr(R), nb, r, p, ptr(G))
    assert call(r=engine.ROWGRAM_RMAX + 1) == _lib.ERR_SHAPE and b"rows" in lib.eofx_last_error(h)
    assert call(nb=engine.SPECTRAL_NBMAX + 1) == _lib.ERR_SHAPE and b"slabs" in lib.eofx_last_error(h)
    assert call(r=0) == _lib.ERR_ARG and call(p=0) == _lib.ERR_ARG and call(nb=-1) == _lib.ERR_ARG
    assert call(nb=0) == _lib.EOFX_OK
    assert lib.eofx_rowgram_f32(h, None, 2, 3, 10, ptr(G)) == _lib.ERR_ARG
    assert lib.eofx_rowgram_f32(h, ptr(R), 2, 3, 10, None) == _lib.ERR_ARG
    assert lib.eofx_rowgram_f32(None, ptr(R), 2, 3, 10, ptr(G)) == _lib.ERR_ARG
    ctx.synchronize()
    assert bool((G == SENTINEL).all())
    with pytest.raises(ValueError, match="rows"):
        engine.rowgram(ctx, torch.zeros((1, engine.ROWGRAM_RMAX + 1, 4), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="batch of matrices"):
        engine.rowgram(ctx, R[0])
    with pytest.raises(ValueError, match="at least one row"):
        engine.rowgram(ctx, R[:, :, :0])
    with pytest.raises(ValueError, match="out must be"):
        engine.rowgram(ctx, R, out=torch.empty((2, 3, 3), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        engine.rowgram(ctx, R, out=torch.empty((2, 3, 4), dtype=torch.float64, device=dev))
    assert tuple(engine.rowgram(ctx, R[:0]).shape) == (0, 3, 3)
