"""GPU tests of the block-transform operator of spectral EOF analysis (engine.blockxform, engine.mat_blockxform;
csrc/eofx_spectral.hpp): Q[c, b, j] = sum_t B[c, t] T[j, b hop + t] against a float64 einsum.

The bound is the fma-chain bound of a float32 chain of n_fft terms, per element:

    |Q[c, b, j] - Q64[c, b, j]| <= n_fft 2^-24 sum_t |B[c, t]| |T[j, b hop + t]|

Shapes: the kernel's edges are the chunk of 32 samples (n_fft 31, 32, 33, 64), the tiles of 128 series and of 128
coefficients (127, 128, 129 / 130, 257), one block and several, hops below, at and above n_fft, and block starts of every
residue mod 4 (hop = 1 and hop = 3 with five blocks).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_LIST = [1, 127, 128, 129, 257]
NFFT_LIST = [2, 5, 31, 32, 33, 64, 100]
NCOEF_LIST = [1, 2, 127, 128, 130]
P_MAX, NCOEF_MAX, NBLK = max(P_LIST), max(NCOEF_LIST), 5
SENTINEL = -12345.678


def hops(n_fft):
    return [1, 3, n_fft, n_fft + 2]


def operands(torch, dev, n_fft, hop, nblk=NBLK, p=P_MAX, ncoef=NCOEF_MAX, seed=0, extra=1):
    g = torch.Generator(device="cpu").manual_seed(100000 * n_fft + 100 * hop + seed)
    n = (nblk - 1) * hop + n_fft + extra
    T = torch.randn((p, n), generator=g, dtype=torch.float32)
    B = torch.randn((ncoef, n_fft), generator=g, dtype=torch.float32)
    return T.to(dev), B.to(dev)


def reference(torch, T, B, hop, nblk):
    """Q64 [ncoef x nblk x p] and the bound of every element, float64 on the device"""
    n_fft = B.shape[1]
    Tb = T.double().unfold(1, n_fft, hop)[:, :nblk]                      # [p x nblk x n_fft]
    q = torch.einsum("ct,jbt->cbj", B.double(), Tb)
    mag = torch.einsum("ct,jbt->cbj", B.double().abs(), Tb.abs())
    return q, n_fft * 2.0 ** -24 * mag


def assert_within(torch, q, ref, bound, what=""):
    assert q.dtype == torch.float32 and q.shape == ref.shape, (q.dtype, q.shape, ref.shape)
    err = (q.double() - ref).abs()
    bad = torch.nonzero(~(err <= bound))
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert len(bad) == 0, f"{what}: {len(bad)} elements outside the bound, first {bad[0].tolist()}"


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. every edge
@pytest.mark.parametrize("n_fft", NFFT_LIST)
def test_random_operands_at_every_edge(ctx, n_fft):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    for hop in hops(n_fft):
        T, B = operands(torch, dev, n_fft, hop)
        ref, bound = reference(torch, T, B, hop, NBLK)                    # Q[c, :, j] depends on row c and series j alone
        for p in P_LIST:
            for nc in NCOEF_LIST:
                q = engine.blockxform(ctx, T[:p], B[:nc], hop, NBLK)
                assert tuple(q.shape) == (nc, NBLK, p) and q.is_cuda and q.is_contiguous()
                assert_within(torch, q, ref[:nc, :, :p], bound[:nc, :, :p], f"n_fft={n_fft} hop={hop} p={p} ncoef={nc}")


@pytest.mark.parametrize("n_fft,hop", [(2, 1), (33, 3), (64, 64), (100, 102)])
def test_one_block(ctx, n_fft, hop):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, B = operands(torch, dev, n_fft, hop, nblk=1, p=129, ncoef=3, extra=0)
    assert T.shape[1] == n_fft
    ref, bound = reference(torch, T, B, hop, 1)
    assert_within(torch, engine.blockxform(ctx, T, B, hop, 1), ref, bound, f"one block n_fft={n_fft}")


def test_more_blocks_than_block_groups(ctx):
    """p = 257 and ncoef = 130 give 3 x 2 tiles, so ceil(1024 / 6) = 171 groups: 400 blocks make a workgroup walk two or
    three; 1500 series tiles leave one group that walks them all"""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, B = operands(torch, dev, 8, 1, nblk=400, p=257, ncoef=130)
    ref, bound = reference(torch, T, B, 1, 400)
    assert_within(torch, engine.blockxform(ctx, T, B, 1, 400), ref, bound, "400 blocks")
    T, B = operands(torch, dev, 5, 2, nblk=3, p=1500 * 128 + 1, ncoef=2)
    ref, bound = reference(torch, T, B, 2, 3)
    assert_within(torch, engine.blockxform(ctx, T, B, 2, 3), ref, bound, "1501 series tiles")


# ------------------------------------------------------------------------------------------------ 2. strides
def test_row_strides_above_the_columns_and_a_strided_view(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    n_fft, hop, nblk, p, nc = 33, 5, 4, 130, 7
    T, B = operands(torch, dev, n_fft, hop, nblk=nblk, p=p, ncoef=nc)
    n = T.shape[1]
    ref, bound = reference(torch, T, B, hop, nblk)
    q0 = engine.blockxform(ctx, T, B, hop, nblk)
    big = torch.full((p, n + 13), float("nan"), dtype=torch.float32, device=dev)
    big[:, :n] = T
    Bb = torch.full((nc, n_fft + 3), float("nan"), dtype=torch.float32, device=dev)
    Bb[:, :n_fft] = B
    q1 = engine.blockxform(ctx, big[:, :n], Bb[:, :n_fft], hop, nblk)     # ld > n, ldb > n_fft: read where they lie
    assert torch.equal(bits(q0), bits(q1))
    wide = torch.zeros((p, 2 * n), dtype=torch.float32, device=dev)
    wide[:, ::2] = T
    q2 = engine.blockxform(ctx, wide[:, ::2], B, hop, nblk)                # a column stride of 2: made contiguous
    assert torch.equal(bits(q0), bits(q2))
    q3 = engine.blockxform(ctx, T.cpu().numpy(), B.cpu().numpy(), hop, nblk)      # host arrays
    assert torch.equal(bits(q0), bits(q3))
    assert_within(torch, q0, ref, bound, "strides")


# ------------------------------------------------------------------------------------------------ 3. exact integers
@pytest.mark.parametrize("n_fft,hop,p,nc", [(2, 1, 1, 1), (33, 3, 129, 130), (64, 66, 257, 2), (100, 50, 128, 128)])
def test_small_integers_bit_for_bit(ctx, n_fft, hop, p, nc):
    """|B| <= 8, |T| <= 8, n_fft <= 100: every partial sum is an integer below 2^24, so float32 is exact in any order"""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    g = torch.Generator(device="cpu").manual_seed(n_fft + p)
    n = (NBLK - 1) * hop + n_fft
    T = torch.randint(-8, 9, (p, n), generator=g).float().to(dev)
    B = torch.randint(-8, 9, (nc, n_fft), generator=g).float().to(dev)
    ref, _ = reference(torch, T, B, hop, NBLK)
    q = engine.blockxform(ctx, T, B, hop, NBLK)
    assert torch.equal(q.double(), ref)


# ------------------------------------------------------------------------------------------------ 4. nothing else is written
@pytest.mark.parametrize("p,nc", [(1, 1), (127, 130), (129, 127), (257, 2)])
def test_canaries_around_q(ctx, p, nc):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    n_fft, hop = 33, 7
    T, B = operands(torch, dev, n_fft, hop, p=p, ncoef=nc)
    pad = 4096
    buf = torch.full((2 * pad + nc * NBLK * p,), SENTINEL, dtype=torch.float32, device=dev)
    out = buf[pad:pad + nc * NBLK * p].view(nc, NBLK, p)
    q = engine.blockxform(ctx, T, B, hop, NBLK, out=out)
    assert q.data_ptr() == out.data_ptr()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + nc * NBLK * p:] == SENTINEL).all())
    ref, bound = reference(torch, T, B, hop, NBLK)
    assert_within(torch, q, ref, bound, f"canaries p={p} ncoef={nc}")
    Tc, Bc = T.clone(), B.clone()
    engine.blockxform(ctx, T, B, hop, NBLK)
    assert torch.equal(T, Tc) and torch.equal(B, Bc)                       # the operands are read only


# ------------------------------------------------------------------------------------------------ 5. bad values stay put
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_bad_series_touches_its_own_outputs_only(ctx, bad):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    n_fft, hop, p, nc = 33, 4, 200, 5
    T, B = operands(torch, dev, n_fft, hop, p=p, ncoef=nc)
    clean = engine.blockxform(ctx, T, B, hop, NBLK)
    Tb = T.clone()
    for j in (0, 63, 128, 199):
        Tb[j, 17] = bad
    q = engine.blockxform(ctx, Tb, B, hop, NBLK)
    keep = torch.ones(p, dtype=torch.bool, device=dev)
    keep[[0, 63, 128, 199]] = False
    assert torch.equal(bits(q[:, :, keep]), bits(clean[:, :, keep]))
    assert bool((~torch.isfinite(q[:, :, ~keep])).any())
    # the trailing sample past the last block is never read
    Tt = T.clone()
    Tt[:, (NBLK - 1) * hop + n_fft:] = bad
    assert torch.equal(bits(engine.blockxform(ctx, Tt, B, hop, NBLK)), bits(clean))


def test_reruns_are_bit_equal(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, B = operands(torch, dev, 100, 50, p=257, ncoef=130)
    a = engine.blockxform(ctx, T, B, 50, NBLK)
    b = engine.blockxform(ctx, T, B, 50, NBLK)
    assert torch.equal(bits(a), bits(b))
    # an element does not depend on what else is in the call: rows of B, series and blocks taken apart
    c = engine.blockxform(ctx, T[64:200], B[3:131], 50, NBLK - 2)
    assert torch.equal(bits(c), bits(a[3:131, :NBLK - 2, 64:200]))


# ------------------------------------------------------------------------------------------------ 6. the resident twin
@pytest.mark.parametrize("n,P,in_place", [(77, 150, True), (130, 65, False)])
def test_the_mat_twin_equals_the_panel_entry(ctx, n, P, in_place):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(n + P)
    X = rng.standard_normal((n, P)).astype(np.float32)
    n_fft, hop = 16, 7
    nblk = (n - (n_fft - hop)) // hop
    B = torch.from_numpy(rng.standard_normal((6, n_fft)).astype(np.float32)).to(dev)
    mat, _ = engine.preprocess(ctx, X, True, False, None, in_place=in_place)
    try:
        had = mat.has_sample_layout()
        Xt = mat.download()
        got = engine.mat_blockxform(ctx, mat, B, hop, nblk)
        assert tuple(got.shape) == (6, nblk, mat.p)
        assert mat.has_sample_layout()                                 # built on demand, kept for the caller to release
        if not had:
            mat.release_sample_layout()
        Tp = torch.from_numpy(np.ascontiguousarray(Xt.T)).to(dev)
        assert torch.equal(bits(got), bits(engine.blockxform(ctx, Tp, B, hop, nblk)))
        ref, bound = reference(torch, Tp, B, hop, nblk)
        assert_within(torch, got, ref, bound, f"resident n={n} P={P}")
        assert np.array_equal(mat.download(), Xt)                      # the field is read only
    finally:
        mat.free()


def test_the_mat_twin_refuses_a_masked_in_place_matrix(ctx):
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(2)
    X = rng.standard_normal((200, 700)).astype(np.float32)     # layout mode 3 keeps a mask in place when n < valid features >= 0.6 P, P % 4 == 0
    X[:, ::3] = np.nan
    mat, st = engine.preprocess(ctx, X, True, False, None, in_place=True, allow_masked=True)
    try:
        assert mat.masked, "the engine did not keep the land mask in place: the case needs another shape"
        B = torch.ones((2, 8), dtype=torch.float32, device=dev)
        with pytest.raises(ValueError, match="masked in-place matrix: compact it first"):
            engine.mat_blockxform(ctx, mat, B, 4, 3)
        q = torch.full((2, 3, mat.p_phys), SENTINEL, dtype=torch.float32, device=dev)
        assert ctx.lib.eofx_mat_blockxform_f32(ctx.handle, mat.handle, ptr(B), 2, 8, 8, 4, 3, ptr(q)) == _lib.ERR_ARG
        assert b"masked in-place matrix: compact it first" in ctx.lib.eofx_last_error(ctx.handle)
        assert ctx.lib.eofx_mat_blockxform_f32(ctx.handle, None, ptr(B), 2, 8, 8, 4, 3, ptr(q)) == _lib.ERR_ARG
        ctx.synchronize()
        assert bool((q == SENTINEL).all())
    finally:
        mat.free()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T = torch.zeros((4, 40), dtype=torch.float32, device=dev)
    B = torch.zeros((3, 8), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="hop"):
        engine.blockxform(ctx, T, B, 0, 2)
    with pytest.raises(ValueError, match="past the series"):
        engine.blockxform(ctx, T, B, 8, 6)                                  # 5 * 8 + 8 = 48 > 40
    engine.blockxform(ctx, T, B, 8, 5)                                      # 4 * 8 + 8 = 40: the last block ends at the end
    with pytest.raises(ValueError, match="past the series"):
        engine.blockxform(ctx, T[:, :7], B, 1, 1)                           # n_fft > n
    with pytest.raises(ValueError, match="nblk"):
        engine.blockxform(ctx, T, B, 1, 0)
    with pytest.raises(ValueError, match="out must be"):
        engine.blockxform(ctx, T, B, 8, 2, out=torch.empty((3, 2, 5), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        engine.blockxform(ctx, T, B, 8, 2, out=torch.empty((3, 2, 4), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="matrix"):
        engine.blockxform(ctx, T[0], B, 8, 2)
    big = torch.zeros((1, engine.BLOCKXFORM_NFFT_MAX + 1), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="n_fft"):
        engine.blockxform(ctx, big, big, 1, 1)
    with pytest.raises(ValueError, match="ncoef"):
        engine.blockxform(ctx, T, torch.zeros((engine.BLOCKXFORM_NCOEF_MAX + 1, 8), dtype=torch.float32, device=dev), 8, 2)
    # the entry itself: strides below the columns, p == 0
    from xeofs_amd import _lib
    from xeofs_amd._lib import ptr

    lib, h = ctx.lib, ctx.handle
    q = torch.full((3, 2, 4), SENTINEL, dtype=torch.float32, device=dev)
    call = lambda p=4, n=40, ld=40, nc=3, nf=8, ldb=8, hop=8, nblk=2: lib.eofx_blockxform_f32(h, ptr(T), p, n, ld, ptr(B), nc, nf, ldb, hop,
                                                                                              nblk, ptr(q))
    assert call(ld=39) == _lib.ERR_ARG and b"stride" in lib.eofx_last_error(h)
    assert call(ldb=7) == _lib.ERR_ARG and b"stride" in lib.eofx_last_error(h)
    assert call(hop=0) == _lib.ERR_ARG and b"hop" in lib.eofx_last_error(h)
    assert call(nblk=6) == _lib.ERR_ARG and b"past the series" in lib.eofx_last_error(h)
    assert call(nblk=0) == _lib.ERR_ARG and call(nc=0) == _lib.ERR_ARG and call(nf=0) == _lib.ERR_ARG and call(p=-1) == _lib.ERR_ARG
    assert call(nf=engine.BLOCKXFORM_NFFT_MAX + 1, n=2 ** 20, ld=2 ** 20, ldb=2 ** 20) == _lib.ERR_SHAPE
    assert call(nc=engine.BLOCKXFORM_NCOEF_MAX + 1) == _lib.ERR_SHAPE
    assert call(p=0) == _lib.EOFX_OK                                     # p == 0: a no-op
    assert call(p=0, hop=0) == _lib.ERR_ARG                              # ... after the argument checks
    assert lib.eofx_blockxform_f32(h, None, 4, 40, 40, ptr(B), 3, 8, 8, 8, 2, ptr(q)) == _lib.ERR_ARG
    assert lib.eofx_blockxform_f32(h, ptr(T), 4, 40, 40, None, 3, 8, 8, 8, 2, ptr(q)) == _lib.ERR_ARG
    assert lib.eofx_blockxform_f32(h, ptr(T), 4, 40, 40, ptr(B), 3, 8, 8, 8, 2, None) == _lib.ERR_ARG
    assert lib.eofx_blockxform_f32(None, ptr(T), 4, 40, 40, ptr(B), 3, 8, 8, 8, 2, ptr(q)) == _lib.ERR_ARG
    ctx.synchronize()
    assert bool((q == SENTINEL).all())
    assert tuple(engine.blockxform(ctx, T[:0], B, 8, 2).shape) == (3, 2, 0)
