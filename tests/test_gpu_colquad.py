"""GPU tests of the quadratic-form operator of empirical orthogonal teleconnections (engine.colquad, engine.mat_colquad;
csrc/eofx_colquad.hpp): q[j] = sum_s sum_t T[j, s] A[s, t] T[j, t] against a float64 einsum.

The bound is the fma-chain bound of the float32 matrix core for ANY summation order, per series:

    |q[j] - q64[j]| <= 1.01 (n + 8) 2^-24 sum_s sum_t |T[j, s]| |A[s, t]| |T[j, t]|

(a float32 fma chain of n terms; the float64 epilogue adds nothing visible to it.)

Shapes: the kernel's edges are the K chunk of 32 samples, the column block of 128 columns of A, the series tile of 128, and the
column split -- min(column blocks, 16, ceil(512 / series tiles)) workgroups share the columns of A: one column block up to
n = 128 (q written directly), one block per workgroup up to n = 2048, and from n = 2049 a workgroup walks more than one block;
the split is 16 up to 34 series tiles (p = 4352), 15 from p = 4353, and 1 from 512 series tiles (p = 65409).
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LIST = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 2048, 2049]
P_LIST = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129]
P_MAX = max(P_LIST)
SENTINEL = -12345.678


def operands(torch, dev, n, p, seed=0, symmetric=False):
    g = torch.Generator(device="cpu").manual_seed(1000 * n + p + seed)
    T = torch.randn((p, n), generator=g, dtype=torch.float32)
    A = torch.randn((n, n), generator=g, dtype=torch.float32)
    if symmetric:
        A = A + A.t()
    return T.to(dev), A.to(dev)


def reference(torch, T, A):
    """q64 and the bound of every series, float64 on the device"""
    T64, A64 = T.double(), A.double()
    q = torch.einsum("js,st,jt->j", T64, A64, T64)
    mag = torch.einsum("js,st,jt->j", T64.abs(), A64.abs(), T64.abs())
    return q, 1.01 * (T.shape[1] + 8) * 2.0 ** -24 * mag


def assert_within(torch, q, ref, bound, what=""):
    assert q.dtype == torch.float64 and q.shape == ref.shape
    err = (q - ref).abs()
    bad = torch.nonzero(~(err <= bound)).flatten()
    worst = float((err / bound.clamp_min(1e-300)).max()) if len(err) else 0.0
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert len(bad) == 0, f"{what}: {len(bad)} series outside the bound, first {int(bad[0])}: {float(err[bad[0]])} > {float(bound[bad[0]])}"


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------ 1. every edge, random A
@pytest.mark.parametrize("n", N_LIST)
def test_random_nonsymmetric_at_every_edge(ctx, n):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, A = operands(torch, dev, n, P_MAX)
    ref, bound = reference(torch, T, A)                                # row j depends on series j alone: shared by every p
    for p in P_LIST:
        q = engine.colquad(ctx, T[:p], A)
        assert tuple(q.shape) == (p,) and q.is_cuda
        assert_within(torch, q, ref[:p], bound[:p], f"n={n} p={p}")


@pytest.mark.parametrize("n,p", [(129, 65408), (129, 65409), (2049, 4352), (2049, 4353)])
def test_either_side_of_a_change_of_the_column_split(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, A = operands(torch, dev, n, p)
    ref, bound = reference(torch, T, A)
    assert_within(torch, engine.colquad(ctx, T, A), ref, bound, f"n={n} p={p}")


# ------------------------------------------------------------------------------------------------ 2. designed matrices
@pytest.mark.parametrize("n,p", [(1, 1), (33, 65), (129, 129), (257, 33)])
def test_zero_and_identity(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, _ = operands(torch, dev, n, p)
    q = engine.colquad(ctx, T, torch.zeros((n, n), dtype=torch.float32, device=dev))
    assert bool((q == 0.0).all())                                      # exactly
    eye = torch.eye(n, dtype=torch.float32, device=dev)
    ref, bound = reference(torch, T, eye)
    assert torch.allclose(ref, (T.double() ** 2).sum(dim=1), rtol=1e-14)
    assert_within(torch, engine.colquad(ctx, T, eye), ref, bound, f"identity n={n} p={p}")


def test_a_single_entry_moved_over_the_tile_corners(ctx):
    """A = a e_s e_t^T gives T[j, s] a T[j, t]: any slip of an index shows"""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    n, p = 257, 33
    T, _ = operands(torch, dev, n, p, seed=5)
    T64 = T.double()
    corners = [0, 1, 31, 32, 33, 63, 64, 127, 128, 129, 255, 256]
    A = torch.zeros((n, n), dtype=torch.float32, device=dev)
    out = torch.empty(p, dtype=torch.float64, device=dev)
    a = 1.7
    worst = 0.0
    for s in corners:
        for t in corners:
            A[s, t] = a
            q = engine.colquad(ctx, T, A, out=out)
            A[s, t] = 0.0
            want = T64[:, s] * float(np.float32(a)) * T64[:, t]
            bound = 1.01 * (n + 8) * 2.0 ** -24 * want.abs()
            err = (q - want).abs()
            assert bool((err <= bound).all()), (s, t, float(err.max()))
            worst = max(worst, float((err / bound).max()))
    print(f"single entry: largest error / bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 3. what is read and written
@pytest.mark.parametrize("n,p", [(33, 65), (130, 129), (257, 31)])
def test_strides_padding_canaries_and_read_only_operands(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, A = operands(torch, dev, n, p, seed=2)
    plain = engine.colquad(ctx, T, A)
    Tbig = torch.full((p, n + 5), float("nan"), dtype=torch.float32, device=dev)
    Abig = torch.full((n, n + 3), float("nan"), dtype=torch.float32, device=dev)
    Tbig[:, :n] = T
    Abig[:, :n] = A
    Tv, Av = Tbig[:, :n], Abig[:, :n]
    assert Tv.stride(0) == n + 5 and Av.stride(0) == n + 3
    T0, A0 = Tbig.clone(), Abig.clone()
    qbuf = torch.full((p + 16,), SENTINEL, dtype=torch.float64, device=dev)
    q = engine.colquad(ctx, Tv, Av, out=qbuf[8:8 + p])
    assert q.data_ptr() == qbuf[8:].data_ptr()
    assert bool(torch.isfinite(q).all())                               # the NaNs of the padding were not read into a result
    assert torch.equal(bits(q), bits(plain))                           # the strides change nothing
    assert bool((qbuf[:8] == SENTINEL).all()) and bool((qbuf[8 + p:] == SENTINEL).all())
    assert torch.equal(Tbig.view(torch.int32), T0.view(torch.int32)) and torch.equal(Abig.view(torch.int32), A0.view(torch.int32))
    again = engine.colquad(ctx, Tv, Av)
    assert torch.equal(bits(again), bits(plain))                       # two runs are equal bit for bit


@pytest.mark.parametrize("n,p", [(33, 65), (257, 129), (2049, 130)])
def test_a_bad_series_stays_in_its_row(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, A = operands(torch, dev, n, p, seed=3)
    clean = engine.colquad(ctx, T, A)
    Tb = T.clone()
    jn, ji = p // 3, p - 1
    Tb[jn, :] = float("nan")
    Tb[ji, n // 2] = float("inf")
    q = engine.colquad(ctx, Tb, A)
    keep = torch.ones(p, dtype=torch.bool, device=dev)
    keep[jn] = keep[ji] = False
    assert torch.equal(bits(q[keep]), bits(clean[keep]))               # every other series bit for bit
    assert bool(torch.isnan(q[jn])) and not bool(torch.isfinite(q[ji]))
    assert torch.equal(bits(engine.colquad(ctx, T, A)), bits(clean))


# ------------------------------------------------------------------------------------------------ 4. limits and refusals
def test_refusals_before_any_launch(ctx):
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    dev = f"cuda:{ctx.device}"
    lib, h = ctx.lib, ctx.handle
    T = torch.zeros((3, 40), dtype=torch.float32, device=dev)
    A = torch.zeros((40, 40), dtype=torch.float32, device=dev)
    q = torch.full((3,), SENTINEL, dtype=torch.float64, device=dev)
    call = lambda n, ld, lda, p=3: lib.eofx_colquad_f32(h, ptr(T), p, n, ld, ptr(A), lda, ptr(q))
    assert call(40, 39, 40) == _lib.ERR_ARG                            # ld < n
    assert call(40, 40, 39) == _lib.ERR_ARG                            # lda < n
    assert call(0, 40, 40) == _lib.ERR_ARG                             # n < 1
    assert call(40, 40, 40, p=-1) == _lib.ERR_ARG
    assert call(16385, 16385, 16385) == _lib.ERR_SHAPE                 # checked by argument: nothing is launched
    assert b"16384" in lib.eofx_last_error(h)
    assert call(16385, 16385, 16385, p=0) == _lib.ERR_SHAPE            # ... also when there is nothing to do
    assert call(40, 40, 40, p=0) == _lib.EOFX_OK                       # p == 0: a no-op
    assert call(40, 39, 40, p=0) == _lib.ERR_ARG                       # ... after the argument checks
    assert lib.eofx_colquad_f32(h, ptr(T), 3, 40, 40, ptr(A), 40, None) == _lib.ERR_ARG
    ctx.synchronize()
    assert bool((q == SENTINEL).all())
    empty = engine.colquad(ctx, torch.zeros((0, 12), dtype=torch.float32, device=dev), torch.zeros((12, 12), device=dev))
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.float64
    with pytest.raises(ValueError, match="square matrix of the 40 samples"):
        engine.colquad(ctx, T, A[:, :39])
    with pytest.raises(ValueError, match="out must be"):
        engine.colquad(ctx, T, A, out=torch.empty(3, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        engine.colquad(ctx, T, A, out=torch.empty(4, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="matrix"):
        engine.colquad(ctx, T[0], A)
    # host arrays are staged
    rng = np.random.default_rng(0)
    Th, Ah = rng.standard_normal((5, 9)).astype(np.float32), rng.standard_normal((9, 9)).astype(np.float32)
    got = engine.colquad(ctx, Th, Ah)
    ref, bound = reference(torch, torch.from_numpy(Th).to(dev), torch.from_numpy(Ah).to(dev))
    assert_within(torch, got, ref, bound, "host operands")


# ------------------------------------------------------------------------------------------------ 5. the resident matrix
@pytest.mark.parametrize("n,P,in_place", [(33, 70, True), (130, 65, False), (257, 300, True)])
def test_resident_matrix_entry_equals_the_panel_entry(ctx, n, P, in_place):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(n + P)
    X = rng.standard_normal((n, P)).astype(np.float32)
    mat, _ = engine.preprocess(ctx, X, True, False, None, in_place=in_place)
    try:
        had = mat.has_sample_layout()
        _, A = operands(torch, dev, n, 1, seed=7)
        Apad = torch.full((n, n + 2), float("nan"), dtype=torch.float32, device=dev)
        Apad[:, :n] = A
        q = engine.mat_colquad(ctx, mat, Apad[:, :n])
        assert tuple(q.shape) == (mat.p,) and q.dtype == torch.float64
        assert mat.has_sample_layout()                                 # built on demand, kept for the caller to release
        if not had:
            mat.release_sample_layout()
            assert not mat.has_sample_layout()
        Xt = mat.download()
        Tp = torch.from_numpy(np.ascontiguousarray(Xt.T)).to(dev)
        assert torch.equal(bits(q), bits(engine.colquad(ctx, Tp, A)))
        ref, bound = reference(torch, Tp, A)
        assert_within(torch, q, ref, bound, f"resident n={n} P={P}")
        qbuf = torch.full((mat.p + 4,), SENTINEL, dtype=torch.float64, device=dev)
        engine.mat_colquad(ctx, mat, A, out=qbuf[2:2 + mat.p])
        assert torch.equal(bits(qbuf[2:2 + mat.p]), bits(q)) and bool((qbuf[:2] == SENTINEL).all()) and bool((qbuf[-2:] == SENTINEL).all())
        assert np.array_equal(mat.download(), Xt)                      # the field is read only
        with pytest.raises(ValueError, match="square matrix"):
            engine.mat_colquad(ctx, mat, A[:-1, :-1])
    finally:
        mat.free()


def test_resident_matrix_entry_refuses_a_masked_in_place_matrix(ctx):
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
        A = torch.zeros((200, 200), dtype=torch.float32, device=dev)
        with pytest.raises(ValueError, match="masked"):
            engine.mat_colquad(ctx, mat, A)
        q = torch.full((mat.p_phys,), SENTINEL, dtype=torch.float64, device=dev)
        assert ctx.lib.eofx_mat_colquad_f32(ctx.handle, mat.handle, ptr(A), 200, ptr(q)) == _lib.ERR_ARG
        assert b"masked" in ctx.lib.eofx_last_error(ctx.handle)
        assert ctx.lib.eofx_mat_colquad_f32(ctx.handle, None, ptr(A), 200, ptr(q)) == _lib.ERR_ARG
        ctx.synchronize()
        assert bool((q == SENTINEL).all())
    finally:
        mat.free()
