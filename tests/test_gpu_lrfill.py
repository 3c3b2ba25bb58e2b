"""The gap operators of DINEOF at their edges (csrc/eofx_lrfill.hpp): engine.gap_mask against numpy's packbits, and
engine.lrfill against a float64 `A @ B.T`.

Bound of a filled entry: the kernel's value is an fmaf chain over the k modes from zero -- k products, each rounded once
into the running float32 sum -- so |new - ref| <= gamma_k sum_m |A_im| |B_jm| with gamma_k = k u / (1 - k u), u = 2^-24;
one more u covers a last rounding (the bound the tests use: (gamma_k + u) sum |A| |B|).  The sums inherit it: with
e the bound of an entry, |(new - old)^2 - (ref - old)^2| <= e (2 |ref - old| + e) and |new^2 - ref^2| <= e (2 |ref| + e),
summed over the written entries, plus the float64 summation itself (1e-12 relative, generous)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 127, 128, 129, 257)
MODES = (1, 2, 3, 50, 255, 256)
U32 = 2.0 ** -24
SENTINEL = np.int32(0x7FC12345)          # a NaN with a payload: nothing computes it by accident


def _shapes():
    """n and p independently from SIZES, k from MODES: the full product, 384 cases of a few milliseconds each"""
    return [(n, p, k) for n in SIZES for p in SIZES for k in MODES]


def _words(p):
    return (p + 31) // 32


def _pack(mask, ldb, stray=False):
    """bool [n x p] -> int32 words [n x ldb]; the words past ceil(p / 32) are all ones (never to be read); stray: the bits of
    the columns >= p in the last word are set as well"""
    n, p = mask.shape
    w = _words(p)
    wide = np.zeros((n, w * 32), bool)
    wide[:, :p] = mask
    if stray:
        wide[:, p:] = True
    bits = np.full((n, ldb), -1, np.int32)
    bits[:, :w] = np.packbits(wide, axis=1, bitorder="little").view(np.uint32).reshape(n, w).view(np.int32)
    return bits


def _masks(n, p, rng):
    empty = np.zeros((n, p), bool)
    out = {"empty": empty, "full": np.ones((n, p), bool)}
    c = empty.copy()
    c[[0, 0, n - 1, n - 1], [0, p - 1, 0, p - 1]] = True
    out["matrix_corners"] = c
    t = empty.copy()                      # the corners of the tile (1, 1) of 128 x 128 where there is one, else of tile (0, 0)
    r0, c0 = (128 if n > 128 else 0), (128 if p > 128 else 0)
    r1, c1 = min(r0 + 127, n - 1), min(c0 + 127, p - 1)
    t[[r0, r0, r1, r1], [c0, c1, c0, c1]] = True
    t[min(127, n - 1), min(127, p - 1)] = True
    out["tile_corners"] = t
    row = empty.copy()
    row[n // 2] = True
    out["row"] = row
    col = empty.copy()
    col[:, p // 2] = True
    out["column"] = col
    out["random"] = rng.random((n, p)) < 0.3
    return out


def _problem(n, p, k, seed):
    import torch

    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k)).astype(np.float32)
    B = rng.standard_normal((p, k)).astype(np.float32)
    old = rng.standard_normal((n, p)).astype(np.float32)
    ld, lda, ldbm = p + 7, k + 3, k + 5
    Ad = torch.full((n, lda), float("nan"), device="cuda")
    Ad[:, :k] = torch.from_numpy(A)
    Bd = torch.full((p, ldbm), float("nan"), device="cuda")
    Bd[:, :k] = torch.from_numpy(B)
    F0 = np.full((n, ld), SENTINEL, np.int32)
    F0[:, :p] = old.view(np.int32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = A64 @ B64.T
    gamma = k * U32 / (1 - k * U32)
    bound = (gamma + U32) * (np.abs(A64) @ np.abs(B64).T)
    return rng, Ad[:, :k], Bd[:, :k], F0, old.astype(np.float64), ref, bound


def _fill(ctx, F0, bits, A, B, p):
    import torch

    from xeofs_amd import engine

    Fd = torch.from_numpy(F0.copy()).cuda()
    bd = torch.from_numpy(bits).cuda()
    sums = engine.lrfill(ctx, Fd.view(torch.float32)[:, :p], bd, A, B)
    return Fd.cpu().numpy(), sums


@pytest.mark.parametrize("n,p,k", _shapes())
def test_lrfill_against_float64(ctx, n, p, k):
    rng, A, B, F0, old, ref, bound = _problem(n, p, k, 1000 * n + 10 * p + k)
    assert A.stride(0) > k and B.stride(0) > k
    ldb = _words(p) + 2
    kinds = _masks(n, p, rng)
    kinds["stray"] = kinds["random"]
    for kind, mask in kinds.items():
        bits = _pack(mask, ldb, stray=kind == "stray")
        got, (count, sd, sn) = _fill(ctx, F0, bits, A, B, p)
        # untouched: every entry whose bit is clear, and all padding, bit for bit
        keep = np.ones(F0.shape, bool)
        keep[:, :p] = ~mask
        assert np.array_equal(got[keep], F0[keep]), kind
        new = got[:, :p].view(np.float32).astype(np.float64)
        err = np.abs(new - ref)[mask]
        assert np.all(err <= bound[mask]), (kind, float((err / bound[mask]).max()))
        assert count == int(mask.sum()), kind
        e = bound[mask]
        ref_sd, tol_sd = ((ref - old)[mask] ** 2).sum(), (e * (2 * np.abs(ref - old)[mask] + e)).sum()
        ref_sn, tol_sn = (ref[mask] ** 2).sum(), (e * (2 * np.abs(ref)[mask] + e)).sum()
        assert abs(sd - ref_sd) <= tol_sd + 1e-12 * ref_sd, (kind, sd, ref_sd, tol_sd)
        assert abs(sn - ref_sn) <= tol_sn + 1e-12 * ref_sn, (kind, sn, ref_sn, tol_sn)
        if kind == "empty":
            assert (count, sd, sn) == (0, 0.0, 0.0)
        if kind in ("random", "full"):          # determinism: a second call on a fresh copy
            again, sums2 = _fill(ctx, F0, bits, A, B, p)
            assert np.array_equal(again, got) and sums2 == (count, sd, sn), kind


def test_lrfill_limits_and_empty_fields(ctx):
    import torch

    from xeofs_amd import _lib, engine

    n, p = 5, 40
    F = torch.zeros((n, p), device="cuda")
    bits = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    A, B = torch.zeros((n, 257), device="cuda"), torch.zeros((p, 257), device="cuda")
    assert engine.LRFILL_KMAX == 256
    with pytest.raises(ValueError, match="k <= 256"):
        engine.lrfill(ctx, F, bits, A, B)
    sums = np.full(3, -1.0)
    rc = ctx.lib.eofx_lrfill_f32(ctx.handle, _lib.ptr(F), n, p, p, _lib.ptr(bits), 2, _lib.ptr(A), 257, _lib.ptr(B), 257, 257,
                                 _lib.ptr(sums))
    assert rc == _lib.ERR_ARG
    with pytest.raises(ValueError):
        _lib.raise_for(rc, ctx.handle)
    for bad in (dict(bits=bits[:, :1]), dict(bits=bits.to(torch.int64)), dict(A=A[:3, :4], B=B[:, :4]), dict(A=A[:, :4], B=B[:, :5]),
                dict(F=F.cpu(), A=A[:, :4], B=B[:, :4]), dict(F=F.double(), A=A[:, :4], B=B[:, :4]), dict(A=A[:, :0], B=B[:, :0])):
        args = dict(F=F, bits=bits, A=A[:, :4], B=B[:, :4])
        args.update(bad)
        with pytest.raises(ValueError):
            engine.lrfill(ctx, **args)
    # the row stride of F: four rows share one buffer resource of the kernel
    wide = torch.empty((2, engine.LRFILL_LDMAX + 1), device="cuda")[:, :p]
    assert wide.stride(0) == engine.LRFILL_LDMAX + 1 == 2 ** 26 + 1
    with pytest.raises(ValueError, match="row stride"):
        engine.lrfill(ctx, wide, bits[:2], A[:2, :4], B[:, :4])
    rc = ctx.lib.eofx_lrfill_f32(ctx.handle, _lib.ptr(wide), 2, p, wide.stride(0), _lib.ptr(bits), 2, _lib.ptr(A), 257, _lib.ptr(B), 257, 4,
                                 _lib.ptr(sums))
    assert rc == _lib.ERR_SHAPE
    del wide
    # an empty field is a successful no-op with zero sums
    for shape in ((0, 40), (5, 0)):
        Fe = torch.zeros(shape, device="cuda")
        be = torch.zeros((shape[0], engine.gap_words(shape[1])), dtype=torch.int32, device="cuda")
        assert engine.lrfill(ctx, Fe, be, torch.zeros((shape[0], 3), device="cuda"), torch.zeros((shape[1], 3), device="cuda")) \
            == (0, 0.0, 0.0)
        got, count = engine.gap_mask(ctx, Fe)
        assert count == 0 and tuple(got.shape) == (shape[0], engine.gap_words(shape[1]))


def test_lrfill_entry_index_beyond_2_31(ctx):
    """an entry whose flat index i ld + j exceeds 2^31 (and 2^32 bytes): the last row of a 32769 x 65600 field; every tile but
    the last row of tiles has no bit and is left at once"""
    import torch

    from xeofs_amd import engine

    n, p, k = 32769, 65600, 3
    assert (n - 1) * p > 2 ** 31
    rng = np.random.default_rng(5)
    A = rng.standard_normal((n, k)).astype(np.float32)
    B = rng.standard_normal((p, k)).astype(np.float32)
    F = torch.empty((n, p), device="cuda")
    cols = np.array([0, 31, 32, 4097, p - 1])
    F[0, :] = 7.0
    F[n - 1, :] = 7.0
    F[n - 2, :] = 7.0
    bits = torch.zeros((n, engine.gap_words(p)), dtype=torch.int32, device="cuda")
    mask = np.zeros((1, p), bool)
    mask[0, cols] = True
    bits[n - 1] = torch.from_numpy(_pack(mask, engine.gap_words(p))[0]).cuda()
    count, sd, sn = engine.lrfill(ctx, F, bits, A, B)
    ref = A[n - 1].astype(np.float64) @ B[cols].astype(np.float64).T
    bound = (k * U32 / (1 - k * U32) + U32) * (np.abs(A[n - 1]).astype(np.float64) @ np.abs(B[cols]).astype(np.float64).T)
    last = F[n - 1].cpu().numpy().astype(np.float64)
    assert count == cols.size and np.all(np.abs(last[cols] - ref) <= bound)
    rest = np.ones(p, bool)
    rest[cols] = False
    assert np.all(last[rest] == 7.0) and bool((F[0] == 7.0).all()) and bool((F[n - 2] == 7.0).all())
    assert abs(sn - (ref ** 2).sum()) <= (bound * (2 * np.abs(ref) + bound)).sum() + 1e-12 * (ref ** 2).sum()


def _nan_field(n, p, kind, rng):
    X = rng.standard_normal((n, p)).astype(np.float32)
    if kind == "corners":
        X[[0, 0, n - 1, n - 1], [0, p - 1, 0, p - 1]] = np.nan
    elif kind == "row":
        X[n // 2] = np.nan
    elif kind == "column":
        X[:, p // 2] = np.nan
    elif kind == "random":
        X[rng.random((n, p)) < 0.3] = np.nan
        # NaNs with a payload, negative and signalling NaNs -- and the infinities, which are no gaps
        special = np.array([0x7FC00001, 0xFFC00000, 0x7F800001, 0xFF800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000], np.uint32)
        flat = X.reshape(-1).view(np.uint32)
        where = rng.choice(n * p, size=min(n * p, special.size), replace=False)
        flat[where] = special[: where.size]
    return X


@pytest.mark.parametrize("n,p", sorted({(n, p) for n, p, _ in _shapes()}))
def test_gap_mask_against_packbits(ctx, n, p):
    import torch

    from xeofs_amd import engine

    rng = np.random.default_rng(100 * n + p)
    w = _words(p)
    for kind in ("none", "corners", "row", "column", "random"):
        X = _nan_field(n, p, kind, rng)
        nan = np.isnan(X)
        wide = np.zeros((n, w * 32), bool)
        wide[:, :p] = nan
        ref = np.packbits(wide, axis=1, bitorder="little").view(np.uint32).reshape(n, w).view(np.int32)
        # ld > p with NaNs in the padding, ldb above the word count with a sentinel in the padding words
        Xd = torch.full((n, p + 5), float("nan"), device="cuda")
        Xd[:, :p] = torch.from_numpy(X)
        out = torch.full((n, w + 2), int(SENTINEL), dtype=torch.int32, device="cuda")
        bits, count = engine.gap_mask(ctx, Xd[:, :p], out=out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :w], ref), kind                 # (the tail bits of the last word are zeros)
        assert np.all(got[:, w:] == SENTINEL), kind
        assert count == int(nan.sum()), kind
        # contiguous, the mask allocated by the call
        bits2, count2 = engine.gap_mask(ctx, torch.from_numpy(X).cuda())
        assert tuple(bits2.shape) == (n, w) and bits2.dtype == torch.int32 and np.array_equal(bits2.cpu().numpy(), ref)
        assert count2 == count


def test_gap_mask_entry_index_beyond_2_31(ctx):
    import torch

    from xeofs_amd import engine

    n, p = 32769, 65600
    X = torch.zeros((n, p), device="cuda")
    X[n - 1, p - 1] = float("nan")
    X[n - 1, 0] = float("nan")
    X[0, 33] = float("nan")
    bits, count = engine.gap_mask(ctx, X)
    assert count == 3
    w = engine.gap_words(p)
    assert (p - 1) & 31 == 31 and int(bits[n - 1, w - 1]) == -2 ** 31            # (bit 31 is the sign of the int32 word)
    assert int(bits[n - 1, 0]) == 1 and int(bits[0, 1]) == 2
    assert int(torch.count_nonzero(bits)) == 3


def test_gap_mask_rejects_what_it_cannot_read(ctx):
    import torch

    from xeofs_amd import engine

    X = torch.zeros((4, 40), device="cuda")
    for bad in (X.cpu(), X.double(), X[:, ::2], X[0]):
        with pytest.raises(ValueError):
            engine.gap_mask(ctx, bad)
    with pytest.raises(ValueError):
        engine.gap_mask(ctx, X, out=torch.zeros((4, 1), dtype=torch.int32, device="cuda"))
