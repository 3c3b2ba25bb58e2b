"""GPU tests of the pairwise-minimum operator of the teleconnectivity map (engine.pairmin, engine.mat_pairmin;
csrc/eofx_pairmin.hpp): rmin[j] = min_i (d[j, i] w[j]) w[i], d = T T^T, over i != j with w[i] > 0 and a value that is not NaN,
and partner[j] the lowest i that attains it -- against float64 on the same float32 T and w.

The bound per pair is the fma-chain bound of the float32 matrix core (tests/test_gpu_colquad.py) plus the two float32 scalings:

    bound[j, i] = 1.01 (n + 10) 2^-24 |w_j| |w_i| sum_t |T[j, t]| |T[i, t]|,      B_j = max over the admissible i of bound[j, i]

and for every j with w[j] > 0 and an admissible i:
    (a) |rmin[j] - rmin64[j]| <= B_j
    (b) r64[j, partner[j]] <= rmin64[j] + 2 B_j
    (c) where the float64 runner-up lies more than 2 B_j above the minimum, partner[j] is the float64 argmin exactly;
every other j gives (NaN, -1).  Where everything is exact (small-integer series, w a power of two) the result must equal the
float64 one bit for bit, and numpy's first argmin: the lowest index.

Shapes: the kernel's edges are the K chunk of 32 samples, the tile of 128 series (of j and of i), the 64 x 64 block of a wave
and its 32 x 32 accumulators, and the split -- min(tiles, 16, ceil(512 / tiles)) workgroups share the tiles of i, restated in
`plan` below: one tile per workgroup up to 16 tiles (p = 2048), from p = 2049 a workgroup walks more than one tile, the split
falls from 16 at 35 tiles (p = 4353) to 1 at 512 tiles (p = 65409).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LIST = [1, 2, 31, 32, 33, 65, 130]
P_LIST = [1, 2, 63, 64, 65, 127, 128, 129, 257, 300]
P_MAX = max(P_LIST)
SENT_V, SENT_I = -12345.678, -77


def plan(p):
    """(tiles, splits) of csrc/eofx_pairmin.hpp, restated"""
    tiles = (p + 127) // 128
    return tiles, min(tiles, 16, (512 + tiles - 1) // tiles)


SPLIT_CHANGES = [t for t in range(2, 600) if plan(128 * t)[1] != plan(128 * (t - 1))[1]]


def operands(torch, dev, n, p, seed=0):
    """a random panel and w = 1 / |T_j| (r is a correlation), a few entries of w zero and one negative where p allows"""
    g = torch.Generator(device="cpu").manual_seed(1000 * n + p + seed)
    T = torch.randn((p, n), generator=g, dtype=torch.float32)
    w = (1.0 / T.double().norm(dim=1).clamp_min(1e-30)).float()
    if p >= 5:
        w[p // 2] = 0.0
        w[p - 2] = -w[p - 2]
    return T.to(dev), w.to(dev)


def reference(torch, T, w, rows=2048):
    """float64 on the device, in row chunks: rmin64, argmin64, the runner-up, B_j, and whether j has a result at all"""
    T64, w64 = T.double(), w.double()
    Ta = T64.abs()
    p, n = T.shape
    col_ok = w64 > 0
    idx = torch.arange(p, device=T.device)
    out = [[] for _ in range(5)]
    for lo in range(0, p, rows):
        hi = min(p, lo + rows)
        r = (T64[lo:hi] @ T64.t()) * w64[lo:hi, None] * w64[None, :]
        ok = col_ok[None, :] & ~torch.isnan(r) & (idx[None, :] != idx[lo:hi, None])
        bound = 1.01 * (n + 10) * 2.0 ** -24 * (Ta[lo:hi] @ Ta.t()) * w64[lo:hi, None].abs() * w64[None, :].abs()
        B = torch.where(ok, bound, torch.zeros_like(bound)).max(dim=1).values
        key = torch.where(ok, r, torch.full_like(r, float("inf")))
        two = torch.topk(key, min(2, p), dim=1, largest=False)
        rmin = two.values[:, 0]
        arg = torch.argmin(key, dim=1)
        # the lowest index among equal minima (argmin names any)
        arg = torch.where(key == rmin[:, None], idx[None, :], torch.full_like(idx, p)[None, :]).min(dim=1).values
        second = two.values[:, 1] if p > 1 else torch.full_like(rmin, float("inf"))
        has = ok.any(dim=1) & (w64[lo:hi] > 0)
        for o, v in zip(out, (rmin, arg, second, B, has)):
            o.append(v)
        del r, ok, bound, key
    return tuple(torch.cat(o) for o in out)


def r64_at(torch, T, w, j, i):
    """r64[j, i] for index vectors j, i"""
    return (T.double()[j] * T.double()[i]).sum(dim=1) * w.double()[j] * w.double()[i]


def assert_within(torch, got, T, w, ref, what=""):
    rmin, partner = got
    p = T.shape[0]
    rmin64, arg64, second, B, has = (x[:p] for x in ref)
    assert rmin.dtype == torch.float32 and partner.dtype == torch.int32 and tuple(rmin.shape) == tuple(partner.shape) == (p,)
    none = ~has
    assert bool(torch.isnan(rmin[none]).all()) and bool((partner[none] == -1).all()), f"{what}: a series without a result"
    j = torch.nonzero(has).flatten()
    if len(j) == 0:
        print(f"{what}: no series has a partner")
        return
    pj = partner[j].long()
    assert bool(((pj >= 0) & (pj < p) & (pj != j)).all()) and bool((w[pj] > 0).all()), f"{what}: an inadmissible partner"
    err = (rmin[j].double() - rmin64[j]).abs()
    worst = float((err / B[j].clamp_min(1e-300)).max())
    gap = r64_at(torch, T, w, j, pj) - rmin64[j]
    print(f"{what}: largest error / bound = {worst:.3f}, largest partner gap / 2 B = {float((gap / (2 * B[j]).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= B[j]).all()), f"{what}: (a) {float(err.max())}"
    assert bool((gap <= 2 * B[j]).all()), f"{what}: (b)"
    clear = second[j] - rmin64[j] > 2 * B[j]
    assert bool((pj[clear] == arg64[j][clear]).all()), f"{what}: (c)"


def bits(pair):
    import torch

    return torch.stack([pair[0].contiguous().view(torch.int32), pair[1].contiguous()])


def exact_reference(Ti, w):
    """small-integer series and w a power of two: everything is exact in float32 and in float64 -> (rmin float32, partner)"""
    T64, w64 = Ti.astype(np.float64), w.astype(np.float64)
    r = (T64 @ T64.T) * w64[:, None] * w64[None, :]
    p = r.shape[0]
    key = np.where((w64 > 0)[None, :] & ~np.eye(p, dtype=bool), r, np.inf)
    partner = np.argmin(key, axis=1)                                   # the first occurrence: the lowest index
    rmin = key[np.arange(p), partner]
    none = np.isinf(rmin) | ~(w64 > 0)
    assert np.array_equal(rmin.astype(np.float32).astype(np.float64), rmin)
    return np.where(none, np.nan, rmin).astype(np.float32), np.where(none, -1, partner).astype(np.int32)


def assert_exact(ctx, Ti, w, what=""):
    import torch
    from xeofs_amd import engine

    rmin, partner = engine.pairmin(ctx, Ti.astype(np.float32), w.astype(np.float32))
    want_v, want_i = exact_reference(Ti, w)
    got_v, got_i = rmin.cpu().numpy(), partner.cpu().numpy()
    bad = np.flatnonzero((got_i != want_i) | (got_v.view(np.int32) != want_v.view(np.int32)) & ~(np.isnan(got_v) & np.isnan(want_v)))
    assert bad.size == 0, f"{what}: series {bad[:5]}: got {got_v[bad[:5]]}, {got_i[bad[:5]]}, want {want_v[bad[:5]]}, {want_i[bad[:5]]}"
    assert got_v.dtype == np.float32 and got_i.dtype == np.int32 and isinstance(rmin, torch.Tensor)


# ------------------------------------------------------------------------------------------------ 1. every edge, random panels
@pytest.mark.parametrize("n", N_LIST)
def test_random_at_every_edge(ctx, n):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    for p in P_LIST:
        T, w = operands(torch, dev, n, p)
        got = engine.pairmin(ctx, T, w)
        assert got[0].is_cuda and got[1].is_cuda
        assert_within(torch, got, T, w, reference(torch, T, w), f"n={n} p={p}")


def test_the_plan_restated():
    assert [plan(p) for p in (1, 128, 129, 2048, 2049, 4352, 4353, 65408, 65409)] == [
        (1, 1), (1, 1), (2, 2), (16, 16), (17, 16), (34, 16), (35, 15), (511, 2), (512, 1)]
    assert SPLIT_CHANGES[:15] == list(range(2, 17)) and SPLIT_CHANGES[15] == 35 and SPLIT_CHANGES[-1] == 512
    assert len(SPLIT_CHANGES) == 30


@pytest.mark.parametrize("tiles", SPLIT_CHANGES + [17])
def test_either_side_of_every_change_of_the_split(ctx, tiles):
    """p = 128 (tiles - 1) is the last p of the old split count, p + 1 the first of the new one; tiles = 17 (p = 2049, n = 8) is
    the first p with fewer splits than tiles"""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    n = 8
    p1 = 128 * (tiles - 1) + 1
    if tiles != 17:
        assert plan(p1 - 1)[1] != plan(p1)[1]
    else:
        assert plan(p1 - 1) == (16, 16) and plan(p1) == (17, 16)
    T, w = operands(torch, dev, n, p1)
    for p in (p1 - 1, p1):
        Tp, wp = T[:p], w[:p].clone()
        got = engine.pairmin(ctx, Tp, wp)
        assert_within(torch, got, Tp, wp, reference(torch, Tp, wp), f"n={n} p={p} plan={plan(p)}")


# ------------------------------------------------------------------------------------------------ 2. designed, exact inputs
CORNERS = {300: [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 299],
           2100: [0, 127, 128, 1791, 1792, 1919, 1920, 2047, 2048, 2049, 2099]}       # 17 tiles, 16 splits: the last takes two


@pytest.mark.parametrize("p", [300, 2100])
def test_the_unique_minimum_moved_over_every_tile_corner(ctx, p):
    """all series are s_j v with small positive integers s_j, but one, -4 v: it is the partner of every other series, and its
    own partner is the lowest index with the largest s_j"""
    rng = np.random.default_rng(p)
    v = np.array([1, -2, 1, 0, 2, -1], dtype=np.int64)
    s = rng.integers(1, 4, p)
    w = 2.0 ** -rng.integers(1, 4, p)
    for i in CORNERS[p]:
        sc = s.copy()
        sc[i] = -4
        Ti = sc[:, None] * v[None, :]
        want_v, want_i = exact_reference(Ti, w)
        assert np.all(np.delete(want_i, i) == i)                       # the case is what it says
        assert_exact(ctx, Ti, w, f"p={p} minimum at {i}")


@pytest.mark.parametrize("p", [300, 2100])
def test_equal_minima_in_two_tiles_and_two_splits_the_lowest_index_wins(ctx, p):
    v = np.array([2, 1, -1, 1], dtype=np.int64)
    w = np.full(p, 0.25)
    places = {300: [(5, 6), (5, 70), (100, 140), (127, 128), (60, 299), (129, 257)],
              2100: [(3, 2099), (1900, 2050), (1919, 1920), (1930, 2047), (2047, 2048)]}[p]
    for lo, hi in places:
        sc = np.ones(p, dtype=np.int64)
        sc[[lo, hi]] = -3
        Ti = sc[:, None] * v[None, :]
        want_v, want_i = exact_reference(Ti, w)
        assert np.all(np.delete(want_i, [lo, hi]) == lo) and want_i[lo] == (1 if lo == 0 else 0)
        assert_exact(ctx, Ti, w, f"p={p} equal minima at {lo} and {hi}")


@pytest.mark.parametrize("p", [2, 129, 300, 2100])
def test_random_small_integers_with_many_ties(ctx, p):
    rng = np.random.default_rng(p + 1)
    Ti = rng.integers(-3, 4, (p, 8))
    w = 2.0 ** -rng.integers(0, 5, p).astype(np.float64)
    if p > 4:
        w[rng.integers(0, p, 3)] = 0.0
    assert_exact(ctx, Ti, w, f"p={p} integers")


def test_a_series_equal_to_its_own_negative_gives_minus_one(ctx):
    import torch
    from xeofs_amd import engine

    rng = np.random.default_rng(4)
    p = 260
    Ti = np.ones((p, 4), dtype=np.int64) * np.array([1, -1, 1, -1]) * rng.choice([1, -1], p)[:, None]
    Ti[::7] = np.array([1, 1, -1, -1])                                 # |T_j| = 2 everywhere: w = 1/2 is the exact norm
    w = np.full(p, 0.5)
    assert_exact(ctx, Ti, w, "r = -1")
    rmin, partner = engine.pairmin(ctx, Ti.astype(np.float32), w.astype(np.float32))
    anti = np.array([np.any(np.all(Ti == -Ti[j], axis=1)) for j in range(p)])
    assert anti.any() and bool((rmin.cpu().numpy()[anti] == -1.0).all())
    pi = partner.cpu().numpy()[anti]
    assert np.array_equal(Ti[pi], -Ti[anti]) and isinstance(rmin, torch.Tensor)


def test_the_diagonal_is_excluded_even_where_it_is_the_smallest(ctx):
    """series j = e, every other series 5 s_i e with s_i >= 1: d[j, j] = 1 < 5 <= d[j, i], and a zero series ties with
    everything at 0, itself included"""
    rng = np.random.default_rng(6)
    p = 200
    e = np.array([1, 0, 0], dtype=np.int64)
    for j in (0, 64, 127, 128, 199):
        Ti = (5 * rng.integers(1, 4, p))[:, None] * e[None, :]
        Ti[j] = e
        w = np.ones(p)
        want_v, want_i = exact_reference(Ti, w)
        assert want_i[j] != j and want_v[j] >= 5.0
        assert_exact(ctx, Ti, w, f"small diagonal at {j}")
        Ti[j] = 0
        want_v, want_i = exact_reference(Ti, w)
        assert want_v[j] == 0.0 and want_i[j] == (1 if j == 0 else 0)
        assert_exact(ctx, Ti, w, f"zero series at {j}")


def test_zero_scales_are_never_partners(ctx):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    n, p = 33, 300
    T, w = operands(torch, dev, n, p, seed=9)
    w = w.abs()
    off = torch.tensor([0, 5, 64, 127, 128, 129, 255, 256, 299], device=dev)
    w[off] = torch.tensor([0.0, -0.0, -1.0, float("nan"), 0.0, float("-inf"), 0.0, -2.0, 0.0], device=dev)
    rmin, partner = engine.pairmin(ctx, T, w)
    assert bool(torch.isnan(rmin[off]).all()) and bool((partner[off] == -1).all())
    assert not bool(torch.isin(partner.long(), off).any())
    assert_within(torch, (rmin, partner), T, w, reference(torch, T, w), "scales <= 0 or NaN")
    # all but one excluded: nobody has a partner
    for keep in (0, 128, 299):
        w1 = torch.zeros(p, device=dev)
        w1[keep] = 1.0
        rmin, partner = engine.pairmin(ctx, T, w1)
        assert bool(torch.isnan(rmin).all()) and bool((partner == -1).all())
    # two left: they are each other's partner, whatever the sign of their product
    w2 = torch.zeros(p, device=dev)
    w2[[3, 290]] = 1.0
    rmin, partner = engine.pairmin(ctx, T, w2)
    assert partner[3] == 290 and partner[290] == 3 and int((partner >= 0).sum()) == 2
    one = engine.pairmin(ctx, T[:1], w[1:2])
    assert bool(torch.isnan(one[0]).all()) and int(one[1][0]) == -1    # p == 1


# ------------------------------------------------------------------------------------------------ 3. what is read and written
@pytest.mark.parametrize("n,p", [(33, 65), (130, 129), (65, 300)])
def test_strides_padding_canaries_and_read_only_operands(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, w = operands(torch, dev, n, p, seed=2)
    plain = engine.pairmin(ctx, T, w)
    # rows past p hold series that would be everybody's partner, columns past n what would change every product
    Tbig = torch.full((p + 3, n + 5), 7.0, dtype=torch.float32, device=dev)
    Tbig[:p, :n] = T
    Tbig[p:, :n] = -50.0 * T[:3]
    wbig = torch.full((2 * (p + 3),), 1.0, dtype=torch.float32, device=dev)
    wbig[:2 * p:2] = w
    Tv, wv = Tbig[:p, :n], wbig[:2 * p:2]
    assert Tv.stride(0) == n + 5 and wv.stride(0) == 2
    T0, w0 = Tbig.clone(), wbig.clone()
    vbuf = torch.full((p + 16,), SENT_V, dtype=torch.float32, device=dev)
    ibuf = torch.full((p + 16,), SENT_I, dtype=torch.int32, device=dev)
    got = engine.pairmin(ctx, Tv, wv, out=(vbuf[8:8 + p], ibuf[8:8 + p]))
    assert got[0].data_ptr() == vbuf[8:].data_ptr() and got[1].data_ptr() == ibuf[8:].data_ptr()
    assert torch.equal(bits(got), bits(plain))                         # the strides and what lies past the panel change nothing
    assert bool((vbuf[:8] == SENT_V).all()) and bool((vbuf[8 + p:] == SENT_V).all())
    assert bool((ibuf[:8] == SENT_I).all()) and bool((ibuf[8 + p:] == SENT_I).all())
    assert torch.equal(Tbig.view(torch.int32), T0.view(torch.int32)) and torch.equal(wbig.view(torch.int32), w0.view(torch.int32))
    assert torch.equal(bits(engine.pairmin(ctx, Tv, wv)), bits(plain))  # two runs are equal bit for bit
    # a panel whose column stride is not 1 is honoured as colquad honours it: staged
    Tt = T.t().contiguous().t()
    assert Tt.stride(1) != 1 or p == 1
    assert torch.equal(bits(engine.pairmin(ctx, Tt, w)), bits(plain))


@pytest.mark.parametrize("n,p", [(8, 2100), (8, 4400)])
def test_bit_equal_reruns_across_splits(ctx, n, p):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, w = operands(torch, dev, n, p, seed=1)
    first = engine.pairmin(ctx, T, w)
    for _ in range(3):
        assert torch.equal(bits(engine.pairmin(ctx, T, w)), bits(first))


@pytest.mark.parametrize("n,p", [(33, 65), (65, 300), (8, 2100)])
def test_a_bad_series_stays_contained(ctx, n, p):
    """sample t0 is made positive in every series, so an infinity there gives d[j, bad] = +inf: never a minimum.  Every series
    whose partner in the clean run was neither bad series must come out bit for bit."""
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    T, w = operands(torch, dev, n, p, seed=3)
    w = w.abs().clamp_min(1e-3)
    t0 = n // 2
    T[:, t0] = T[:, t0].abs() + 0.5
    clean = engine.pairmin(ctx, T, w)
    Tb = T.clone()
    jn, ji = p // 3, p - 1
    Tb[jn, :] = float("nan")
    Tb[ji, t0] = float("inf")
    got = engine.pairmin(ctx, Tb, w)
    keep = (clean[1] != jn) & (clean[1] != ji)
    keep[jn] = keep[ji] = False
    assert int(keep.sum()) >= p - 12                                   # the minima do lie elsewhere
    assert torch.equal(bits(got)[:, keep], bits(clean)[:, keep])
    assert not bool(torch.isin(got[1][keep].long(), torch.tensor([jn, ji], device=dev)).any())
    assert bool(torch.isnan(got[0][jn])) and int(got[1][jn]) == -1     # every pair of the NaN series is NaN
    assert float(got[0][ji]) == float("inf") and int(got[1][ji]) == 0  # +inf with everybody: the lowest index
    others = ~keep
    others[jn] = others[ji] = False                                    # their partner went bad: the next one, a larger value
    assert bool((got[0][others] >= clean[0][others]).all()) and bool((got[1][others] >= 0).all())
    assert torch.equal(bits(engine.pairmin(ctx, T, w)), bits(clean))


# ------------------------------------------------------------------------------------------------ 4. limits and refusals
def test_refusals_before_any_launch(ctx):
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    dev = f"cuda:{ctx.device}"
    lib, h = ctx.lib, ctx.handle
    T = torch.zeros((3, 40), dtype=torch.float32, device=dev)
    w = torch.ones(3, dtype=torch.float32, device=dev)
    v = torch.full((3,), SENT_V, dtype=torch.float32, device=dev)
    x = torch.full((3,), SENT_I, dtype=torch.int32, device=dev)
    call = lambda n, ld, p=3: lib.eofx_pairmin_f32(h, ptr(T), p, n, ld, ptr(w), ptr(v), ptr(x))
    assert call(40, 39) == _lib.ERR_ARG                                # ld < n
    assert call(0, 40) == _lib.ERR_ARG                                 # n < 1
    assert call(40, 40, p=-1) == _lib.ERR_ARG
    assert call(40, 40, p=2 ** 31) == _lib.ERR_ARG                     # partner is an int32
    assert b"2^31" in lib.eofx_last_error(h)
    assert call(2 ** 30 + 1, 2 ** 30 + 1) == _lib.ERR_SHAPE            # checked by argument: nothing is launched
    assert call(2 ** 30 + 1, 2 ** 30 + 1, p=0) == _lib.ERR_SHAPE       # ... also when there is nothing to do
    assert call(40, 40, p=0) == _lib.EOFX_OK                           # p == 0: a no-op
    assert call(40, 39, p=0) == _lib.ERR_ARG                           # ... after the argument checks
    assert lib.eofx_pairmin_f32(h, None, 3, 40, 40, ptr(w), ptr(v), ptr(x)) == _lib.ERR_ARG
    assert lib.eofx_pairmin_f32(h, ptr(T), 3, 40, 40, None, ptr(v), ptr(x)) == _lib.ERR_ARG
    assert lib.eofx_pairmin_f32(h, ptr(T), 3, 40, 40, ptr(w), None, ptr(x)) == _lib.ERR_ARG
    assert lib.eofx_pairmin_f32(h, ptr(T), 3, 40, 40, ptr(w), ptr(v), None) == _lib.ERR_ARG
    assert lib.eofx_pairmin_f32(None, ptr(T), 3, 40, 40, ptr(w), ptr(v), ptr(x)) == _lib.ERR_ARG
    ctx.synchronize()
    assert bool((v == SENT_V).all()) and bool((x == SENT_I).all())
    empty = engine.pairmin(ctx, torch.zeros((0, 12), dtype=torch.float32, device=dev), torch.zeros(0, device=dev))
    assert tuple(empty[0].shape) == tuple(empty[1].shape) == (0,)
    assert empty[0].dtype == torch.float32 and empty[1].dtype == torch.int32
    with pytest.raises(ValueError, match="one entry per series"):
        engine.pairmin(ctx, T, w[:2])
    with pytest.raises(ValueError, match="one entry per series"):
        engine.pairmin(ctx, T, torch.ones((3, 1), device=dev))
    with pytest.raises(ValueError, match="out must be"):
        engine.pairmin(ctx, T, w, out=v)
    with pytest.raises(ValueError, match="out must be"):
        engine.pairmin(ctx, T, w, out=(v, x.float()))
    with pytest.raises(ValueError, match="out must be"):
        engine.pairmin(ctx, T, w, out=(torch.empty(4, dtype=torch.float32, device=dev), x))
    with pytest.raises(ValueError, match="out must be"):
        engine.pairmin(ctx, T, w, out=(torch.empty(6, dtype=torch.float32, device=dev)[::2], x))
    with pytest.raises(ValueError, match="matrix"):
        engine.pairmin(ctx, T[0], w)
    # host arrays are staged
    rng = np.random.default_rng(0)
    Th = rng.standard_normal((9, 5)).astype(np.float32)
    wh = (1.0 / np.linalg.norm(Th.astype(np.float64), axis=1))
    got = engine.pairmin(ctx, Th, wh)
    Td, wd = torch.from_numpy(Th).to(dev), torch.from_numpy(wh.astype(np.float32)).to(dev)
    assert_within(torch, got, Td, wd, reference(torch, Td, wd), "host operands")


# ------------------------------------------------------------------------------------------------ 5. the resident matrix
@pytest.mark.parametrize("n,P,in_place", [(33, 70, True), (130, 65, False), (65, 300, True)])
def test_resident_matrix_entry_equals_the_panel_entry(ctx, n, P, in_place):
    import torch
    from xeofs_amd import engine

    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(n + P)
    X = rng.standard_normal((n, P)).astype(np.float32)
    mat, _ = engine.preprocess(ctx, X, True, False, None, in_place=in_place)
    try:
        had = mat.has_sample_layout()
        Xt = mat.download()
        wh = (1.0 / np.linalg.norm(Xt.astype(np.float64), axis=0)).astype(np.float32)
        got = engine.mat_pairmin(ctx, mat, wh)
        assert tuple(got[0].shape) == tuple(got[1].shape) == (mat.p,)
        assert mat.has_sample_layout()                                 # built on demand, kept for the caller to release
        if not had:
            mat.release_sample_layout()
            assert not mat.has_sample_layout()
        Tp = torch.from_numpy(np.ascontiguousarray(Xt.T)).to(dev)
        wd = torch.from_numpy(wh).to(dev)
        assert torch.equal(bits(got), bits(engine.pairmin(ctx, Tp, wd)))
        assert_within(torch, got, Tp, wd, reference(torch, Tp, wd), f"resident n={n} P={P}")
        vbuf = torch.full((mat.p + 4,), SENT_V, dtype=torch.float32, device=dev)
        ibuf = torch.full((mat.p + 4,), SENT_I, dtype=torch.int32, device=dev)
        engine.mat_pairmin(ctx, mat, wd, out=(vbuf[2:2 + mat.p], ibuf[2:2 + mat.p]))
        assert torch.equal(bits((vbuf[2:2 + mat.p], ibuf[2:2 + mat.p])), bits(got))
        assert bool((vbuf[:2] == SENT_V).all()) and bool((vbuf[-2:] == SENT_V).all())
        assert bool((ibuf[:2] == SENT_I).all()) and bool((ibuf[-2:] == SENT_I).all())
        assert np.array_equal(mat.download(), Xt)                      # the field is read only
        with pytest.raises(ValueError, match="one entry per series"):
            engine.mat_pairmin(ctx, mat, wd[:-1])
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
        w = torch.ones(mat.p, dtype=torch.float32, device=dev)
        with pytest.raises(ValueError, match="masked"):
            engine.mat_pairmin(ctx, mat, w)
        v = torch.full((mat.p_phys,), SENT_V, dtype=torch.float32, device=dev)
        x = torch.full((mat.p_phys,), SENT_I, dtype=torch.int32, device=dev)
        assert ctx.lib.eofx_mat_pairmin_f32(ctx.handle, mat.handle, ptr(w), ptr(v), ptr(x)) == _lib.ERR_ARG
        assert b"masked" in ctx.lib.eofx_last_error(ctx.handle)
        assert ctx.lib.eofx_mat_pairmin_f32(ctx.handle, None, ptr(w), ptr(v), ptr(x)) == _lib.ERR_ARG
        ctx.synchronize()
        assert bool((v == SENT_V).all()) and bool((x == SENT_I).all())
    finally:
        mat.free()
