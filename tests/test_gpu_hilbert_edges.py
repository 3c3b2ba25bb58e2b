"""The Hilbert stage at its edges, feature by feature against the float64 oracle (`orc.hilbert_transform`):
hilbert_fft_kernel<L, MODE> (csrc/eofx_hfft.hpp), the hipFFT route's hilbert_pack / filter / unpack kernels
(csrc/eofx_kernels.hpp), and the entries eofx_hilbert_f32 / eofx_hilbert_sumsq_f64 (csrc/eofx_abi.hip).

error measure  `check_groups` (tests/test_hilbert_edges_checker_cpu.py): every feature against the scale of its own transform
               group -- the pair {2j, 2j + 1} for series of up to 8192 samples (two features share one complex transform),
               the feature alone for longer series -- never against the maximum of the field
tolerance      2e-6 on the one-kernel route, 2e-5 on the hipFFT route (the header of tests/test_gpu_complex.py)
inputs         the generator of test_hilbert_every_plan (travelling waves, per-feature trends and offsets of the waves' order)
               times a per-feature factor; uncentred through `from_dense` unless the case is about an in-place input
dirty pool     before the stage runs, the context's pool holds buffers of the outputs' padded size full of 1e3
               (`_dirty_pool`): whatever the stage leaves unwritten shows
padding        the padded buffers are not downloadable, so the tail rows [n, n_pad) and the padding features are checked through
               what reads them: `sumsq()` runs over the whole padded buffer and must equal the float64 sum of squares of the
               downloaded n x p block to 1e-11, and the exact-f32 products with panels that are non-zero in THEIR padding
               rows must come back with exact zeros in the output's padding rows and the float64 product elsewhere

Every test prints the largest error / scale it met, next to its tolerance.  On an MI355X with 256 CUs: A 1.82e-6 (n = 8193,
"exp"; 1.69e-6 at 4097, 1.45e-6 at 2049 -- the padded transform of the longest series of a plan is the closest to 2e-6; without
padding at most 4.6e-7), B 1.47e-6, D 1.06e-6, F 1.32e-6 of 2e-6; C 1.15e-6 of 2e-5; E at most 1.0e-6 relative against bounds of
2.7e-5 and more; the real part everywhere below 2.4e-7.
"""

import numpy as np
import pytest

from oracle import eof_oracle as orc
from test_hilbert_edges_checker_cpu import check_groups, own_group, pair_group

pytestmark = pytest.mark.gpu

TOL_FUSED, TOL_FFT = 2e-6, 2e-5
DECAY = 0.35
PAIR_FACTORS = np.array([1.0, 1e-3, 1e3, 1.0, 1e3, 1e-3, 1.0, 1.0])
N_LONG = 16385                  # first length of the hipFFT route


def _up(x, m):
    return (x + m - 1) // m * m


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _per_cu_ub(P):
    """upper bound on the workgroups per CU of launch_hilbert_fused (its LDS size adds the skew and 1536 bytes)"""
    return min(163840 // (8 * P), 2048 // (P // 16))


def _engine_grid(P, cus):
    """the grid cap of launch_hilbert_fused itself (plan<L>::lds = phys(P) * 8 + 1536): only to lay out the factors below"""
    lds = (P + 2 * (P >> 4) + 16 * (P >> 8)) * 8 + 1536
    return cus * max(1, min(163840 // lds, 2048 // (P // 16)))


def _trip_factors(p, per_item, grid):
    """1, 1e-3, 1e3, 1, 1e3, 1e-3, 1, 1 by PAIR of features (both features of a pair equal): neighbouring pairs differ by up to
    1e6.  With 256 CUs every grid is a multiple of 8, and the plain cycle would hand a workgroup the same factor on every trip:
    the cycle advances one place per lap of the grid (per_item features per work item), so a later trip's item differs from
    the one the workgroup held before"""
    f = np.arange(p)
    return PAIR_FACTORS[(f // 2 + (f // per_item) // grid) % 8]


def _alternating(p):
    return np.where(np.arange(p) % 2 == 0, 1e3, 1e-3)


def _field(n, p, seed, factors=None):
    """test_hilbert_every_plan's field: travelling waves + noise + a common and a per-feature trend + per-feature offsets"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = (3.0 * np.cos(0.21 * t - 2 * x) + 1.7 * np.cos(0.37 * t + 3 * x + 0.4) + 0.9 * np.sin(0.11 * t - x) + 0.01 * t
         + 0.3 * rng.standard_normal((n, p)))
    X += 0.002 * t * rng.standard_normal(p)[None, :] + rng.standard_normal(p)[None, :]
    if factors is not None:
        X *= np.asarray(factors)[None, :]
    return X.astype(np.float32)


def _reference(X64, padding):
    """analytic signal of the float64 copy of what the engine was given, both parts centred (hilbert_transform.py:40-72)"""
    ref = orc.hilbert_transform(X64, padding=padding, decay_factor=DECAY)
    return ref - ref.mean(axis=0)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dirty_pool(ctx, n, p, padding):
    """A same-shape matrix full of 1e3 goes through one `engine.hilbert` call and back to the pool (test_hilbert_every_plan) --
    and, because `from_dense` zeroes the padding of what it writes, the six buffers that leaves in the pool are then taken
    out again by matrices of the PADDED shape: every element of every buffer the stage will be handed is 1e3, the tail rows
    and the padding features included."""
    from xeofs_amd import engine

    ctx.trim()
    dirty = engine.from_dense(ctx, np.full((n, p), 1.0e3, np.float32))
    for m in engine.hilbert(ctx, dirty, padding, DECAY, want_real=True):
        m.free()
    dirty.free()
    full = np.full((_up(n, 512), _up(p, 512)), 1.0e3, np.float32)
    for m in [engine.from_dense(ctx, full) for _ in range(3)]:
        m.free()


def _assert_padding_zero(ctx, m, D, what, f16=False):
    """the tail rows [n, n_pad) and the padding features [p, p_pad) of the resident matrix `m` (download D) are zero, seen
    through `sumsq()` and the products (module docstring); f16: also the split-fp16 products at test_hilbert_every_plan's
    2e-5 (the recorded absmax is usable)"""
    import torch

    from xeofs_amd import engine

    n, p = D.shape
    assert (m.n, m.p, m.n_pad, m.p_pad) == (n, p, _up(n, 512), _up(p, 512)), what
    D64 = D.astype(np.float64)
    ss = float((D64 ** 2).sum())
    assert abs(m.sumsq() - ss) <= 1e-11 * ss, f"{what}: sumsq over the padded buffer {m.sumsq()!r} != {ss!r} over the n x p block"
    g = torch.Generator(device="cuda").manual_seed(n + p)
    Y = torch.rand((m.p_pad, 32), device="cuda", generator=g) + 0.5      # positive everywhere, the padding rows included
    Z = torch.rand((m.n_pad, 32), device="cuda", generator=g) + 0.5
    for prec in ("f32", "f16x3") if f16 else ("f32",):
        for got, want, rows, name in ((engine.panel_mul(ctx, m, Y, prec=prec), D64 @ Y[:p].double().cpu().numpy(), n, "X Y"),
                                      (engine.panel_tmul(ctx, m, Z, prec=prec), D64.T @ Z[:n].double().cpu().numpy(), p, "X^T Z")):
            torch.cuda.synchronize()
            got = got.double().cpu().numpy()
            assert np.isfinite(got).all(), f"{what} {name} {prec}"
            assert not got[rows:].any(), f"{what} {name} {prec}: the matrix is not zero beyond its {rows} rows of this product"
            assert np.abs(got[:rows] - want).max() <= 2e-5 * max(np.abs(want).max(), 1e-30), f"{what} {name} {prec}"


def _sumsq_bound(ref, part, tol):
    """element-wise |got - part| <= tol max|ref| gives ||got - part||_F <= rho ||part||_F with
    rho = tol sqrt(n p) max|ref| / ||part||_F, hence | ||got||^2 - ||part||^2 | <= (2 rho + rho^2) ||part||^2"""
    n, p = part.shape
    rho = tol * np.sqrt(n * p) * np.abs(ref).max() / np.linalg.norm(part)
    return 2 * rho + rho ** 2


def _run_uncentred(ctx, X, padding, group, tol, what, scale_ref=None, f16=False):
    """the assertions of test A on the written, uncentred matrix of X: both parts per group, the sums of squares, the padding
    of both outputs from a dirty pool, and the same bits without the real part; -> (Im, Re) as downloaded"""
    from xeofs_amd import engine

    n, p = X.shape
    ref = _reference(X.astype(np.float64), padding)
    scale_ref = ref if scale_ref is None else scale_ref(ref)
    mat = engine.from_dense(ctx, X)
    _dirty_pool(ctx, n, p, padding)
    B, A2 = engine.hilbert(ctx, mat, padding, DECAY, want_real=True)
    b, a = B.download(), A2.download()
    r_im = check_groups(b, ref.imag, scale_ref, group, tol, f"{what} Im")
    r_re = check_groups(a, ref.real, scale_ref, group, tol, f"{what} Re")
    print(f"hilbert-edges {what}: Im {r_im:.3g} Re {r_re:.3g} of the group's scale (tolerance {tol:.0e})")
    for m, d, part, name in ((B, b, ref.imag, "Im"), (A2, a, ref.real, "Re")):
        ss = float((part ** 2).sum())
        assert abs(m.sumsq() - ss) <= _sumsq_bound(ref, part, tol) * ss, f"{what} {name}: sumsq"
        _assert_padding_zero(ctx, m, d, f"{what} {name}", f16=f16)
    B2, none = engine.hilbert(ctx, mat, padding, DECAY)
    assert none is None and _same_bits(B2.download(), b), f"{what}: Im differs without the real part"
    for m in (mat, B, A2, B2):
        m.free()
    return b, a


# ---------------------------------------------------------------------------------------------------------------------
# A. later trips of the persistent pair loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", ["exp", None])
@pytest.mark.parametrize("n,L", [(33, 10), (513, 11), (1025, 12), (2049, 13), (4097, 14), (8193, 15)])
def test_later_trips_of_the_pair_loop(ctx, n, L, padding):
    """launch_hilbert_fused caps the grid at CUs * per_cu; the field has more pairs than an upper bound of that cap, so
    workgroups take a second pair (the first two where the bound is the engine's own figure, L = 13, 14 and MODE 1; about
    40 % of them at L = 10 .. 12): the prefetch `load_pair(pair + stride)` during the inverse stages and the one past the end, the
    reuse of coef / edge / red1 / red2 in LDS, the `fresh()` barriers -- and the odd last feature arrives on a later trip.
    The smallest n of every plan; the pair a workgroup held one trip earlier and the neighbouring pairs are up to 1e6 apart."""
    cus = _cus()
    if L <= 14:
        cap = cus * _per_cu_ub(1 << L)
        p = 2 * cap + 3
        assert p > 2 * cap and (p + 1) // 2 > cap and p % 2 == 1
        group, factors = pair_group(p), _trip_factors(p, 2, _engine_grid(1 << L, cus))
    else:                       # MODE 1: one feature per workgroup of plan<14>, one workgroup per CU
        cap = cus * 1
        p = cap + 3
        assert p > cap
        group, factors = own_group, _trip_factors(p, 1, _engine_grid(1 << 14, cus))
    _run_uncentred(ctx, _field(n, p, n, factors), padding, group, TOL_FUSED, f"A n={n} p={p} {padding}")


# ---------------------------------------------------------------------------------------------------------------------
# B. disparity inside a pair / between neighbours; a constant and an all-zero column
# ---------------------------------------------------------------------------------------------------------------------
CONST_COL, ZERO_COL = 4, 7          # partners 5 (factor 1e-3) and 6 (factor 1e3)


def _disparity_field(n, p=10):
    f = _alternating(p)
    X = _field(n, p, n, f)
    c = np.float32(2.0 * f[CONST_COL ^ 1])       # at the wave amplitude of its live partner
    X[:, CONST_COL] = c
    X[:, ZERO_COL] = 0.0
    return X, float(c)


@pytest.mark.parametrize("padding", ["exp", None])
@pytest.mark.parametrize("n", [200, 700, 1500, 3000, 6000])
def test_disparity_inside_a_pair(ctx, n, padding):
    """features of 1e3 and 1e-3 in ONE complex transform: each is within 2e-6 of its PAIR's scale -- the known trade of sharing
    a transform, the small feature carries the large one's rounding -- and of nothing larger.  A constant column (its transform
    is the cancellation T c + c0 u3) and an all-zero column, each beside a live feature, are bounded by their pair's scale."""
    X, _ = _disparity_field(n)
    _run_uncentred(ctx, X, padding, pair_group(X.shape[1]), TOL_FUSED, f"B n={n} {padding}")


@pytest.mark.parametrize("padding", ["exp", None])
def test_disparity_between_neighbours_one_feature_per_workgroup(ctx, padding):
    """n = 9000 (MODE 1): features of 1e3 and 1e-3 side by side, each within 2e-6 of its OWN scale; the all-zero column comes
    back as exact zeros in both parts.  The constant column's centred reference is zero, so its own scale is that of the series
    the kernel transformed, |c| (the rounding of T c + c0 u3 is relative to c: the bound presumes offsets at or below the
    amplitude, and this column is all offset)."""
    n = 9000
    X, c = _disparity_field(n)

    def scale_ref(ref):
        s = ref.copy()
        s[:, CONST_COL] += c
        return s

    b, a = _run_uncentred(ctx, X, padding, own_group, TOL_FUSED, f"B n={n} {padding}", scale_ref=scale_ref)
    assert not b[:, ZERO_COL].any() and not a[:, ZERO_COL].any()


# ---------------------------------------------------------------------------------------------------------------------
# in-place inputs (C, D): the Scaler map on the fly, the transient sample-contiguous copy from a dirty pool
# ---------------------------------------------------------------------------------------------------------------------
def _in_place_case(ctx, n, P, padding, group, tol, what, masked=False, for_hilbert=False, want_real=False):
    """standardised, weighted, preprocessed in place (the pool is dirty BEFORE the preprocess: the raw sample-contiguous layout
    of for_hilbert comes from it, and so does the transient copy of the stage); against the oracle's Hilbert transform of
    orc.preprocess(...)["X"], per group; a second call returns the same bits.  masked: 30 % all-NaN columns."""
    from xeofs_amd import engine

    rng = np.random.default_rng(n + P)
    X = _field(n, P, n + 1, _alternating(P))
    dead = np.sort(rng.choice(P, size=int(0.3 * P), replace=False)) if masked else np.zeros(0, int)
    X[:, dead] = np.nan
    live = np.setdiff1d(np.arange(P), dead)
    w = rng.uniform(0.4, 1.3, size=P)
    pre = orc.preprocess(X.astype(np.float64), True, True, w)["X"]
    ref = _reference(pre, padding)
    _dirty_pool(ctx, n, P, padding)
    A, _ = engine.preprocess(ctx, X, True, True, w, in_place=True, allow_masked=masked, for_hilbert=for_hilbert)
    if masked:
        # apply_plan (eofx_plans.hpp) keeps a mask in place only when n < valid features; at a test's size a series of 8193
        # samples or more has fewer, so the field is compacted into written layouts, silently -- the masked in-place layout is
        # out of reach here, and the call must still give the transform of the valid features.  (Measured once at the sizes that
        # reach it, 8193 x 11776 and 16385 x 23552 with 30 % masked, standardised, weighted, from a pool full of 1e3: exact
        # zeros at the masked columns, the rest bit-identical to the compaction route, both paddings.)
        assert n >= live.size and not A.masked and A.p == live.size and A.layout() == (True, False), what
    else:
        assert not A.masked and A.p == P and A.layout() == (False, True), what
    B, A2 = engine.hilbert(ctx, A, padding, DECAY, want_real=want_real)
    if not masked:
        assert A.layout() == (False, True) and not A.has_sample_layout(), what      # the copy was transient
        assert B.layout()[0] is False and B.has_sample_layout(), what               # lean: the sample-contiguous layout only
    b = B.download()
    r = check_groups(b, ref.imag, ref, group, tol, f"{what} Im")
    print(f"hilbert-edges {what}: Im {r:.3g} of the group's scale (tolerance {tol:.0e})")
    if want_real:
        a = A2.download()
        r = check_groups(a, ref.real, ref, group, tol, f"{what} Re")
        print(f"hilbert-edges {what}: Re {r:.3g} of the group's scale (tolerance {tol:.0e})")
        _assert_padding_zero(ctx, A2, a, f"{what} Re")
    _assert_padding_zero(ctx, B, b, f"{what} Im")
    if masked:      # the compaction route asked for by name (test_masked_field_through_hilbert_and_complex_rsvd_in_place's bound)
        A0, _ = engine.preprocess(ctx, X, True, True, w)
        B0, _ = engine.hilbert(ctx, A0, padding, DECAY)
        b0 = B0.download()
        assert np.abs(b - b0).max() <= 2e-6 * np.abs(b0).max(), what
        A0.free(); B0.free()
    B2, _ = engine.hilbert(ctx, A, padding, DECAY)        # (a for_hilbert buffer is gone by now, used or not)
    assert _same_bits(B2.download(), B.download()), f"{what}: a second call returns other bits"
    for m in (A, B, A2, B2):
        if m is not None:
            m.free()
    return b


# ---------------------------------------------------------------------------------------------------------------------
# C. the hipFFT route at its first length
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", ["exp", None])
def test_long_route_uncentred_both_parts(ctx, padding):
    """n = 16385, uncentred, with the real part (the At branch of hilbert_unpack_kernel): both parts within 2e-5 of the
    feature's own scale with features 1e6 apart side by side, both sums of squares, both outputs zero in their padding from a
    dirty pool and usable by the f32 and split-fp16 products (the recorded absmax), the same bits without the real part"""
    X = _field(N_LONG, 5, 11, _alternating(5))
    _run_uncentred(ctx, X, padding, own_group, TOL_FFT, f"C n={N_LONG} {padding}", f16=True)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("padding", ["exp", None])
def test_long_route_in_place_input(ctx, padding, masked):
    """n = 16385 from an in-place (lean) input, and from a field with a mask (see _in_place_case: compacted at this size)"""
    _in_place_case(ctx, N_LONG, 8, padding, own_group, TOL_FFT, f"C in place n={N_LONG} {padding} masked={masked}", masked=masked)


# ---------------------------------------------------------------------------------------------------------------------
# D. MODE 1 (and the declined raw-layout shortcut) from in-place inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("for_hilbert", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [8193, 16384])
def test_one_feature_per_workgroup_from_in_place_input(ctx, n, masked, for_hilbert):
    """MODE 1 loads whole 8-byte pairs up to n_pad and relies on the zero tail of the row it is given -- here the transient
    copy of an in-place matrix, taken from a dirty pool (n = 8193: sample 8193 shares its load with the last sample).  The
    raw-layout shortcut of for_hilbert is limited to L <= 14: it is declined and the stage gives the same transform."""
    _in_place_case(ctx, n, 8, "exp", own_group, TOL_FUSED, f"D n={n} masked={masked} for_hilbert={for_hilbert}", masked=masked,
                   for_hilbert=for_hilbert)


def test_raw_layout_shortcut_is_declined_when_the_real_part_is_wanted(ctx):
    """for_hilbert=True at n = 700, asked for the real part: the kernel's Scaler-map route has no At branch, the stage builds
    the transient copy instead"""
    _in_place_case(ctx, 700, 12, "exp", pair_group(12), TOL_FUSED, "D n=700 for_hilbert want_real", for_hilbert=True, want_real=True)


def _check_physical(B, ref, live, P, tol, what):
    """Im of a masked in-place matrix is a written matrix over the PHYSICAL columns: exact zeros at the masked grid points
    (`oscale` in hilbert_fft_kernel: a masked feature shares its transform with whatever lies beside it), every valid
    feature within tol of its physical pair's scale.  ref: the oracle over the valid features."""
    assert B.p == P and not B.masked, what
    b = B.download()
    assert not b[:, np.setdiff1d(np.arange(P), live)].any(), f"{what}: masked grid points are not exact zeros"
    phys = np.zeros((ref.shape[0], P), dtype=np.complex128)
    phys[:, live] = ref
    r = check_groups(b, phys.imag, phys, pair_group(P), tol, what)
    print(f"hilbert-edges {what}: Im {r:.3g} of the physical pair's scale (tolerance {tol:.0e})")


@pytest.mark.parametrize("masked", [False, True])
def test_raw_layout_route_over_several_trips(ctx, masked):
    """for_hilbert=True at test A's feature count for L = 10: the kernel reads the raw sample-contiguous layout the statistics
    pass wrote (into a buffer from a dirty pool) and applies the Scaler map `aff` -- and the zero columns of a mask, `oscale`
    -- to the prefetched registers of every later trip.  eofx_hilbert_f32 and eofx_hilbert_sumsq_f64 each consume one."""
    from xeofs_amd import engine

    n, cus = 300, _cus()
    P = _up(2 * cus * _per_cu_ub(1024) + 3, 4)
    assert P // 2 > cus * _per_cu_ub(1024)
    rng = np.random.default_rng(P)
    X = _field(n, P, 17, _trip_factors(P, 2, _engine_grid(1024, cus)))
    live = np.arange(P)
    if masked:
        live = np.setdiff1d(live, rng.choice(P, size=int(0.3 * P), replace=False))
        X[:, np.setdiff1d(np.arange(P), live)] = np.nan
    w = rng.uniform(0.4, 1.3, size=P)
    ref = _reference(orc.preprocess(X.astype(np.float64), True, False, w)["X"], "exp")
    what = f"D raw layout n={n} P={P} masked={masked}"
    _dirty_pool(ctx, n, P, "exp")
    A, _ = engine.preprocess(ctx, X, True, False, w, in_place=True, allow_masked=masked, for_hilbert=True)
    assert A.masked == masked and A.p == live.size and A.layout() == (False, True), what
    B, _ = engine.hilbert(ctx, A, "exp", DECAY)
    assert A.layout() == (False, True) and not A.has_sample_layout() and B.layout()[0] is False, what
    _check_physical(B, ref, live, P, TOL_FUSED, what)
    A2, _ = engine.preprocess(ctx, X, True, False, w, in_place=True, allow_masked=masked, for_hilbert=True)
    sq, want = engine.hilbert_sumsq(ctx, A2, "exp", DECAY), float((ref.imag ** 2).sum())
    assert abs(sq - want) <= _sumsq_bound(ref, ref.imag, TOL_FUSED) * want, what
    assert abs(sq - B.sumsq()) <= 1e-6 * B.sumsq(), what
    for m in (A, A2, B):
        m.free()


# ---------------------------------------------------------------------------------------------------------------------
# E. engine.hilbert_sumsq on every route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["written", "in_place", "masked"])
@pytest.mark.parametrize("padding", ["exp", None])
@pytest.mark.parametrize("n", [300, 8193, N_LONG])
def test_hilbert_sumsq_every_route(ctx, n, padding, kind):
    """the sum of squares of the imaginary part without writing it: the one-kernel route's per-wave partials over several
    trips (n = 300 at test A's feature count), and the two materialising fallbacks (L = 15, hipFFT).  Bound from the
    element-wise tolerance (`_sumsq_bound`); equal to the materialised part's sumsq() to 1e-6; without padding the decay
    factor is ignored (and keys ONE cached setup)."""
    from xeofs_amd import engine

    cus = _cus()
    if n == 300:
        p = 2 * cus * _per_cu_ub(1024) + 3
        factors = lambda q: _trip_factors(q, 2, _engine_grid(1024, cus))
    else:
        p, factors = (7 if n == 8193 else 5), _alternating
    tol = TOL_FFT if n > 16384 else TOL_FUSED
    what = f"E n={n} {padding} {kind}"
    if kind == "written":
        assert p % 2 == 1
        X = _field(n, p, n, factors(p))
        ref = _reference(X.astype(np.float64), padding)
        A = engine.from_dense(ctx, X)
    else:
        P = _up(p, 4)                                    # the in-place layouts need P % 4 == 0
        X = _field(n, P, n, factors(P))
        live = np.arange(P)
        if kind == "masked":
            live = np.setdiff1d(live, np.random.default_rng(P).choice(P, size=int(0.3 * P), replace=False))
            X[:, np.setdiff1d(np.arange(P), live)] = np.nan
        ref = _reference(orc.preprocess(X.astype(np.float64), True, False, None)["X"], padding)
        A, _ = engine.preprocess(ctx, X, True, False, None, in_place=True, allow_masked=(kind == "masked"))
        if kind == "masked" and n >= live.size:          # (compacted: see _in_place_case)
            assert not A.masked and A.p == live.size, what
        else:
            assert A.masked == (kind == "masked") and A.layout() == (False, True) and A.p == live.size, what
    want = float((ref.imag ** 2).sum())
    bound = _sumsq_bound(ref, ref.imag, tol)
    sq = engine.hilbert_sumsq(ctx, A, padding, DECAY)
    print(f"hilbert-edges {what}: sumsq off by {abs(sq - want) / want:.3g} (bound {bound:.3g})")
    assert abs(sq - want) <= bound * want, what
    B, _ = engine.hilbert(ctx, A, padding, DECAY)
    assert abs(sq - B.sumsq()) <= 1e-6 * B.sumsq(), what
    if A.masked:        # Im over the PHYSICAL columns: exact zeros at the masked ones, also beside a live partner in a pair
        _check_physical(B, ref, live, X.shape[1], tol, what)
    else:
        check_groups(B.download(), ref.imag, ref, pair_group(ref.shape[1]) if n <= 8192 else own_group, tol, what)
    assert engine.hilbert_sumsq(ctx, A, padding, DECAY) == sq, f"{what}: a second call returns another value"
    if padding is None:
        assert engine.hilbert_sumsq(ctx, A, None, 0.05) == sq and engine.hilbert_sumsq(ctx, A, None, 7.0) == sq, what
    A.free(); B.free()


# ---------------------------------------------------------------------------------------------------------------------
# F. short series and lengths at a plan's upper end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", ["exp", None])
@pytest.mark.parametrize("p", [1, 2, 7])
@pytest.mark.parametrize("n", [3, 5, 31, 512, 2048, 4096])
def test_short_and_boundary_lengths(ctx, n, p, padding):
    """series shorter than 33 samples (almost every lane of the workgroup is idle; the linear fit on 3 points), and n = 512,
    2048, 4096: the last sample sits in a thread's eighth register (cl = 7, tl = NT - 1) and n = n_pad = P / 2"""
    _run_uncentred(ctx, _field(n, p, 100 * n + p), padding, pair_group(p), TOL_FUSED, f"F n={n} p={p} {padding}")
