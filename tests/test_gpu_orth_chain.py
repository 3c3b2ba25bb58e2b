"""The kernels of the Cholesky-QR chain every randomized SVD here orthonormalises its panels with -- eofx_panel_rinv_f64
(chol_rinv_kernel up to 64 columns, launch_rinv_blocked beyond: chol_blocked_init / chol_rinv_kernel on the diagonal blocks /
dgemm64_kernel / chol_blocked_export, and the host route hostla::chol_rinv_padded), eofx_panel_matmul_f32
(panel_matmul_kernel<false>: the "fits in LDS" form, the windowed form, the triangular chunk skip) and their chain
eofx_panel_cholqr_f32 -- against the extended-precision reference of tests/orth_reference.py (checked on the CPU by
tests/test_orth_reference_cpu.py), at the edges of the 8-row register panels, the 16 x 16 inverse blocks, the 64-column
blocks and merge levels, the 32-row groups, the 64-column K chunks and the 256-row LDS windows.

Every output buffer arrives full of NaN: an element a route does not write shows.  That is how the defect this module was
written around was confirmed: for l <= 64 < L the one-workgroup kernel stores only its 64 x 64 block, and before
launch_rinv zeroed the rest, rows and columns 64 .. L-1 of R^-1 came back as they went in (test_rinv_one_workgroup with
L = 96 / 128; through eofx_panel_cholqr_f32 the product then read that memory).

Tolerances -- none is taken from the kernels' output.
  R^-1:     E = max |X - Xref|_ij sqrt(G_ii) / max |Xref_ij| sqrt(G_ii) (orth_reference.scaled_error), asserted against
            32 x max(E_numpy, 2^-53) with E_numpy the same figure for numpy.linalg.inv(numpy.linalg.cholesky(G).T) on the
            same case: the factor covers another fixed summation order, the Newton-refined rsq pivots and, on the blocked
            route, the log-depth of the merge levels -- a few ulp each.  A case listed in DERIVED_BOUND is held to the
            first-order bound 4 l 2^-53 kappa_2 (G scaled to a unit diagonal) instead; the list is empty: every case met
            32 x numpy.
  product:  |out - ref| <= 2^-24 |ref| + L 2^-52 (|P| |M|) elementwise: float64 FMAs, one rounding to float32.
  chain:    Q against fl32(P Rinv_dev) at the product bound; ||Q^T Q - I||_F over the live columns within 4 x the figure of
            Q_ref = fl32(P Xref) on the same case.
  f16x3:    2e-5 of the largest expected entry, the bound of test_hilbert_every_plan for the same consumer.

Measured on an MI355X.  E_kernel / max(E_numpy, 2^-53), with E_numpy between 5e-17 and 2.5e-16 -- every case on the
32 x numpy bound, none on the derived one:
  one workgroup (50 cases, dependent sets included)   0.63 .. 2.42
  blocked device route (11 cases, l = 65 .. 320)      0.93 .. 2.03
  host route, same cases                              1.29 .. 6.86   (no FMA; 6.86 at l = 320)
Product: the worst element of 505 shapes sits at 0.999 of its bound (the float32 rounding term; the float64 term is never
reached).  Chain: ||Q^T Q - I||_F equals the reference's to three digits in all five cases (3.5e-8 .. 4.7e-7).
"""

import functools

import numpy as np
import pytest

import orth_reference as oref

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
DERIVED_BOUND = set()          # test ids held to 4 l 2^-53 kappa_2 instead of 32 x numpy (see the module docstring)


def _up(l, m=32):
    return (l + m - 1) // m * m


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _nan(shape, dtype):
    import torch

    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# R^-1
# ------------------------------------------------------------------------------------------------------------------------
def _rinv(ctx, Gp, l):
    """eofx_panel_rinv_f64 through the library itself, into an output full of NaN"""
    import torch
    from xeofs_amd._lib import ptr, raise_for

    L = Gp.shape[0]
    Gd = _dev(Gp)
    out = _nan((L, L), torch.float64)
    raise_for(ctx.lib.eofx_panel_rinv_f64(ctx.handle, ptr(Gd), L, int(l), ptr(out)), ctx.handle)
    return _host(out)


def _dead_of(X, l):
    return [j for j in range(l) if X[j, j] == 0.0]


def _check_structure(X, l, dead=()):
    assert np.isfinite(X).all(), f"{np.count_nonzero(~np.isfinite(X))} elements not written (first at {np.argwhere(~np.isfinite(X))[0]})"
    assert not np.tril(X, -1).any(), "below the diagonal"
    assert not X[l:].any() and not X[:, l:].any(), "outside l x l"
    dead = list(dead)
    assert not X[dead].any() and not X[:, dead].any(), "dead rows / columns"


def _check_error(X, Gp, l, dead, tag, test_id):
    """the forward error of the live block against the reference without the dead columns, at 32 x numpy's on the same case
    (or, for the listed cases, the first-order bound)"""
    keep = np.setdiff1d(np.arange(l), list(dead))
    Gk = Gp[np.ix_(keep, keep)]
    Xref = oref.chol_rinv_ref(Gp, l, dead)[:l, :l]
    E = oref.scaled_error(X[:l, :l], Xref, Gp[:l, :l])
    En = oref.scaled_error(oref.numpy_rinv(Gk), Xref[np.ix_(keep, keep)], Gk)
    kappa = oref.unit_diagonal_cond(Gk)
    derived = 4 * l * U53 * kappa
    print(f"{tag}: l={l} L={Gp.shape[0]} dead={list(dead)} E_kernel={E:.3e} E_numpy={En:.3e} "
          f"ratio={E / max(En, U53):.2f} derived={derived:.3e} kappa={kappa:.2f}")
    assert E <= (derived if test_id in DERIVED_BOUND else 32 * max(En, U53))


ONE_WG = sorted({(l, L) for l in (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
                 for L in [_up(l)] + ([64] if l <= 32 else []) + ([96, 128] if l in (9, 64) else [])})


@pytest.mark.parametrize("l,L", ONE_WG)
def test_rinv_one_workgroup(ctx, l, L, request):
    """chol_rinv_kernel at the edges of its 8-row panels, its 16 x 16 inverse blocks and a full wave, in every padded width --
    L > 64 included, where the kernel's store loop ends at 64: every element written, exact zeros where R^-1 has none, the same
    bits twice, the forward error at 32 x numpy's"""
    G, _ = oref.design_gram(l, seed=l)
    Gp = oref.embed(G, L, fill=np.nan)                 # (outside l x l: never read)
    X = _rinv(ctx, Gp, l)
    _check_structure(X, l)
    assert _dead_of(X, l) == []
    assert _same_bits(X, _rinv(ctx, Gp, l))
    _check_error(X, Gp, l, (), "one workgroup", request.node.name)


NEAR_ONE_WG = [(l, j) for l in (9, 17, 64) for j in (2, 7, 8, 15, 16, 63) if j < l]


@pytest.mark.parametrize("l,j", NEAR_ONE_WG)
def test_rinv_one_workgroup_designed_column(ctx, l, j, request):
    """column j a distance rho from the span of two earlier ones: 1e-15 is dependent (pivot <= 1e-13 x its original diagonal
    entry) -- exact zero row and column, the rest the factor WITHOUT it --, 1e-11 is not (condition 1e11: classification,
    finiteness and structure only)"""
    L = _up(l)
    G, _ = oref.design_gram(l, seed=l, near={j: 1e-15})
    Gp = oref.embed(G, L, fill=np.nan)
    X = _rinv(ctx, Gp, l)
    assert _dead_of(X, l) == [j]
    _check_structure(X, l, [j])
    assert _same_bits(X, _rinv(ctx, Gp, l))
    _check_error(X, Gp, l, [j], "one workgroup, dependent column", request.node.name)
    G, _ = oref.design_gram(l, seed=l, near={j: 1e-11})
    X = _rinv(ctx, oref.embed(G, L, fill=np.nan), l)
    assert _dead_of(X, l) == []
    _check_structure(X, l)


DEAD_ONE_WG = oref.DEAD_ONE_WG


@pytest.mark.parametrize("case,l,kw,dead", DEAD_ONE_WG, ids=[c[0] for c in DEAD_ONE_WG])
def test_rinv_one_workgroup_dead_sets(ctx, case, l, kw, dead, request):
    """an all-zero column (original diagonal 0), column 0 zero, dependent columns in different 8-row panels, a pair dependent on
    the same two earlier columns, several across the 16-column inverse blocks: exactly the designed set, exact zeros there, the
    rest within tolerance of the reference without them"""
    L = _up(l)
    G, _ = oref.design_gram(l, seed=l, **kw)
    Gp = oref.embed(G, L, fill=np.nan)
    X = _rinv(ctx, Gp, l)
    assert _dead_of(X, l) == dead
    _check_structure(X, l, dead)
    assert _same_bits(X, _rinv(ctx, Gp, l))
    _check_error(X, Gp, l, dead, "one workgroup, " + case, request.node.name)


BLOCKED = oref.BLOCKED


@pytest.mark.parametrize("case,l,L,kw,dead", BLOCKED, ids=[c[0] for c in BLOCKED])
def test_rinv_blocked_and_host_routes(ctx, case, l, L, kw, dead, request, monkeypatch):
    """l > 64: the blocked device factorisation and the host route (EOFX_HOST_RINV, read per call) on the same input -- the same
    dependent set (late blocks are judged against the ORIGINAL diagonal, block edges 64 / 127 / 128), both within tolerance of
    the reference, every element of the L x L output written"""
    G, _ = oref.design_gram(l, seed=l, **kw)
    Gp = oref.embed(G, L, fill=np.nan)
    Xd = _rinv(ctx, Gp, l)
    assert _same_bits(Xd, _rinv(ctx, Gp, l))
    monkeypatch.setenv("EOFX_HOST_RINV", "1")
    Xh = _rinv(ctx, Gp, l)
    monkeypatch.delenv("EOFX_HOST_RINV")
    for route, X in (("blocked", Xd), ("host", Xh)):
        assert _dead_of(X, l) == (dead or []), route
        _check_structure(X, l, dead or [])
        if dead is not None:                       # (the live column at 1e-11: condition 1e11, classification and structure only)
            _check_error(X, Gp, l, dead, f"{route}, {case}", request.node.name + ":" + route)


# ------------------------------------------------------------------------------------------------------------------------
# P M
# ------------------------------------------------------------------------------------------------------------------------
MM_ROWS, MM_K, MM_COLS = 1029, 544, 130


@functools.lru_cache(maxsize=None)
def _mm_inputs(tri):
    """P float32 with column scales over 10^+-3; M float64, dense or with an exactly zero lower triangle"""
    rng = np.random.default_rng(11)
    P = (rng.standard_normal((MM_ROWS, MM_K)) * 10.0 ** rng.uniform(-3.0, 3.0, size=MM_K)).astype(np.float32)
    M = rng.standard_normal((MM_K, MM_COLS))
    return P, (np.triu(M) if tri else M)


@functools.lru_cache(maxsize=None)
def _mm_ref(L, tri, rows):
    """the reference and |P| |M| for the leading L columns / rows of the shared operands: every smaller row count and output
    width is a corner of these"""
    P, M = _mm_inputs(tri)
    P, M = P[:rows, :L], M[:L]
    return oref.matmul_ref(P, M), np.abs(P.astype(np.float64)) @ np.abs(M)


def _matmul(ctx, P, M):
    import torch
    from xeofs_amd._lib import ptr, raise_for

    Pd, Md = _dev(P), _dev(M)
    out = _nan((P.shape[0], M.shape[1]), torch.float32)
    raise_for(ctx.lib.eofx_panel_matmul_f32(ctx.handle, ptr(Pd), P.shape[0], P.shape[1], ptr(Md), M.shape[1], ptr(out)), ctx.handle)
    return _host(out)


def _check_product(out, ref, absprod, L, tag):
    assert np.isfinite(out).all(), f"{tag}: {np.count_nonzero(~np.isfinite(out))} elements not written"
    err = oref.to_f64(np.abs(oref.extended(out) - ref))
    bound = 2.0 ** -24 * oref.to_f64(np.abs(ref)) + L * 2.0 ** -52 * absprod
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), (tag, worst)


@pytest.mark.parametrize("tri", [False, True], ids=["dense", "zero-lower-triangle"])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 127, 129, 1029])
@pytest.mark.parametrize("L", [32, 96, 160, 256, 288, 544])
def test_panel_matmul_general_route(ctx, L, rows, tri):
    """panel_matmul_kernel<false>, upper = 0 (Lo < 256 keeps the call off the NT route): the "fits in LDS" form with 1, 2, 3 (the
    odd tail of the two-item loop) and 4 K chunks, the windowed form with a last window of one chunk (288) and three windows
    (544), row counts around the 32-row groups and the 128-row units, output widths around the 64-column blocks -- elementwise at
    the float64-FMA bound, every element written, the same bits twice.  M with an exactly zero lower triangle goes the same
    way: the general route skips nothing"""
    if tri and rows > 129:
        rows = 130                                  # (one more row count instead of a second 1029-row reference)
    P, M = _mm_inputs(tri)
    ref, absprod = _mm_ref(L, tri, 130 if tri else MM_ROWS)
    for Lo in (1, 3, 33, 64, 65, 130):
        Pc, Mc = np.ascontiguousarray(P[:rows, :L]), np.ascontiguousarray(M[:L, :Lo])
        out = _matmul(ctx, Pc, Mc)
        _check_product(out, ref[:rows, :Lo], absprod[:rows, :Lo], L, f"rows={rows} L={L} Lo={Lo} tri={tri}")
        assert _same_bits(out, _matmul(ctx, Pc, Mc))


def test_panel_matmul_past_the_grid_cap(ctx):
    """131072 + 160 rows at L = Lo = 32: 1026 units against the cap of 1024 workgroups, so the waves walk several 32-row groups
    and five of them get two items, the others one"""
    rows, L = 131072 + 160, 32
    rng = np.random.default_rng(5)
    P = (rng.standard_normal((rows, L)) * 10.0 ** rng.uniform(-3.0, 3.0, size=L)).astype(np.float32)
    M = rng.standard_normal((L, L))
    out = _matmul(ctx, P, M)
    _check_product(out, oref.matmul_ref(P, M), np.abs(P.astype(np.float64)) @ np.abs(M), L, f"rows={rows}")
    assert _same_bits(out, _matmul(ctx, P, M))


def test_panel_matmul_feeds_the_f16x3_product(ctx):
    """the product's output, entries from 1e-6 to 1e+6, as the panel of a split-fp16 pass (eofx_panel_tmul_f32, f16x3): the pass
    scales its fp16 planes by the panel's maximum -- recorded where the panel is written inside the SVD drivers, taken by the
    pass itself at this level of the ABI --, and a maximum that is not the real one shows as overflow or lost digits.  Against
    float64 at the bound of test_hilbert_every_plan for this consumer"""
    import torch
    from xeofs_amd import engine

    n, p, L = 300, 517, 64
    rng = np.random.default_rng(9)
    X = rng.standard_normal((n, p)).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    P = np.zeros((mat.n_pad, L), np.float32)
    P[:n] = rng.standard_normal((n, L))
    M = rng.standard_normal((L, L)) / np.sqrt(L) * 10.0 ** np.linspace(-6.0, 6.0, L)
    Zn = _nan((mat.n_pad, L), torch.float32)
    engine.panel_matmul(ctx, _dev(P), _dev(M), out=Zn)
    Z = _host(Zn).astype(np.float64)
    assert np.isfinite(Z).all() and not Z[n:].any()
    _check_product(Z.astype(np.float32), oref.matmul_ref(P, M), np.abs(P.astype(np.float64)) @ np.abs(M), L, "f16x3 feed")
    colmax = np.abs(Z).max(axis=0)
    assert colmax.min() < 1e-5 and colmax.max() > 1e5
    Y = _host(engine.panel_tmul(ctx, mat, Zn, prec="f16x3"))[:p].astype(np.float64)
    want = X.astype(np.float64).T @ Z[:n]
    assert np.abs(Y - want).max() <= 2e-5 * np.abs(want).max()
    mat.free()


# ------------------------------------------------------------------------------------------------------------------------
# the chain: Q = P R^-1, upper = 1
# ------------------------------------------------------------------------------------------------------------------------
# (515, 300, 320): column blocks 0 .. 3 of the triangular product take the "fits" form, block 4 (five K chunks) the windowed one
CHAIN = [
    (33, 5, 32, {3: (0, 1)}, []),
    (129, 64, 64, {8: (1, 5), 63: (2, 40)}, [31]),
    (257, 100, 128, {64: (3, 20), 77: (5, 70)}, []),
    (1029, 200, 224, {127: (2, 90), 128: (5, 100), 130: (3, 70)}, [0]),
    (515, 300, 320, {130: (3, 70), 299: (64, 256)}, [5]),
]


@functools.lru_cache(maxsize=None)
def _chain_case(rows, l, L):
    """P [rows x L] float32 (columns >= l zero; dependent columns = the float32 sum of two earlier ones: a residual of 2^-24, so a
    pivot ratio near 1e-15; zero columns) and its Gram matrix from the extended-precision product, rounded once"""
    dep, zero = next((d, z) for r, ll, LL, d, z in CHAIN if (r, ll, LL) == (rows, l, L))
    rng = np.random.default_rng(rows + l)
    D = 10.0 ** rng.uniform(-2.0, 2.0, size=l)
    B = rng.standard_normal((rows, l))
    for j, (a, b) in dep.items():
        B[:, j] = 0.8 * B[:, a] - 0.6 * B[:, b]
    P = np.zeros((rows, L), np.float32)
    P[:, :l] = (B * D).astype(np.float32)
    for j, (a, b) in dep.items():                    # exactly representable parents, then ONE rounding of the combination
        P[:, j] = (D[j] * (0.8 / D[a] * P[:, a].astype(np.float64) - 0.6 / D[b] * P[:, b].astype(np.float64))).astype(np.float32)
    P[:, zero] = 0.0
    G = oref.to_f64(oref.matmul_ref(P.T, P))
    G[l:] = np.nan
    G[:, l:] = np.nan
    return P, G, sorted(list(dep) + list(zero))


@pytest.mark.parametrize("rows,l,L", [c[:3] for c in CHAIN])
def test_cholqr_chain(ctx, rows, l, L):
    """eofx_panel_cholqr_f32 = R^-1 into the arena, then the product with upper = 1 (output column block b reads K chunks 0 .. b):
    Q equals fl32(P Rinv_dev) at the product's bound with Rinv_dev from eofx_panel_rinv_f64 on the same G (same kernels, fixed
    order) -- the chunk skip drops exact zeros only --, columns >= l and dependent columns are exact zeros, and Q is as
    orthonormal as the reference's Q is after its rounding to float32"""
    import torch
    from xeofs_amd import engine
    from xeofs_amd._lib import ptr, raise_for

    P, G, dead = _chain_case(rows, l, L)
    Pd, Gd = _dev(P), _dev(G)
    Rinv = _host(engine.panel_rinv(ctx, Gd, l))
    assert _dead_of(Rinv, l) == dead
    _check_structure(Rinv, l, dead)
    Q = _nan((rows, L), torch.float32)
    raise_for(ctx.lib.eofx_panel_cholqr_f32(ctx.handle, ptr(Pd), rows, L, l, ptr(Gd), ptr(Q)), ctx.handle)
    Q = _host(Q)
    _check_product(Q, oref.matmul_ref(P, Rinv), np.abs(P.astype(np.float64)) @ np.abs(Rinv), L, f"chain rows={rows} l={l}")
    assert not Q[:, l:].any() and not Q[:, dead].any()
    Q2 = _nan((rows, L), torch.float32)
    raise_for(ctx.lib.eofx_panel_cholqr_f32(ctx.handle, ptr(Pd), rows, L, l, ptr(Gd), ptr(Q2)), ctx.handle)
    assert _same_bits(Q, _host(Q2))
    live = np.setdiff1d(np.arange(l), dead)
    Qref = oref.to_f64(oref.matmul_ref(P, oref.chol_rinv_ref(G, l, dead))).astype(np.float32)

    def departure(Qm):
        Ql = Qm[:, live].astype(np.float64)
        return float(np.linalg.norm(Ql.T @ Ql - np.eye(live.size)))
    e, eref = departure(Q), departure(Qref)
    print(f"chain rows={rows} l={l} L={L}: ||QtQ - I||_F = {e:.3e}, reference {eref:.3e}, ratio {e / eref:.2f}")
    assert e <= 4 * eref
