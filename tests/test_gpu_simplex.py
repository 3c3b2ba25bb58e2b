"""GPU tests of the two operators of archetypal analysis (engine.simplex_rows, engine.simplex_pg; csrc/eofx_simplex.hpp) against
the float64 restatement (tests/aa_reference.py) on the same float32 operands.

simplex_rows: out_i = the Euclidean projection of u_i = fmaf(-step, G_i, V_i) onto the probability simplex.  With u given
exactly (G absent, or step a power of two so that the product is exact and the fmaf is one float32 addition) the kernel's only
roundings are those of tau in float64 (about m 2^-53 max|u|) and the one rounding of out_j = u_j - tau <= 1 to float32 (at most
2^-24), so

    out >= 0,    |sum_j out_ij - 1| <= (|S_i| + 2) 2^-24,    |out_ij - ref_ij| <= 2^-23 max(1, max_j |u_ij|)  =: b_i,

and the support equals the reference's wherever |u_ij - tau_i| > b_i.  With a general step the test restates u in float64 and
rounds it, which can differ from the fmaf by one rounding of u: then tau moves by at most 2^-24 max_S |u| and entry j by
2^-24 |u_ij| more, so the bound is b_i + 2^-23 max_j |u_ij| <= 2^-22 max(1, max_j |u_ij|) (test_general_step).

simplex_pg: T iterations of a <- P(a - inv_L (a M - q)).  One iteration rounds: the k-term fmaf chain acc_j (at most
k 2^-24 sum_l |a_l| |M_lj|), the subtraction of q_j (2^-24 (|acc_j| + |q_j|)), the fmaf with inv_L and a_j (inv_L times what
came before, plus 2^-24 |u_j|), and the one rounding of the projection (2^-24 out_j).  With a on the simplex,
sum_l |a_l| |M_lj| <= max_l |M_lj| =: m_j and |u_j| <= |a_j| + c_j with c_j = inv_L (m_j + |q_j|), so per row, in the 2-norm
(|a|_2 <= 1, |out|_2 <= 1),

    delta_i = 2^-24 ((k + 3) |c_i|_2 + 2).

The projection is nonexpansive in the 2-norm and so is a -> a - inv_L (a M - q) for inv_L <= 1 / lambda_max(M): the error of
iteration t passes through the later ones without growing and the bound after T iterations is T delta_i.  The restatement
rounds M to float32 as the kernel does, so that rounding is no part of the error.

Every test prints its worst error-to-bound ratio (docs/EXPERIMENTS.md records them).
"""

import numpy as np
import pytest

import aa_reference as ar
import simplex_plan as sp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
M_LIST = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 16383, 16384]
R_LIST = [1, 2, 63, 65, 300]
R_MAX = max(R_LIST)


def boundary_lengths():
    try:
        b = sp.tier_boundary()
    except BaseException:        # (no host compiler: the documented boundary)
        b = 1024
    return [b, b + 1]


def designed_rows(m, r=R_MAX, seed=0):
    """r float32 rows of m entries, eight kinds in turn: Gaussian, wide Gaussian, a ramp (the active set shrinks over many
    rounds), ten decades of spread with both signs, all negative, one dominant entry, a point near the simplex, and nearly
    equal entries (every entry stays active)"""
    rs = np.random.RandomState(100 * m + seed)
    U = np.empty((r, m))
    for i in range(r):
        kind = i % 8
        if kind == 0:
            U[i] = rs.standard_normal(m)
        elif kind == 1:
            U[i] = 10.0 * rs.standard_normal(m)
        elif kind == 2:
            U[i] = np.linspace(-1.0, 1.0 + rs.random_sample(), m)[rs.permutation(m)] if m > 1 else rs.standard_normal(1)
        elif kind == 3:
            U[i] = 10.0 ** rs.uniform(-5, 5, m) * rs.choice([-1.0, 1.0], m)
        elif kind == 4:
            U[i] = -1.0 - 5.0 * rs.random_sample(m)
        elif kind == 5:
            U[i] = rs.standard_normal(m)
            U[i, rs.randint(m)] += 60.0
        elif kind == 6:
            U[i] = rs.dirichlet(np.ones(m)) + 1e-3 * rs.standard_normal(m)
        else:
            U[i] = 1.0 / m + 1e-3 / m * rs.standard_normal(m)
    return U.astype(np.float32)


def run_rows(ctx, V, G=None, step=0.0, **kw):
    from xeofs_amd import engine

    return engine.simplex_rows(ctx, V, G, step, **kw).cpu().numpy()


def check_rows(out, u32, bound_factor=1.0):
    """the four assertions of the module docstring on out against the float64 projection of u32; -> the worst ratios"""
    u = u32.astype(np.float64)
    ref, tau = ar.project_sort(u)
    scale = np.maximum(1.0, np.abs(u).max(axis=1))
    b = bound_factor * 2.0 * EPS * scale
    assert out.dtype == np.float32 and out.shape == u.shape and np.all(out >= 0.0)
    S = ar.active_count(u, tau)
    sums = np.abs(out.astype(np.float64).sum(axis=1) - 1.0)
    assert np.all(sums <= (S + 2) * EPS), (sums / ((S + 2) * EPS)).max()
    err = np.abs(out - ref)
    assert np.all(err <= b[:, None]), (err / b[:, None]).max()
    clear = np.abs(u - tau[:, None]) > b[:, None]
    assert np.array_equal((out > 0.0)[clear], (ref > 0.0)[clear])
    return float((err / b[:, None]).max()), float((sums / ((S + 2) * EPS)).max())


# ------------------------------------------------------------------------------------------------ simplex_rows: the shapes
@pytest.mark.parametrize("m", M_LIST + ["boundary", "boundary+1"])
def test_rows_against_float64_at_every_edge(ctx, m):
    if isinstance(m, str):
        m = boundary_lengths()[m.endswith("+1")]
    U = designed_rows(m)
    worst = (0.0, 0.0)
    for r in R_LIST:
        out = run_rows(ctx, U[:r])
        worst = tuple(max(a, b) for a, b in zip(worst, check_rows(out, U[:r])))
        if r == 65:
            assert np.array_equal(out, run_rows(ctx, U[:r]))          # a rerun, bit for bit
            assert np.array_equal(out[:63], run_rows(ctx, U[:63]))    # a row's result does not depend on its neighbours
        # one dominant entry: exactly one-hot
        dom = np.arange(r) % 8 == 5
        if m > 1 and dom.any():
            assert np.all(np.sort(out[dom], axis=1)[:, -1] == 1.0) and np.all(np.sort(out[dom], axis=1)[:, :-1] == 0.0)
    print(f"simplex_rows m={m}: worst |out - ref| / bound = {worst[0]:.3f}, worst |sum - 1| / bound = {worst[1]:.3f}")
    assert worst[0] < 1.0 and worst[1] < 1.0


def test_m_equal_one_gives_one(ctx):
    V = np.array([[0.0], [1.0], [-7.5], [3e-30], [1e20], [-1e30]], dtype=np.float32)
    assert np.array_equal(run_rows(ctx, V), np.ones((6, 1), np.float32))


# ------------------------------------------------------------------------------------------------ simplex_rows: exact cases
@pytest.mark.parametrize("m", [1, 2, 3, 33, 64, 65, 257, 1024, 1025, 5000, 16384])
def test_exact_cases_bit_for_bit(ctx, m):
    rs = np.random.RandomState(m)
    rows, want = [], []
    # rows already on the simplex: integer counts over 2^12 that sum to 2^12 (tau = 0 exactly)
    for conc in (0.05, 1.0):
        c = rs.multinomial(4096, rs.dirichlet(conc * np.ones(m))).astype(np.float64) / 4096.0
        rows.append(c), want.append(c)
    # one-hot rows
    for j in {0, m // 2, m - 1}:
        e = np.zeros(m)
        e[j] = 1.0
        rows.append(e), want.append(e)
    # equal entries: out = c - (m c - 1) / m, every step of it exact or rounded as float64 rounds it
    for c in (0.25, -3.0, 1.5, 0.0):
        rows.append(np.full(m, c)), want.append(np.full(m, np.float64(c) - (m * np.float64(c) - 1.0) / m))
    # dyadic values with a dyadic tau: a dyadic point x of the simplex on a support of s = 2^q entries, u = x + tau there,
    # u = tau - (a dyadic amount >= 0, some of them 0) elsewhere
    for tau in (0.375, -2.5, 16.0):
        s = 1 << rs.randint(0, min(int(np.log2(m)), 9) + 1)                # (at most 512: x is in units of 2^-10)
        x = np.zeros(m)
        supp = rs.permutation(m)[:s]
        x[supp] = (rs.multinomial(1024 - s, np.ones(s) / s) + 1) / 1024.0
        u = np.where(x > 0, x + tau, tau - rs.randint(0, 4, m) / 8.0)
        rows.append(u), want.append(x)
    V = np.stack(rows).astype(np.float32)
    assert np.array_equal(V.astype(np.float64), np.stack(rows))            # (the designed rows are float32 values)
    out = run_rows(ctx, V)
    assert np.array_equal(out, np.stack(want).astype(np.float32))


# ------------------------------------------------------------------------------------------------ simplex_rows: G, aliasing, strides
@pytest.mark.parametrize("m", [5, 64, 300, 1024, 1025, 4097])
def test_gradient_step_null_gradient_and_aliased_out(ctx, m):
    import torch

    from xeofs_amd import engine

    r = 37
    V = designed_rows(m, r, seed=1)
    G = designed_rows(m, r, seed=2)[::-1].copy()
    base = run_rows(ctx, V)
    assert np.array_equal(run_rows(ctx, V, None), base)
    assert np.array_equal(run_rows(ctx, V, G, 0.0), base)                  # step 0 leaves V's projection
    worst = 0.0
    for step in (0.25, 2.0 ** -20, 8.0):                                   # a power of two: fmaf(-step, G, V) is one float32 addition
        u = V + (-np.float32(step) * G)
        assert u.dtype == np.float32
        ok = np.isfinite(u).all(axis=1)
        out = run_rows(ctx, V, G, step)
        worst = max(worst, check_rows(out[ok], u[ok])[0])
    # out aliases V: the same bits
    Vd = torch.from_numpy(V).cuda()
    Gd = torch.from_numpy(G).cuda()
    want = engine.simplex_rows(ctx, Vd.clone(), Gd, 0.25).cpu().numpy()
    got = engine.simplex_rows(ctx, Vd, Gd, 0.25, out=Vd)
    assert got.data_ptr() == Vd.data_ptr() and np.array_equal(Vd.cpu().numpy(), want)
    print(f"simplex_rows with G, m={m}: worst |out - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("m", [7, 300, 2049])
def test_general_step(ctx, m):
    V = designed_rows(m, 40, seed=3)
    G = designed_rows(m, 40, seed=4)
    step = np.float32(0.3)
    u = (V.astype(np.float64) - np.float64(step) * G.astype(np.float64)).astype(np.float32)
    ratio = check_rows(run_rows(ctx, V, G, float(step)), u, bound_factor=2.0)[0]
    print(f"simplex_rows with a general step, m={m}: worst |out - ref| / (2^-22 max(1, max|u|)) = {ratio:.3f}")


@pytest.mark.parametrize("m", [3, 64, 65, 1024, 1025, 16384])
def test_strided_operands_with_decoys_and_canaries(ctx, m):
    import torch

    from xeofs_amd import engine

    r, pad_c, pad_r = 9, 5, 2
    V = designed_rows(m, r, seed=5)
    G = designed_rows(m, r, seed=6)

    def big(fill, src=None):
        t = torch.full((r + pad_r, m + pad_c), fill, dtype=torch.float32, device="cuda")
        if src is not None:
            t[:r, :m] = torch.from_numpy(src).cuda()
        return t

    Vb, Gb, Ob = big(float("nan"), V), big(float("inf"), G), big(-777.0)      # decoys past m and past r; canaries in out
    want = run_rows(ctx, V, G, 0.5)
    got = engine.simplex_rows(ctx, Vb[:r, :m], Gb[:r, :m], 0.5, out=Ob[:r, :m])
    assert got.data_ptr() == Ob.data_ptr()
    O = Ob.cpu().numpy()
    assert np.array_equal(O[:r, :m], want) and np.all(O[r:] == -777.0) and np.all(O[:, m:] == -777.0)
    Vn = Vb.cpu().numpy()
    assert np.array_equal(Vn[:r, :m], V) and np.isnan(Vn[r:]).all() and np.isnan(Vn[:, m:]).all()


@pytest.mark.parametrize("m", [1, 4, 64, 100, 1024, 1025, 9000])
def test_a_nan_row_and_an_infinite_row_come_back_nan_and_change_nothing_else(ctx, m):
    r = 70
    V = designed_rows(m, r, seed=7)
    clean = run_rows(ctx, V)
    bad = {3: np.nan, 20: np.inf, 41: -np.inf, 69: np.nan}
    W = V.copy()
    for i, v in bad.items():
        W[i, (7 * i) % m] = v
    out = run_rows(ctx, W)
    for i in range(r):
        if i in bad:
            assert np.isnan(out[i]).all()
        else:
            assert np.array_equal(out[i], clean[i])
    # an overflow of the step itself is an infinity of u
    G = np.zeros_like(V)
    G[5, 0] = 3e38
    out = run_rows(ctx, V, G, 16.0)
    assert np.isnan(out[5]).all() and np.array_equal(np.delete(out, 5, 0), np.delete(clean, 5, 0))


def test_refusals_and_no_ops(ctx):
    import torch

    from xeofs_amd import engine

    assert tuple(engine.simplex_rows(ctx, np.zeros((0, 5), np.float32)).shape) == (0, 5)
    with pytest.raises(ValueError, match="16384"):
        engine.simplex_rows(ctx, np.zeros((1, 16385), np.float32))
    with pytest.raises(ValueError, match="at least one entry"):
        engine.simplex_rows(ctx, np.zeros((3, 0), np.float32))
    with pytest.raises(ValueError, match="shape of V"):
        engine.simplex_rows(ctx, np.zeros((3, 4), np.float32), np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="out must be"):
        engine.simplex_rows(ctx, np.zeros((3, 4), np.float32), out=torch.zeros((3, 5), device="cuda"))
    # the entry itself: strides below m, m < 1
    lib, h = ctx.lib, ctx.handle
    t = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    import ctypes as C

    vp = C.c_void_p
    assert lib.eofx_simplex_rows_f32(h, vp(p), 4, 8, 7, None, 0, 0.0, vp(p), 8) == -1
    assert lib.eofx_simplex_rows_f32(h, vp(p), 4, 8, 8, None, 0, 0.0, vp(p), 7) == -1
    assert lib.eofx_simplex_rows_f32(h, vp(p), 4, 8, 8, vp(p), 7, 0.0, vp(p), 8) == -1
    assert lib.eofx_simplex_rows_f32(h, vp(p), 4, 0, 8, None, 0, 0.0, vp(p), 8) == -1
    assert lib.eofx_simplex_rows_f32(h, vp(p), -1, 8, 8, None, 0, 0.0, vp(p), 8) == -1
    assert lib.eofx_simplex_rows_f32(h, vp(p), 1, 16385, 16385, None, 0, 0.0, vp(p), 16385) == -8
    assert lib.eofx_simplex_rows_f32(h, vp(p), 0, 8, 8, None, 0, 0.0, vp(p), 8) == 0
    assert lib.eofx_simplex_pg_f32(h, vp(p), 8, vp(p), 8, vp(p), 1.0, 1, 4, 33, vp(p), 8) == -8
    assert lib.eofx_simplex_pg_f32(h, vp(p), 8, vp(p), 8, vp(p), 1.0, 0, 4, 8, vp(p), 8) == -1
    assert lib.eofx_simplex_pg_f32(h, vp(p), 7, vp(p), 8, vp(p), 1.0, 1, 4, 8, vp(p), 8) == -1
    assert lib.eofx_simplex_pg_f32(h, vp(p), 8, vp(p), 8, vp(p), 1.0, 1, 4, 0, vp(p), 8) == -1
    assert lib.eofx_simplex_pg_f32(h, vp(p), 8, vp(p), 8, vp(p), 1.0, 1, 0, 8, vp(p), 8) == 0
    with pytest.raises(ValueError, match="32"):
        engine.simplex_pg(ctx, np.zeros((4, 33), np.float32), np.zeros((4, 33), np.float32), np.eye(33), 1.0, 1)
    with pytest.raises(ValueError, match="shape of A"):
        engine.simplex_pg(ctx, np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32), np.eye(3), 1.0, 1)
    with pytest.raises(ValueError, match="M must be"):
        engine.simplex_pg(ctx, np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.eye(2), 1.0, 1)
    assert tuple(engine.simplex_pg(ctx, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.eye(3), 1.0, 1).shape) == (0, 3)


# ------------------------------------------------------------------------------------------------ simplex_pg
N_LIST = [1, 63, 64, 65, 257, 1000]
N_MAX = max(N_LIST)


def pg_problem(k, seed=0):
    """N_MAX least-squares problems |x_i - a Z|^2 over the simplex: (A0, Q, M, inv_L) with float32 A0 and Q, float64 M"""
    rs = np.random.RandomState(1000 * k + seed)
    d = 3 * k + 5
    Z = rs.standard_normal((k, d))
    X = rs.dirichlet(0.5 * np.ones(k), N_MAX) @ Z + 0.5 * rs.standard_normal((N_MAX, d))
    Q = (X @ Z.T).astype(np.float32)
    M = Z @ Z.T
    A0 = rs.dirichlet(np.ones(k), N_MAX).astype(np.float32)
    inv_L = np.float32(0.99 / ar.lambda_max(M.astype(np.float32).astype(np.float64)))
    return A0, Q, M, inv_L


@pytest.mark.parametrize("k", [1, 2, 3, 8, 31, 32])
def test_pg_against_float64_within_the_composed_bound(ctx, k):
    from xeofs_amd import engine

    A0, Q, M, inv_L = pg_problem(k)
    M32 = M.astype(np.float32).astype(np.float64)
    c = float(inv_L) * (np.abs(M32).max(axis=0)[None, :] + np.abs(Q.astype(np.float64)))
    delta = EPS * ((k + 3) * np.sqrt((c * c).sum(axis=1)) + 2.0)
    worst = 0.0
    for iters in (1, 10, 50):
        ref = ar.pg_steps(A0, Q, M, inv_L, iters)
        full = None
        for n in N_LIST:
            out = engine.simplex_pg(ctx, A0[:n], Q[:n], M, inv_L, iters).cpu().numpy()
            assert out.dtype == np.float32 and out.shape == (n, k) and np.all(out >= 0.0)
            assert np.all(np.abs(out.astype(np.float64).sum(axis=1) - 1.0) <= (k + 2) * EPS)
            err = np.sqrt(((out - ref[:n]) ** 2).sum(axis=1))
            ratio = float((err / (iters * delta[:n])).max())
            assert ratio <= 1.0, (k, n, iters, ratio)
            worst = max(worst, ratio)
            if n == N_MAX:
                full = out
            if k == 1:
                assert np.all(out == 1.0)
        for n in N_LIST:                                          # a row's result does not depend on the rows beside it
            assert np.array_equal(engine.simplex_pg(ctx, A0[:n], Q[:n], M, inv_L, iters).cpu().numpy(), full[:n])
    print(f"simplex_pg k={k}: worst row error / (T delta) = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("k", [2, 5, 32])
def test_pg_identity_reaches_the_one_hot_in_one_step_exactly(ctx, k):
    from xeofs_amd import engine

    rs = np.random.RandomState(k)
    n = 130
    A0 = (rs.multinomial(64, np.ones(k) / k, n) / 64.0).astype(np.float32)          # dyadic points of the simplex
    hot = rs.randint(0, k, n)
    Q = np.zeros((n, k), np.float32)
    Q[np.arange(n), hot] = 1.0
    for iters in (1, 7):
        out = engine.simplex_pg(ctx, A0, Q, np.eye(k), 1.0, iters).cpu().numpy()
        assert np.array_equal(out, Q)


@pytest.mark.parametrize("k", [3, 32])
def test_pg_host_and_device_m_strides_aliasing_and_isolation(ctx, k):
    import torch

    from xeofs_amd import engine

    A0, Q, M, inv_L = pg_problem(k, seed=1)
    n = 300
    A0, Q = A0[:n], Q[:n]
    want = engine.simplex_pg(ctx, A0, Q, M, inv_L, 10).cpu().numpy()
    assert np.array_equal(engine.simplex_pg(ctx, A0, Q, torch.from_numpy(M).cuda(), inv_L, 10).cpu().numpy(), want)   # M on the device
    assert np.array_equal(engine.simplex_pg(ctx, A0, Q, M, inv_L, 10).cpu().numpy(), want)                              # a rerun
    # strided operands with decoys, canaries in out, and out aliasing A
    Ab = torch.full((n + 2, k + 3), float("nan"), device="cuda")
    Qb = torch.full((n + 2, k + 1), float("inf"), device="cuda")
    Ob = torch.full((n + 2, k + 2), -777.0, device="cuda")
    Ab[:n, :k], Qb[:n, :k] = torch.from_numpy(A0).cuda(), torch.from_numpy(Q).cuda()
    engine.simplex_pg(ctx, Ab[:n, :k], Qb[:n, :k], M, inv_L, 10, out=Ob[:n, :k])
    O = Ob.cpu().numpy()
    assert np.array_equal(O[:n, :k], want) and np.all(O[n:] == -777.0) and np.all(O[:, k:] == -777.0)
    engine.simplex_pg(ctx, Ab[:n, :k], Qb[:n, :k], M, inv_L, 10, out=Ab[:n, :k])
    An = Ab.cpu().numpy()
    assert np.array_equal(An[:n, :k], want) and np.isnan(An[n:]).all() and np.isnan(An[:, k:]).all()
    # a NaN in A, an infinity in Q: those rows come back NaN, no other row changes
    A1, Q1 = A0.copy(), Q.copy()
    A1[17, k - 1] = np.nan
    Q1[200, 0] = np.inf
    out = engine.simplex_pg(ctx, A1, Q1, M, inv_L, 10).cpu().numpy()
    assert np.isnan(out[17]).all() and np.isnan(out[200]).all()
    keep = np.setdiff1d(np.arange(n), [17, 200])
    assert np.array_equal(out[keep], want[keep])
