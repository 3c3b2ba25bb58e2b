"""GPU tests of the FastICA solver (engine.fastica; csrc/eofx_ica.hpp) against the float64 restatement (tests/ica_reference.py)
on the same float32 operands.

    exact        fun = cube on integer panels (|z| <= 3, W in {-1, 0, 1} with at most 6 entries a row, so that |s| <= 18 and
                 s^3, 3 s^2, s^4 / 4 are integers or quarters below 2^24; n a power of two): every product and sum is exact and W1
                 and gmean equal numpy's bit for bit
    moments      per element of W1 within ica_reference.moment_bound: the float32 chain's (q + 1) 2^-24 sum |w||z| through the
                 Lipschitz constants of g and g', plus the error of the device's g and g' themselves (EPS_G, measured by the
                 sweep below through the operator, doubled), plus n 2^-53 of the float64 sums
    decorrelate  W against the polar factor U V^T of numpy's SVD of the DEVICE's W1: at most 32 times the error of numpy's own
                 eigh route against that factor, floor q 2^-52;  || W W^T - I ||_F <= 64 q 2^-52 (the rotations a column takes in
                 the Jacobi sweeps, each with one rounding)
    trajectory   every W_t of the float64 reference as one restart of one max_iter = 1 call: W1 within the moment bound, W within
                 the perturbation bound of the polar factor 2 ||dW1||_F / (sigma_min(W1) + sigma_min(W1 + dW1))
    whole runs   the iteration count of the reference (cases conditioned on the CPU), the final W within 16 times the deviation
                 of the reference's own float32 emulation from its float64 run (floor 1e-6)
Every test prints its worst error-to-bound ratio.  No test here tries to make the kernel fault or hang."""

import numpy as np
import pytest

import ica_reference as kr

pytestmark = pytest.mark.gpu

EPS53, EPS52 = 2.0 ** -53, 2.0 ** -52


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


GUARD = 16                                   # words on either side of every buffer the operator reads or writes


class State:
    """the device state of a call: W, status, iters and all four outputs, as torch tensors -- each carved out of a larger
    buffer with GUARD canary words on both sides, which host() checks: a write before or after a buffer is seen"""

    def __init__(self, ctx, W, status=None, iters=None):
        import torch

        self.dev = f"cuda:{ctx.device}"
        W = np.ascontiguousarray(W, dtype=np.float64)
        R, q = W.shape[0], W.shape[1]
        self.bufs = {}

        def carve(name, host, canary):
            t = torch.full((host.size + 2 * GUARD,), canary, dtype=getattr(torch, str(host.dtype)), device=self.dev)
            view = t[GUARD:GUARD + host.size].view(host.shape)
            view.copy_(torch.from_numpy(host.copy()).to(self.dev))
            self.bufs[name] = (t, canary)
            assert view.is_contiguous() and view.data_ptr() == t.data_ptr() + GUARD * t.element_size()
            return view

        self.W = carve("W", W, -9.0)
        self.status = carve("status", np.zeros(R, np.int32) if status is None else np.asarray(status, np.int32), -9)
        self.iters = carve("iters", np.zeros(R, np.int32) if iters is None else np.asarray(iters, np.int32), -9)
        self.out = dict(W1=carve("W1", np.full((R, q, q), -7.0), -9.0), gmean=carve("gmean", np.full((R, q), -7.0), -9.0),
                        lim=carve("lim", np.full((R,), -7.0), -9.0), nused=carve("nused", np.full((1,), -7, np.int64), -9))

    def host(self):
        for name, (t, canary) in self.bufs.items():
            h = t.cpu().numpy()
            assert (h[:GUARD] == canary).all() and (h[-GUARD:] == canary).all(), f"a canary around {name} was overwritten"
        res = {k: v.cpu().numpy() for k, v in self.out.items()}
        res.update(W=self.W.cpu().numpy(), status=self.status.cpu().numpy(), iters=self.iters.cpu().numpy())
        return res


def call(ctx, Z, W, T, fun="logcosh", alpha=1.0, tol=1e-4, status=None, iters=None):
    """one engine.fastica call from a fresh state -> a dict of host arrays"""
    from xeofs_amd import engine

    st = State(ctx, W, status, iters)
    engine.fastica(ctx, Z, st.W, st.status, st.iters, fun=fun, alpha=alpha, tol=tol, max_iter=T, out=st.out)
    ctx.synchronize()
    return st.host()


def padded(ctx, Z, extra=3):
    """Z as a device view with row stride q + extra and NaN in the columns past q"""
    import torch

    n, q = Z.shape
    buf = torch.full((n, q + extra), float("nan"), dtype=torch.float32, device=f"cuda:{ctx.device}")
    buf[:, :q] = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float32)).to(buf.device)
    return buf[:, :q]


# ------------------------------------------------------------------------------------------------ exact fields
def integer_case(rs, n, q, R):
    Z = rs.randint(-3, 4, size=(n, q)).astype(np.float32)
    W = np.zeros((R, q, q))
    for r in range(R):
        for j in range(q):
            idx = rs.choice(q, size=min(q, 6), replace=False)
            W[r, j, idx] = rs.randint(-1, 2, size=idx.size)
    return Z, W


def assert_exact(res, Z, W, what):
    """bit for bit, the sign of a zero apart (numpy's own products may give -0 where every term is -0)"""
    for r in range(W.shape[0]):
        W1, gmean, nused = kr.moments(Z, W[r], "cube")
        assert np.array_equal(bits(res["W1"][r] + 0.0), bits(W1 + 0.0)), f"{what}: W1 of restart {r}"
        assert np.array_equal(bits(res["gmean"][r] + 0.0), bits(gmean + 0.0)), f"{what}: gmean of restart {r}"
        assert int(res["nused"][0]) == nused
    assert np.array_equal(bits(res["W"]), bits(W)), f"{what}: max_iter = 0 moved W"
    assert (res["status"] == 0).all() and (res["iters"] == 0).all() and (res["lim"] == -7.0).all()


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32])
def test_exact_integer_panels(ctx, q):
    rs = np.random.RandomState(100 + q)
    for n in (1, 64, 256, 512, 1024):
        for R in (1, 2, 7):
            Z, W = integer_case(rs, n, q, R)
            res = call(ctx, padded(ctx, Z), W, 0, fun="cube")
            assert_exact(res, Z, W, f"q = {q}, n = {n}, R = {R}")


def test_exact_beyond_one_slab(ctx):
    """n = 2^18 = 2 x 256 x ICA_BMAX rows: a block holds 512 rows"""
    from xeofs_amd import engine

    rs = np.random.RandomState(7)
    n = 262144
    assert n > 256 * 512
    Z, W = integer_case(rs, n, 4, 2)
    res = call(ctx, padded(ctx, Z, 1), W, 0, fun="cube")
    assert_exact(res, Z, W, "n = 2^18")
    assert engine.ICA_NMAX >= n


# ------------------------------------------------------------------------------------------------ the contrast's own error
def sweep_values():
    v = np.linspace(-16.0, 16.0, 2 ** 16).astype(np.float32)
    ends = np.array([0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-38, 1e-30, -1e-30, 1e-10, 20.0, -20.0, 50.0, 88.0, -88.0, 100.0, 1e3,
                     -1e3, 1e4, 1e9, -1e9, 1e18, -1e18, 1e30, -1e30], dtype=np.float32)
    return v, ends


def sweep(ctx, s, fun, alpha):
    """g, g', G of the device at the float32 values s through the operator: q = 2, n = 1, Z = [[1, 0]], W_r = [[s, 1], [s', 1]]"""
    s = np.asarray(s, dtype=np.float32)
    pad = (-s.size) % 2
    s2 = np.concatenate([s, np.zeros(pad, np.float32)]).reshape(-1, 2)
    Z = np.array([[1.0, 0.0]], dtype=np.float32)
    g, gp, G = [], [], []
    for r0 in range(0, s2.shape[0], 1024):
        blk = s2[r0:r0 + 1024].astype(np.float64)
        W = np.ones((blk.shape[0], 2, 2))
        W[:, :, 0] = blk
        res = call(ctx, Z, W, 0, fun=fun, alpha=alpha)
        d = -res["W1"][:, :, 1]
        gp.append(d.reshape(-1))
        g.append((res["W1"][:, :, 0] + d * blk).reshape(-1))
        G.append(res["gmean"].reshape(-1))
    cut = lambda x: np.concatenate(x)[:s.size]
    return cut(g), cut(gp), cut(G)


@pytest.mark.parametrize("fun,alpha", [("logcosh", 1.0), ("logcosh", 1.5), ("logcosh", 2.0), ("exp", 1.0), ("cube", 1.0)])
def test_contrast_error_sweep(ctx, fun, alpha):
    v, ends = sweep_values()
    s = v if fun == "cube" else np.concatenate([v, ends])
    g, gp, G = sweep(ctx, s, fun, alpha)
    s64 = s.astype(np.float64)
    rg, rgp, rG = kr.contrast(s64, fun, alpha)
    with np.errstate(invalid="ignore", over="ignore"):
        big = np.abs(s64) > 1e8                     # (g = W1_j1 + g' s loses g' s there; g' is 0 and g is read directly)
        assert np.isfinite(g).all() and np.isfinite(gp).all() and np.isfinite(G).all()
        if fun == "cube":
            eg, egp, eG = np.abs(g - rg) / np.maximum(np.abs(rg), 1e-300), np.abs(gp - rgp) / np.maximum(np.abs(rgp), 1e-300), \
                np.abs(G - rG) / np.maximum(np.abs(rG), 1e-300)
            eg[rg == 0], egp[rgp == 0], eG[rG == 0] = np.abs(g[rg == 0]), np.abs(gp[rgp == 0]), np.abs(G[rG == 0])
            lim = (kr.CUBE_REL,) * 3
        else:
            eg, egp, eG = np.abs(g - rg), np.abs(gp - rgp), np.abs(G - rG) / (1.0 + np.abs(rG))
            lim = kr.EPS_G[fun]
    print(f"{fun} alpha = {alpha}: max err g = {eg.max():.4g} (at s = {s[eg.argmax()]:.6g}), g' = {egp.max():.4g} "
          f"(at s = {s[egp.argmax()]:.6g}), G = {eG.max():.4g} (at s = {s[eG.argmax()]:.6g}); bounds {lim}; big = {int(big.sum())}")
    assert eg.max() <= lim[0] and egp.max() <= lim[1] and eG.max() <= lim[2]


# ------------------------------------------------------------------------------------------------ the moments on general data
def panels(n, q, seed):
    rs = np.random.RandomState(seed)
    return dict(gauss=rs.standard_normal((n, q)).astype(np.float32), heavy=rs.standard_t(3, size=(n, q)).astype(np.float32)), rs


def check_moments(res_r, Z, W, fun, alpha, what):
    """W1 and gmean of one restart against float64 within the bounds -> the worst ratios"""
    W1, gmean, nused = kr.moments(Z, W, fun, alpha)
    Zf = np.asarray(Z, np.float64)[kr.finite_rows(Z)]
    n = max(nused, 1)
    g, gp, G = kr.contrast(Zf @ W.T, fun, alpha)
    b1 = kr.moment_bound(Z, W, fun, alpha) + 2 * n * EPS53 * ((np.abs(g).T @ np.abs(Zf)) / n + (np.abs(gp).sum(axis=0) / n)[:, None] * np.abs(W))
    e1 = np.abs(res_r["W1"] - W1)
    assert (e1 <= b1).all(), f"{what}: W1 off by {np.max(e1 / b1):.3g} of its bound"
    b2 = kr.gmean_bound(Z, W, fun, alpha) + 2 * n * EPS53 * np.abs(G).sum(axis=0) / n
    e2 = np.abs(res_r["gmean"] - gmean)
    assert (e2 <= b2).all(), f"{what}: gmean off by {np.max(e2 / b2):.3g} of its bound"
    return float(np.max(e1 / b1)), float(np.max(e2 / b2))


@pytest.mark.parametrize("n,q", [(1500, 5), (777, 32), (4097, 17)])
@pytest.mark.parametrize("fun,alpha", [("logcosh", 1.0), ("logcosh", 2.0), ("exp", 1.0), ("cube", 1.0)])
def test_moments_general(ctx, n, q, fun, alpha):
    data, rs = panels(n, q, 11 * n + q)
    W = np.stack([kr.random_orthogonal(q, rs) for _ in range(2)])
    for name, Z in data.items():
        res = call(ctx, padded(ctx, Z), W, 0, fun=fun, alpha=alpha)
        assert int(res["nused"][0]) == n
        for r in range(2):
            r1, r2 = check_moments({k: res[k][r] for k in ("W1", "gmean")}, Z, W[r], fun, alpha, f"{name} {fun} n = {n} q = {q}")
            print(f"{name} {fun} alpha = {alpha} n = {n} q = {q} restart {r}: W1 at {r1:.3g}, gmean at {r2:.3g} of the bound")


# ------------------------------------------------------------------------------------------------ the decorrelation
def with_singular_values(q, sv, rs):
    return (kr.random_orthogonal(q, rs) * sv) @ kr.random_orthogonal(q, rs)


@pytest.mark.parametrize("q,cond", [(1, 1.0), (2, 2.0), (7, 2.0), (7, 1e4), (32, 2.0), (32, 1e4), (31, 1e4)])
def test_decorrelation(ctx, q, cond):
    """all-zero Z and logcosh give W1 = -alpha W for ANY W on entry: the entry's W sets the condition of W1"""
    rs = np.random.RandomState(1000 + q)
    sv = np.logspace(0.0, -np.log10(cond), q) if q > 1 else np.array([0.7])
    Win = np.stack([with_singular_values(q, sv, rs) for _ in range(3)])
    res = call(ctx, np.zeros((5, q), np.float32), Win, 1, fun="logcosh", alpha=1.0)
    assert np.array_equal(res["W1"], -Win) and (res["iters"] == 1).all() and (res["status"] != 2).all()
    for r in range(3):
        P = kr.polar(res["W1"][r])
        e_dev = np.linalg.norm(res["W"][r] - P)
        e_eigh = np.linalg.norm(kr.sym_decorrelation(res["W1"][r]) - P)
        bound = 32.0 * max(e_eigh, q * EPS52)
        orth = np.linalg.norm(res["W"][r] @ res["W"][r].T - np.eye(q))
        print(f"q = {q} cond = {cond:g}: device {e_dev:.3g}, eigh route {e_eigh:.3g}, orthogonality {orth:.3g}")
        assert e_dev <= bound, f"the polar factor is off by {e_dev / bound:.3g} of its bound"
        assert orth <= 64 * q * EPS52
        lim = np.max(np.abs(np.abs(np.einsum("ij,ij->i", res["W"][r], Win[r])) - 1.0))
        assert abs(res["lim"][r] - lim) <= 8 * q * EPS52 * (1.0 + lim)


# ------------------------------------------------------------------------------------------------ along a trajectory
@pytest.mark.parametrize("case", kr.RUN_CASES, ids=lambda c: f"{c[0]}-{c[1]}-q{c[4]}")
def test_trajectory_steps(ctx, case):
    fun, alpha, seed, n, q, tol = case
    Z, W0 = kr.mixed_panel(seed, n, q)
    ref = kr.run(Z, W0, fun, alpha, tol, 200)
    path = np.stack(ref["path"])
    res = call(ctx, Z, path, 1, fun=fun, alpha=alpha, tol=tol)
    worst = [0.0, 0.0]
    for t, Wt in enumerate(path):
        st = kr.step(Z, Wt, fun, alpha)
        r1, _ = check_moments({k: res[k][t] for k in ("W1", "gmean")}, Z, Wt, fun, alpha, f"{fun} step {t}")
        dW1 = kr.moment_bound(Z, Wt, fun, alpha)
        bound = kr.polar_bound(st["W1"], dW1) + 32 * q * EPS52
        err = np.linalg.norm(res["W"][t] - st["W"])
        assert err <= bound, f"{fun} step {t}: W off by {err / bound:.3g} of the polar factor's perturbation bound"
        worst = [max(worst[0], r1), max(worst[1], err / bound)]
        assert abs(res["lim"][t] - st["lim"]) <= 2 * bound
    assert (res["iters"] == 1).all()
    print(f"{fun} alpha = {alpha}: {len(path)} steps, W1 at {worst[0]:.3g}, W at {worst[1]:.3g} of the bounds")


# ------------------------------------------------------------------------------------------------ whole runs
def solve(ctx, Z, W0, fun, alpha, tol, max_iter, chunk):
    from xeofs_amd import engine

    st = State(ctx, W0)
    done = 0
    while done < max_iter:
        T = min(chunk, max_iter - done)
        engine.fastica(ctx, Z, st.W, st.status, st.iters, fun=fun, alpha=alpha, tol=tol, max_iter=T, out=st.out)
        done += T
        if bool((st.status != 0).all()):
            break
    ctx.synchronize()
    return st.host()


@pytest.mark.parametrize("case", kr.RUN_CASES, ids=lambda c: f"{c[0]}-{c[1]}-q{c[4]}")
def test_whole_runs(ctx, case):
    fun, alpha, seed, n, q, tol = case
    Z, W0 = kr.mixed_panel(seed, n, q)
    ref = kr.run(Z, W0, fun, alpha, tol, 200)
    emu = kr.run(Z, W0, fun, alpha, tol, 200, f32=True)
    res = solve(ctx, Z, W0[None], fun, alpha, tol, 200, 64)
    assert res["status"][0] == 1 and ref["status"] == 1
    assert res["iters"][0] == ref["iters"], f"{res['iters'][0]} iterations, the reference takes {ref['iters']}"
    dev = np.abs(res["W"][0] - ref["W"]).max()
    own = np.abs(emu["W"] - ref["W"]).max()
    bound = max(16.0 * own, 1e-6)
    print(f"{fun} alpha = {alpha} q = {q}: {ref['iters']} iterations; device - float64 = {dev:.3g}, emulation - float64 = {own:.3g}, "
          f"ratio {dev / max(own, 1e-300):.3g}")
    assert dev <= bound
    st = kr.step(Z, res["W"][0], fun, alpha)
    eta = kr.polar_bound(st["W1"], kr.moment_bound(Z, res["W"][0], fun, alpha))
    assert st["lim"] <= tol + 2 * eta


# ------------------------------------------------------------------------------------------------ the rules
def mixed_state(q=5, n=700, R=7, seed=3):
    Z, _ = kr.mixed_panel(seed, n, q)
    rs = np.random.RandomState(seed)
    return Z, np.stack([kr.random_orthogonal(q, rs) for _ in range(R)])


KEYS = ("W", "W1", "gmean", "lim", "nused", "status", "iters")


def same(a, b, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("fun", kr.FUNS)
def test_reruns_chains_and_company(ctx, fun):
    Z, W = mixed_state()
    a = call(ctx, Z, W, 8, fun=fun, tol=1e-6)
    same(a, call(ctx, Z, W, 8, fun=fun, tol=1e-6), "a rerun")
    # T calls of 1 against one call of T
    st = State(ctx, W)
    from xeofs_amd import engine

    for _ in range(8):
        engine.fastica(ctx, Z, st.W, st.status, st.iters, fun=fun, tol=1e-6, max_iter=1, out=st.out)
    ctx.synchronize()
    same(a, st.host(), "eight calls of one iteration")
    assert (a["iters"] >= 1).all() and (a["iters"] <= 8).all() and (a["status"] != 2).all()
    print(f"{fun}: iterations {a['iters'].tolist()}, status {a['status'].tolist()}")
    # a restart alone against the same restart among seven
    for r in (0, 3, 6):
        alone = call(ctx, Z, W[r:r + 1], 8, fun=fun, tol=1e-6)
        for k in ("W", "W1", "gmean", "lim", "status", "iters"):
            assert np.array_equal(bits(alone[k][0]), bits(a[k][r])), f"restart {r} alone: {k} differs"
    # max_iter = 0 at the final W: the moments without the decorrelation, whatever the status
    m = call(ctx, Z, a["W"], 0, fun=fun, status=np.array([0, 1, 2, 0, 1, 2, 0]), iters=np.arange(7))
    assert np.array_equal(bits(m["W"]), bits(a["W"])) and (m["iters"] == np.arange(7)).all() and (m["lim"] == -7.0).all()
    assert (m["status"] == [0, 1, 2, 0, 1, 2, 0]).all() and (m["W1"] != -7.0).all() and (m["gmean"] != -7.0).all()


def test_stopped_restarts_are_untouched(ctx):
    import torch
    from xeofs_amd import engine

    Z, W = mixed_state()
    status = np.array([1, 0, 2, 0, 1, 2, 0], np.int32)
    res = call(ctx, Z, W, 3, status=status, iters=10 * np.arange(7), tol=1e-6)
    for r in range(7):
        if status[r]:
            assert np.array_equal(bits(res["W"][r]), bits(W[r])) and (res["W1"][r] == -7.0).all() and (res["gmean"][r] == -7.0).all()
            assert res["lim"][r] == -7.0 and res["iters"][r] == 10 * r and res["status"][r] == status[r]
        else:
            assert 10 * r < res["iters"][r] <= 10 * r + 3 and res["status"][r] != 2 and res["lim"][r] != -7.0
            assert not np.array_equal(res["W"][r], W[r])
    # a null output pointer writes nothing: the state alone moves, equal to the run with outputs
    st = State(ctx, W, status, 10 * np.arange(7))
    out = engine.fastica(ctx, Z, st.W, st.status, st.iters, tol=1e-6, max_iter=3, want=())
    ctx.synchronize()
    assert out == {}
    h = st.host()
    same(h, res, "no outputs", ("W", "status", "iters"))
    assert all((h[k] == -7).all() for k in ("W1", "gmean", "lim", "nused"))
    only = engine.fastica(ctx, Z, st.W, st.status, st.iters, tol=1e-6, max_iter=0, want=("gmean",))
    assert set(only) == {"gmean"} and only["gmean"].dtype == torch.float64


def test_rows_with_nan_or_infinity_are_left_out(ctx):
    Z, W = mixed_state(q=6, n=900, R=2)
    bad = Z.copy()
    rows = [0, 5, 255, 256, 511, 899]
    for i, v in zip(rows, (np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan)):
        bad[i, i % 6] = v
    keep = np.ones(900, bool)
    keep[rows] = False
    Zk = np.asarray(Z[keep], np.float64)
    for fun in kr.FUNS:
        a = call(ctx, bad, W, 0, fun=fun)
        b = call(ctx, Z[keep], W, 0, fun=fun)
        assert int(a["nused"][0]) == 894 and int(b["nused"][0]) == 894
        for r in range(2):
            check_moments({k: a[k][r] for k in ("W1", "gmean")}, bad, W[r], fun, 1.0, f"{fun} with bad rows")
            # the same rows in other blocks: the float64 sums differ by their own rounding and no more
            g, gp, _ = kr.contrast(Zk @ W[r].T, fun)
            tol = 4 * 894 * EPS53 * ((np.abs(g).T @ np.abs(Zk)) / 894 + (np.abs(gp).sum(axis=0) / 894)[:, None] * np.abs(W[r]))
            assert (np.abs(a["W1"][r] - b["W1"][r]) <= tol).all()
        s2 = call(ctx, bad, W, 2, fun=fun, tol=1e-6)
        assert (s2["iters"] >= 1).all() and (s2["status"] != 2).all() and int(s2["nused"][0]) == 894
    alln = call(ctx, np.full((10, 6), np.nan, np.float32), W, 1)
    assert (alln["status"] == 2).all() and int(alln["nused"][0]) == 0 and np.array_equal(bits(alln["W"]), bits(W)) and (alln["iters"] == 0).all()


def test_degenerate_and_trivial_inputs(ctx):
    rs = np.random.RandomState(5)
    q = 6
    W = np.stack([kr.random_orthogonal(q, rs) for _ in range(2)])
    zero = np.zeros((300, q), np.float32)
    a = call(ctx, zero, W, 3, fun="logcosh", alpha=1.5)
    assert np.array_equal(a["W1"], -1.5 * W) and (a["status"] == 1).all() and (a["iters"] == 1).all() and (a["lim"] <= 16 * q * EPS52).all()
    assert np.abs(a["W"] + W).max() <= 16 * q * EPS52
    c = call(ctx, zero, W, 3, fun="cube")
    assert (c["W1"] == 0).all() and (c["status"] == 2).all() and (c["iters"] == 0).all() and np.array_equal(bits(c["W"]), bits(W))
    assert (c["lim"] == -7.0).all()
    Z, _ = kr.mixed_panel(2, 512, q)
    twin = W.copy()
    twin[0, 4] = twin[0, 1]
    for fun in kr.FUNS:
        t = call(ctx, Z, twin, 2, fun=fun)
        assert t["status"][0] == 2 and t["iters"][0] == 0 and np.array_equal(bits(t["W"][0]), bits(twin[0])), fun
        assert t["status"][1] != 2 and t["iters"][1] >= 1


def test_every_refusal(ctx):
    import torch
    from xeofs_amd import _lib, engine

    dev = f"cuda:{ctx.device}"
    Z = np.random.RandomState(0).standard_normal((10, 3)).astype(np.float32)

    def refuse(match, Z=Z, W=None, T=1, R=1, **kw):
        q = Z.shape[1] if getattr(Z, "ndim", 2) == 2 else 1
        W = torch.zeros((R, q, q), dtype=torch.float64, device=dev) if W is None else W
        R = W.shape[0] if hasattr(W, "shape") and len(W.shape) else 1
        status = kw.pop("status", torch.zeros(R, dtype=torch.int32, device=dev))
        iters = kw.pop("iters", torch.zeros(R, dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match=match):
            engine.fastica(ctx, Z, W, status, iters, max_iter=T, **kw)

    refuse("q <= 32", Z=np.zeros((40, 33), np.float32))
    refuse("R <= 1024", R=1025)
    refuse("n <= 4194304", Z=torch.zeros((4194305, 1), dtype=torch.float32, device=dev))
    refuse("64", T=65)
    refuse("max_iter", T=-1)
    refuse("max_iter", T=True)
    refuse("max_iter", T=1.5)
    refuse("fun", fun="tanh")
    refuse("alpha", alpha=0.5)
    refuse("alpha", alpha=2.5)
    refuse("alpha", alpha=float("nan"))
    refuse("tol", tol=0.0)
    refuse("tol", tol=-1.0)
    refuse("tol", tol=2.0)
    refuse("tol", tol=float("nan"))
    refuse("matrix", Z=Z[0])
    refuse(">= 1", Z=Z[:0])
    refuse(">= 1", R=0)
    refuse("W must", W=torch.zeros((1, 3, 4), dtype=torch.float64, device=dev))
    refuse("W must", W=torch.zeros((1, 3, 3), dtype=torch.float32, device=dev))
    refuse("W must", W=np.zeros((1, 3, 3)))
    refuse("status", status=torch.zeros(2, dtype=torch.int32, device=dev))
    refuse("iters", iters=torch.zeros(1, dtype=torch.int64, device=dev))
    refuse("unknown", out=dict(w1=None))
    refuse("unknown", want=("w1",))
    refuse("W1", out=dict(W1=torch.zeros((1, 3, 4), dtype=torch.float64, device=dev)))
    refuse("gmean", out=dict(gmean=torch.zeros((1, 3), dtype=torch.float32, device=dev)))
    refuse("lim", out=dict(lim=torch.zeros((2,), dtype=torch.float64, device=dev)))
    refuse("nused", out=dict(nused=torch.zeros((1,), dtype=torch.int32, device=dev)))
    # the entry itself: fun out of range, a row stride below q, a missing and a host buffer
    Zd = torch.from_numpy(Z).to(dev)
    Wd = torch.zeros((1, 3, 3), dtype=torch.float64, device=dev)
    st, it = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    lib = ctx.lib

    def entry(Zp=None, ldz=3, Wp=None, fun=0, stp=None):
        return lib.eofx_fastica_f32(ctx.handle, p(Zd) if Zp is None else Zp, 10, 3, ldz, p(Wd) if Wp is None else Wp, 1, fun, 1.0, 1e-4, 1,
                                    p(st) if stp is None else stp, p(it), None, None, None, None)

    assert entry() == 0
    assert entry(fun=3) == _lib.ERR_ARG and entry(fun=-1) == _lib.ERR_ARG
    assert entry(ldz=2) == _lib.ERR_ARG
    host = np.zeros((1, 3, 3))
    assert entry(Wp=host.ctypes.data) == _lib.ERR_ARG
    assert entry(stp=0) == _lib.ERR_ARG
    ctx.synchronize()
