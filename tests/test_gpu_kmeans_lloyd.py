"""GPU tests of the Lloyd solver of weather-regime clustering (engine.kmeans_lloyd; csrc/eofx_kmeans.hpp) against the float64
restatement (tests/kmeans_reference.py) on the same float32 operands.

Exact fields are compared bit for bit: integer data with |z| <= 64 and integer centroids (every (z - c)^2 and every sum of at
most 32 of them is an integer below 2^24, so the float32 chain is exact, ties included); one full step on integer data (the
float64 sum is exact and the centroid must equal float32(sum / count)); several steps on dyadic data whose clusters hold
power-of-two counts on the whole trajectory (every centroid stays dyadic, every own-cluster distance exact).

General data go one step at a time, each launch replayed in float64 from the centroids the device was given:
    labels      equal on every row whose margin (d_second - d_best) / d_second exceeds 2 (q + 3) 2^-24 -- the two distances carry
                (q + 2) 2^-24 each: one rounding of every z - c (2 2^-24 on its square) and q roundings of the chain on a sum of
                non-negative terms -- and the rows at or below it stay within 0.1 % of the rows (one row is always allowed)
    mind2       |mind2_i - d64_i| <= (q + 3) 2^-24 d64_i against the float64 distance to the centroid the DEVICE chose
    inertia     within ((q + 3) 2^-24 + n 2^-53) relative of the float64 sum of those distances
    centroids   against the float64 mean over the DEVICE's labels within n 2^-53 sum_i |z_ij| / count + 2^-24 |c_cj|: a float64
                sum of `count` <= n terms in any order, an exact float64 division and one rounding to float32
Every test prints its worst error-to-bound ratio.  No test here tries to make the kernel fault or hang."""

import numpy as np
import pytest

import kmeans_reference as kr

pytestmark = pytest.mark.gpu

EPS24, EPS53 = 2.0 ** -24, 2.0 ** -53
KEYS = ("labels", "centroids", "counts", "inertia", "iters", "converged", "mind2")


def run(ctx, Z, C0, T, **kw):
    """engine.kmeans_lloyd -> a dict of host arrays (mind2 always asked for)"""
    from xeofs_amd import engine

    kw.setdefault("want_mind2", True)
    res = engine.kmeans_lloyd(ctx, Z, C0, T, **kw)
    ctx.synchronize()
    return {name: t.cpu().numpy() for name, t in res.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_state(a, b, what=""):
    """C, labels, counts, mind2 and inertia of two results, bit for bit"""
    for name in ("centroids", "labels", "counts", "mind2", "inertia"):
        assert np.array_equal(bits(a[name]), bits(b[name])), f"{what}: {name} differs"


def d64_to(Z, C, labels):
    """float64 squared distance of every row to the centroid `labels` names (NaN for label -1)"""
    Z, C = np.asarray(Z, np.float64), np.asarray(C, np.float64)
    ok = labels >= 0
    d = np.full(Z.shape[0], np.nan)
    d[ok] = ((Z[ok] - C[labels[ok]]) ** 2).sum(axis=1)
    return d


def check_assignment(Z, C, res_r, what):
    """one restart's labels, mind2, counts and inertia against float64 and the centroids C they belong to -> (undecided rows,
    the worst mind2 and inertia ratios)"""
    n, q = Z.shape
    labels, mind2 = res_r["labels"].astype(np.int64), res_r["mind2"].astype(np.float64)
    ref_l, _, margin = kr.assign(Z, C)
    decided = margin > kr.undecided_margin(q)
    assert np.array_equal(labels[decided], ref_l[decided]), f"{what}: a decided row has another label"
    und = int((~decided).sum())
    assert und <= kr.allowed_undecided(n), f"{what}: {und} undecided rows of {n}"
    assert ((labels >= 0) & (labels < C.shape[0])).all()
    assert np.array_equal(res_r["counts"], np.bincount(labels, minlength=C.shape[0]))
    d = d64_to(Z, C, labels)
    bound = (q + 3) * EPS24 * d
    err = np.abs(mind2 - d)
    assert (err <= bound).all(), f"{what}: mind2 off by {np.max(err / np.maximum(bound, 1e-300)):.3g} of its bound"
    r_md = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))
    ib = ((q + 3) * EPS24 + n * EPS53) * d.sum()
    ie = abs(float(res_r["inertia"]) - d.sum())
    assert ie <= ib, f"{what}: inertia off by {ie / max(ib, 1e-300):.3g} of its bound"
    return und, r_md, (ie / ib if ib > 0 else 0.0)


def check_centroids(Z, C_in, labels, C_out, what):
    """the update: C_out against the float64 mean over the device's `labels`; a cluster without rows keeps C_in bit for bit
    -> the worst ratio"""
    Z64 = np.asarray(Z, np.float64)
    n = Z.shape[0]
    worst = 0.0
    for c in range(C_in.shape[0]):
        mem = labels == c
        m = int(mem.sum())
        if m == 0:
            assert np.array_equal(bits(C_out[c]), bits(C_in[c])), f"{what}: the empty cluster {c} moved"
            continue
        ref = Z64[mem].sum(axis=0) / m
        bound = n * EPS53 * np.abs(Z64[mem]).sum(axis=0) / m + EPS24 * np.abs(ref)
        err = np.abs(C_out[c].astype(np.float64) - ref)
        assert (err <= bound).all(), f"{what}: centroid {c} off by {np.max(err / np.maximum(bound, 1e-300)):.3g} of its bound"
        worst = max(worst, float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0))))
    return worst


def restart(res, r):
    return {name: v[r] for name, v in res.items()}


# ------------------------------------------------------------------------------------------------ exact fields
EXACT = [(1, 1, 1, 1), (2, 2, 2, 2), (63, 3, 3, 1), (65, 5, 31, 2), (255, 4, 2, 3), (257, 32, 32, 2), (513, 16, 3, 1), (1025, 31, 32, 1),
         (4099, 2, 5, 3), (511, 1, 2, 300)]


def integer_case(n, q, k, R, seed=0):
    rs = np.random.RandomState(7919 * n + 31 * q + k + seed)
    Z = rs.randint(-64, 65, size=(n, q)).astype(np.float32)
    C0 = rs.randint(-64, 65, size=(R, k, q)).astype(np.float32)
    if k >= 3:
        C0[:, k - 1] = C0[:, 0]                    # two equal centroids: every row nearest to them is a tie
    if n >= 3:
        Z[n // 2] = C0[0, 0]                       # a row on a centroid
    return Z, C0


@pytest.mark.parametrize("n, q, k, R", EXACT)
def test_integer_assignment_bit_for_bit(ctx, n, q, k, R):
    Z, C0 = integer_case(n, q, k, R)
    res = run(ctx, Z, C0, 0)
    assert (res["iters"] == 0).all() and (res["converged"] == 0).all() and np.array_equal(bits(res["centroids"]), bits(C0))
    ties = 0
    for r in range(R):
        D = ((Z.astype(np.float64)[:, None, :] - C0[r].astype(np.float64)[None]) ** 2).sum(axis=2)      # integers: exact
        lab = np.argmin(D, axis=1)                                                                       # the first of equals
        best = D[np.arange(n), lab]
        ties += int(((D == best[:, None]).sum(axis=1) > 1).sum())
        assert np.array_equal(res["labels"][r], lab)
        assert np.array_equal(res["mind2"][r].astype(np.float64), best) and float(res["inertia"][r]) == best.sum()
        assert np.array_equal(res["counts"][r], np.bincount(lab, minlength=k))
    print(f"n={n} q={q} k={k} R={R}: {ties} rows with tied distances, all at the lowest index")
    assert ties > 0 or k < 3


@pytest.mark.parametrize("n, q, k, R", EXACT)
def test_one_full_step_on_integer_data(ctx, n, q, k, R):
    Z, C0 = integer_case(n, q, k, R, seed=1)
    res = run(ctx, Z, C0, 1)
    assert (res["iters"] == 1).all()
    Z64 = Z.astype(np.float64)
    for r in range(R):
        lab, _, _ = kr.assign(Z, C0[r])                                          # exact
        want = C0[r].copy()
        for c in range(k):
            if (lab == c).any():
                want[c] = np.float32(Z64[lab == c].sum(axis=0) / (lab == c).sum())
        assert np.array_equal(bits(res["centroids"][r]), bits(want))
        assert np.array_equal(res["counts"][r], np.bincount(res["labels"][r], minlength=k))


def dyadic_case(q, k, m, seed=0):
    """Clusters in pairs, a pair every 4096 along column 0: three groups of 2^(m+1) rows at x = 0, 10 and 40 and the starts in the
    first two.  Assignment 1 gives (A | B C), assignment 2 (A B | C), assignment 3 repeats it: 2 updates, every count a power of
    two.  An odd k ends with a single cluster of 2^(m+1) rows.  Offsets are -1/2, 0 or 1/2 and sum to zero in pairs: the other
    columns move a squared distance by at most 31, the groups are 81 apart at the least.  Centroids then lie on a grid of
    2^-(m+3) below 2^16 and the squares of the own-cluster differences on 2^-(2m+6) below 512: 24 bits hold them up to m = 4.
    The rows are shuffled.  -> (Z, C0 [1 x k x q])"""
    rs = np.random.RandomState(1000 * q + 10 * k + m + seed)
    g = 2 ** (m + 1)
    rows, starts = [], []

    def group(x0):
        off = rs.randint(-1, 2, size=(g // 2, q)) / 2.0
        G = np.concatenate([off, -off])
        G[:, 0] += x0
        return G

    for b in range(k // 2):
        base = 4096.0 * b
        A, B, Cg = group(base), group(base + 10.0), group(base + 40.0)
        starts += [A[0].copy(), B[0].copy()]
        rows += [A, B, Cg]
    if k % 2:
        A = group(4096.0 * (k // 2))
        starts.append(A[0].copy())
        rows.append(A)
    Z = np.concatenate(rows)
    Z = Z[rs.permutation(Z.shape[0])]
    return Z.astype(np.float32), np.asarray(starts, dtype=np.float32)[None]


@pytest.mark.parametrize("q, k, m", [(1, 2, 0), (3, 3, 1), (5, 31, 2), (32, 32, 2), (16, 2, 4), (4, 1, 3), (31, 32, 4)])
def test_dyadic_trajectory_bit_for_bit(ctx, q, k, m):
    Z, C0 = dyadic_case(q, k, m)
    assert np.array_equal(Z.astype(np.float64) * 2, np.round(Z.astype(np.float64) * 2))
    for T in (1, 2, 5):
        ref = kr.lloyd(Z, C0[0], T)
        cnt = ref["counts"]
        assert all(c & (c - 1) == 0 for c in cnt.tolist())
        res = restart(run(ctx, Z, C0, T), 0)
        what = f"q={q} k={k} m={m} T={T}"
        assert (int(res["iters"]), int(res["converged"])) == (ref["iters"], ref["converged"]), what
        assert np.array_equal(res["labels"], ref["labels"]) and np.array_equal(res["counts"], cnt), what
        assert np.array_equal(res["centroids"].astype(np.float64), ref["C"]), what
        assert np.array_equal(res["mind2"].astype(np.float64), ref["mind2"]) and float(res["inertia"]) == ref["inertia"], what
    assert ref["iters"] == (2 if k >= 2 else 1) and ref["converged"] == 1


# ------------------------------------------------------------------------------------------------ general data, a step at a time
@pytest.mark.parametrize("case", kr.CASES, ids=kr.case_id)
def test_general_data_one_step_at_a_time(ctx, case):
    n, q, k, R, _ = case
    Z, C = kr.make_case(case)
    worst = dict(undecided=0, mind2=0.0, inertia=0.0, centroid=0.0)
    for s in range(kr.STEPS):
        first = run(ctx, Z, C, 0)                                                # the assignment the step starts with
        one = run(ctx, Z, C, 1)
        assert (one["iters"] == 1).all()
        for r in range(R):
            what = f"{kr.case_id(case)} step {s} restart {r}"
            for res, Cr in ((restart(first, r), C[r]), (restart(one, r), one["centroids"][r])):
                und, r_md, r_in = check_assignment(Z, Cr, res, what)
                worst.update(undecided=max(worst["undecided"], und), mind2=max(worst["mind2"], r_md), inertia=max(worst["inertia"], r_in))
            worst["centroid"] = max(worst["centroid"], check_centroids(Z, C[r], first["labels"][r], one["centroids"][r], what))
            assert int(one["converged"][r]) == int(np.array_equal(one["labels"][r], first["labels"][r])), what
        C = one["centroids"]
    print(f"{kr.case_id(case)}: worst ratios to the bounds {worst}")


@pytest.mark.parametrize("case", [kr.CASES[3], kr.CASES[5], kr.CASES[9], kr.CASES[11], kr.CASES[13]], ids=kr.case_id)
def test_a_chain_of_one_step_launches_is_one_launch_and_reruns_are_equal(ctx, case):
    Z, C0 = kr.make_case(case)
    R = C0.shape[0]
    for T in (2, 3, 7):
        whole = run(ctx, Z, C0, T)
        again = run(ctx, Z, C0, T)
        assert_same_state(whole, again, "rerun")
        assert np.array_equal(whole["iters"], again["iters"]) and np.array_equal(whole["converged"], again["converged"])
        C, first_conv = C0, np.full(R, -1)
        for t in range(T):
            link = run(ctx, Z, C, 1)
            assert (link["iters"] == 1).all()
            first_conv = np.where((first_conv < 0) & (link["converged"] != 0), t + 1, first_conv)
            C = link["centroids"]
        assert_same_state(whole, link, f"{kr.case_id(case)} T={T}")
        assert np.array_equal(whole["converged"] != 0, first_conv > 0)
        assert np.array_equal(whole["iters"], np.where(first_conv > 0, first_conv, T))


@pytest.mark.parametrize("case", [kr.CASES[3], kr.CASES[7], kr.CASES[9], kr.CASES[13]], ids=kr.case_id)
def test_a_converged_state_is_a_fixed_point_in_float64(ctx, case):
    n, q, k, R, _ = case
    Z, C0 = kr.make_case(case)
    res = run(ctx, Z, C0, 1000)
    assert (res["converged"] == 1).all() and (res["iters"] >= 1).all()
    worst = 0.0
    for r in range(min(R, 20)):
        what = f"{kr.case_id(case)} restart {r}"
        check_assignment(Z, res["centroids"][r], restart(res, r), what)
        # every centroid is the mean of its members: the last update ran over these very labels
        worst = max(worst, check_centroids(Z, res["centroids"][r], res["labels"][r], res["centroids"][r], what))
    print(f"{kr.case_id(case)}: iterations {res['iters'].min()} .. {res['iters'].max()}, centroid ratio {worst:.3g}")


# ------------------------------------------------------------------------------------------------ the edges
def test_an_empty_cluster_keeps_its_centroid(ctx):
    Z, C0 = kr.make_case(kr.CASES[3])
    C0 = C0.copy()
    C0[:, 1] = 1.0e6                                                             # far from every row
    res = run(ctx, Z, C0, 5)
    assert (res["counts"][:, 1] == 0).all() and not (res["labels"] == 1).any()
    assert np.array_equal(bits(res["centroids"][:, 1]), bits(C0[:, 1])) and (res["counts"].sum(axis=1) == Z.shape[0]).all()
    assert (res["iters"] >= 1).all()


@pytest.mark.parametrize("n, q", [(1, 1), (64, 3), (257, 32), (1025, 5)])
def test_all_rows_identical(ctx, n, q):
    z = np.linspace(-3.25, 2.5, q, dtype=np.float32)
    Z = np.tile(z, (n, 1))
    k = min(3, n)
    C0 = np.stack([z, z + 1.0, z][:k])[None].astype(np.float32)
    res = restart(run(ctx, Z, C0, 4), 0)
    assert (res["labels"] == 0).all() and res["counts"].tolist() == [n, 0, 0][:k]      # a tie of 0 and 2: the lowest index
    assert (int(res["iters"]), int(res["converged"])) == (1, 1) and float(res["inertia"]) == 0.0 and (res["mind2"] == 0).all()
    assert np.array_equal(bits(res["centroids"]), bits(C0[0]))


def test_rows_that_are_not_finite_take_part_in_nothing(ctx):
    case = kr.CASES[8]                                                           # n = 257, q = 32, k = 32
    Z, C0 = kr.make_case(case)
    n, q = Z.shape
    bad = np.array([0, 63, 64, 200, 256])
    Za, Zb = Z.copy(), Z.copy()
    Za[bad, 0] = np.nan
    Zb[bad] = 3.0e38
    Zb[bad[:2], q - 1], Zb[bad[2:], 5] = np.inf, -np.inf
    for T in (0, 3):
        a, b = run(ctx, Za, C0, T), run(ctx, Zb, C0, T)
        for name in KEYS:                                                        # whatever the rows hold, bit for bit
            assert np.array_equal(bits(a[name]), bits(b[name])), name
        assert (a["labels"][:, bad] == -1).all() and np.isnan(a["mind2"][:, bad]).all()
        good = np.setdiff1d(np.arange(n), bad)
        assert (a["labels"][:, good] >= 0).all() and (a["counts"].sum(axis=1) == n - bad.size).all()
        assert np.isfinite(a["inertia"]).all() and np.isfinite(a["centroids"]).all()
    # one step against float64 over the finite rows
    first, one = run(ctx, Za, C0, 0), run(ctx, Za, C0, 1)
    for r in range(C0.shape[0]):
        lab = first["labels"][r].astype(np.int64)
        ref_l, _, margin = kr.assign(Za, C0[r])
        dec = margin > kr.undecided_margin(q)
        assert np.array_equal(lab[dec], ref_l[dec])
        check_centroids(np.where(np.isfinite(Za), Za, 0.0), C0[r], lab, one["centroids"][r], f"restart {r}")


@pytest.mark.parametrize("case", [kr.CASES[2], kr.CASES[5], kr.CASES[8], kr.CASES[9], kr.CASES[11]], ids=kr.case_id)
def test_strided_views_and_canaries(ctx, case):
    """Z as a view of a wider and longer panel of NaN (a NaN that is read would unlabel a row), every output in the middle of a
    buffer whose ends hold a pattern"""
    import torch
    from xeofs_amd import engine

    n, q, k, R, _ = case
    Z, C0 = kr.make_case(case)
    dev = f"cuda:{ctx.device}"
    plain = run(ctx, Z, C0, 3)
    big = torch.full((n + 3, q + 5), float("nan"), dtype=torch.float32, device=dev)
    big[:n, :q] = torch.from_numpy(Z).to(dev)
    view = big[:n, :q]
    assert view.stride(0) == q + 5
    shapes = dict(labels=(R, n), centroids=(R, k, q), counts=(R, k), inertia=(R,), iters=(R,), converged=(R,), mind2=(R, n))
    dts = dict(labels=torch.int32, centroids=torch.float32, counts=torch.int32, inertia=torch.float64, iters=torch.int32,
               converged=torch.int32, mind2=torch.float32)
    GUARD, bufs, out = 64, {}, {}
    for name in KEYS:
        numel = int(np.prod(shapes[name]))
        buf = torch.full((numel + 2 * GUARD,), 77, dtype=dts[name], device=dev)
        bufs[name] = buf
        out[name] = buf[GUARD:GUARD + numel].view(shapes[name])
    res = engine.kmeans_lloyd(ctx, view, C0, 3, out=out)
    ctx.synchronize()
    for name in KEYS:
        assert res[name] is out[name]
        assert np.array_equal(bits(res[name].cpu().numpy()), bits(plain[name])), name
        ends = torch.cat([bufs[name][:GUARD], bufs[name][-GUARD:]]).cpu().numpy()
        assert (ends == 77).all(), f"the canary around {name} changed"
    back = big.cpu().numpy()
    assert np.isnan(back[n:]).all() and np.isnan(back[:, q:]).all() and np.array_equal(back[:n, :q], Z)


def test_max_iter_at_zero_one_and_the_cap(ctx):
    from xeofs_amd import engine

    Z, C0 = kr.make_case(kr.CASES[3])
    zero, one, cap = run(ctx, Z, C0, 0), run(ctx, Z, C0, 1), run(ctx, Z, C0, engine.KMEANS_ITER_MAX)
    assert (zero["iters"] == 0).all() and (zero["converged"] == 0).all() and np.array_equal(bits(zero["centroids"]), bits(C0))
    assert (one["iters"] == 1).all()
    assert (cap["converged"] == 1).all() and (cap["iters"] < 100).all()
    assert_same_state(cap, run(ctx, Z, C0, 100), "the cap against 100")
    assert (cap["inertia"] <= one["inertia"] * (1 + 1e-6)).all() and (one["inertia"] <= zero["inertia"] * (1 + 1e-6)).all()
    with pytest.raises(ValueError, match="1000"):
        run(ctx, Z, C0, engine.KMEANS_ITER_MAX + 1)
    # the defaults: no mind2 unless asked for; a host array and a device tensor give the same
    res = engine.kmeans_lloyd(ctx, Z, C0, 2)
    assert sorted(res) == sorted(KEYS[:-1]) and res["labels"].dtype == engine._torch().int32
    assert np.array_equal(res["labels"].cpu().numpy(), run(ctx, engine.device_panel(ctx, Z), C0, 2)["labels"])


def test_every_refusal(ctx):
    import torch
    from xeofs_amd import _lib, engine

    rs = np.random.RandomState(0)
    Z = rs.standard_normal((10, 3)).astype(np.float32)
    C0 = Z[None, :4].copy()

    def refuse(match, Z=Z, C0=C0, T=1, **kw):
        with pytest.raises(ValueError, match=match):
            engine.kmeans_lloyd(ctx, Z, C0, T, **kw)

    refuse("more clusters than rows", Z=Z[:3])
    refuse("k <= 32", Z=rs.standard_normal((40, 3)).astype(np.float32), C0=np.zeros((1, 33, 3), np.float32))
    refuse("q <= 32", Z=np.zeros((40, 33), np.float32), C0=np.zeros((1, 2, 33), np.float32))
    refuse("R <= 4096", C0=np.zeros((4097, 2, 3), np.float32))
    refuse("n <= 262144", Z=torch.zeros((262145, 1), dtype=torch.float32, device=f"cuda:{ctx.device}"), C0=np.zeros((1, 1, 1), np.float32))
    for v in (np.nan, np.inf, -np.inf):
        bad = C0.copy()
        bad[0, 2, 1] = v
        refuse("NaN or an infinity", C0=bad)
    refuse("1000", T=1001)
    refuse("max_iter", T=-1)
    refuse("max_iter", T=True)
    refuse("max_iter", T=1.5)
    refuse("q = 3", C0=np.zeros((1, 2, 4), np.float32))
    refuse("R x k x q", C0=np.zeros((2, 3), np.float32))
    refuse("matrix", Z=Z[0])
    refuse(">= 1", Z=Z[:0], C0=np.zeros((1, 1, 3), np.float32))
    refuse(">= 1", C0=np.zeros((0, 2, 3), np.float32))
    refuse("unknown", out=dict(label=None))
    dev = f"cuda:{ctx.device}"
    refuse("labels", out=dict(labels=torch.zeros((1, 10), dtype=torch.int64, device=dev)))
    refuse("centroids", out=dict(centroids=torch.zeros((1, 4, 4), dtype=torch.float32, device=dev)))
    refuse("inertia", out=dict(inertia=torch.zeros((1,), dtype=torch.float32, device=dev)))
    refuse("mind2", out=dict(mind2=torch.zeros((2, 10), dtype=torch.float32, device=dev)))
    refuse("counts", out=dict(counts=torch.zeros((1, 8), dtype=torch.int32, device=dev)[:, ::2]))
    # the entry itself: a row stride below q, a missing output and a host buffer
    Zd, Cd = torch.from_numpy(Z).to(dev), torch.from_numpy(C0).to(dev)
    lab, cnt = torch.zeros((1, 10), dtype=torch.int32, device=dev), torch.zeros((1, 4), dtype=torch.int32, device=dev)
    ine, its, cv = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    Co = torch.zeros_like(Cd)
    p = _lib.ptr

    def entry(Zp=None, ldz=3, labels=lab, inertia=ine):
        return ctx.lib.eofx_kmeans_lloyd_f32(ctx.handle, p(Zd) if Zp is None else Zp, 10, 3, ldz, p(Cd), 4, 1, 1, p(labels), p(Co), p(cnt),
                                             p(inertia), p(its), p(cv), None)

    assert entry() == _lib.EOFX_OK
    assert entry(ldz=2) == _lib.ERR_ARG and entry(labels=None) == _lib.ERR_ARG and entry(Zp=p(Z)) == _lib.ERR_ARG
    assert entry(inertia=np.zeros(1)) == _lib.ERR_ARG
    ctx.synchronize()
    assert (lab.cpu().numpy() >= 0).all()
