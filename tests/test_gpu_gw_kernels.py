"""The GWPCA kernels one step at a time against an 80-bit reference (csrc/eofx_gw.hpp: gw_cov_kernel, gw_finalize_kernel,
gw_syev_kernel, through engine.gw_cov, engine.gwpca and engine.batched_syev).

Reference.  The definition restated in numpy.longdouble (eps 1.08e-19), two passes, no shift, no packed moments:
    w_ij = K(d_ij / b) from the coordinates the caller passed,  W = sum_j w,  mu = sum_j w x_j / W,
    C = sum_j w (x_j - mu)(x_j - mu)^T / W,  tv = trace C.
The field rows are the float32 array handed to engine.from_dense, promoted exactly.

Bound.  The kernel adds N_i terms w y_a y_b in float64, y = x - r with r the mean of (up to) 16 rows of the field, so
|y_ja| <= 2 M_a with M_a = max_j |x_ja - mean_j x_ja|, and then forms (S_ab - S_a S_b / W) / W.  Asserted, entry by entry:
    |C_dev - C_ref|_ab <= (N_i + 8) 2^-52 4 M_a M_b,      |tv_dev - tv_ref| <= the sum of the diagonal bounds,
N_i = the number of locations whose weight is non-zero in float64.  It is derived, not tuned; tests/test_gw_model_host.py
shows a float64 emulation of the kernel's algorithm inside half of it and two broken variants (float32 weights, no shift)
far outside, without a GPU.

Haversine.  The device's a = sin^2(dlat / 2) + cos cos sin^2(dlon / 2) carries an absolute error of at most
da = 64 * 2^-53 (u = 2^-53: the radians of a coordinate are off by 2u relative, 4 pi u for |lon| <= 2 pi and pi u for a
latitude; half the difference of two of them by 5 pi u and 1.5 pi u; sin^2 has a slope <= 1 and sin and the square
round, 21u and 10u; the product of the two cosines 9.3u; the sum 43u, rounded up), and d = 2 R asin(sqrt a) amplifies it
by R / sqrt(a (1 - a)).  The general cases keep 1 - a >= 1e-6 for every pair with a non-zero weight (asserted on the
reference) and are held to the bound above as it stands.  The one antipodal case adds, for the pairs with 1 - a < 1e-6 only:
asin(sqrt .) is concave and 0 at 0, hence subadditive, so |d_dev - d_ref| <= dd = 2 R asin(sqrt da); every kernel decreases
with d, so |w_dev - w_ref| <= dw = max(w(d - dd) - w(d), w(d) - w(min(d + dd, pi R))) (longdouble); and
dC / dw_j = ((x_j - mu)(x_j - mu)^T - C) / W, at most 8 M_a M_b / W in absolute value, so the extra term of centre i is
    sum over those pairs of dw_ij * 8 M_a M_b / W_i        (first order; the next is (dw / W)^2, 1e-20).

Eigenpairs.  numpy.linalg.eigh of the DEVICE's covariance, so the eigensolver's error is kept apart from the covariance's, at
the tolerances of test_gpu_gwpca.test_batched_syev_vs_numpy.

Global covariance.  Where every weight is 1 within delta (one point, a bandwidth of 1e9) the normalised weights differ from
1 / n by at most 2 delta / (1 - delta) in sum, so both terms of C move by at most that times M_a M_b and its square: C is the
unweighted covariance within 4 delta M_a M_b, which is added to the bound for that comparison.

Every test prints the share of the covariance bound the device used (run with -s).  Largest per case group on an MI355X:
features 0.035 (p = 127), locations 0.043 (n = 2), kernels 0.014 (haversine, bisquare), ranges 0.011, geometry 0.0077,
shift 0.018.
"""

import functools

import numpy as np
import pytest

import test_gpu_gwpca as gwp

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -52
R_EARTH = LD(6371.0)
DA = 64.0 * 2.0 ** -53          # the absolute error of the device's haversine a (module docstring)
GW_T = 16


# ------------------------------------------------------------------------------------------------ the reference
def ld_pi():
    return 4 * np.arctan(LD(1))


def kernel_ld(d, bw, kernel):
    u = d / LD(bw)
    if kernel == "bisquare":
        return np.where(d <= LD(bw), (1 - u * u) ** 2, LD(0))
    with np.errstate(under="ignore"):
        return np.exp(-u * u / 2) if kernel == "gaussian" else np.exp(-u / 2)


def ref_weights(xy, metric, kernel, bw):
    """-> (w [n, n], d [n, n], 1 - a [n, n] or None) in longdouble, from the coordinates as passed"""
    assert np.finfo(LD).eps < 1e-18, "the reference needs an 80-bit long double"
    xy = np.asarray(xy, np.float64).astype(LD)
    one_minus_a = None
    if metric == "haversine":
        lon, lat = xy[:, 0] * (ld_pi() / 180), xy[:, 1] * (ld_pi() / 180)
        a = np.sin((lat[None, :] - lat[:, None]) / 2) ** 2 + \
            np.cos(lat)[:, None] * np.cos(lat)[None, :] * np.sin((lon[None, :] - lon[:, None]) / 2) ** 2
        a = np.clip(a, LD(0), LD(1))
        one_minus_a = 1 - a
        d = R_EARTH * 2 * np.arctan2(np.sqrt(a), np.sqrt(one_minus_a))
    else:
        d = np.sqrt((xy[None, :, 0] - xy[:, None, 0]) ** 2 + (xy[None, :, 1] - xy[:, None, 1]) ** 2)
    return kernel_ld(d, bw, kernel), d, one_minus_a


class Ref:
    """C [count, p, p], tv [count] (longdouble), N [count], M [p], bound [count, p, p] (float64, the antipodal term included
    where the case asks for it), near_antipodal = the number of pairs that term covers"""


def reference(case):
    return _reference(case.name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = CASE[name]
    X = case.X.astype(LD)
    n, p = X.shape
    w_all, d_all, oma = ref_weights(case.xy, case.metric, case.kernel, case.bw)
    dev = X - X.mean(0)
    M = np.abs(dev).max(0)
    MM = (4 * M[:, None] * M[None, :])
    r = Ref()
    r.M = M.astype(np.float64)
    r.C = np.zeros((case.count, p, p), LD)
    r.tv = np.zeros(case.count, LD)
    r.N = np.zeros(case.count, np.int64)
    r.bound = np.zeros((case.count, p, p))
    r.near_antipodal = 0
    for s in range(case.count):
        i = case.first + s
        w = w_all[i]
        live = w.astype(np.float64) != 0.0
        keep = w != 0
        if oma is not None:
            near = keep & (oma[i] < 1e-6)
            assert case.antipodal or not near.any(), (name, i)
        wk, x = w[keep], X[keep]
        W = wk.sum()
        mu = (wk[:, None] * x).sum(0) / W
        y = x - mu
        r.C[s] = (wk[:, None] * y).T @ y / W
        r.tv[s], r.N[s] = np.trace(r.C[s]), int(live.sum())
        b = (r.N[s] + 8) * LD(EPS) * MM
        if case.antipodal and near.any():
            dd = 2 * R_EARTH * np.arcsin(np.sqrt(LD(DA)))
            dj = d_all[i][near]
            w0 = kernel_ld(dj, case.bw, case.kernel)
            dw = np.maximum(kernel_ld(dj - dd, case.bw, case.kernel) - w0,
                            w0 - kernel_ld(np.minimum(dj + dd, ld_pi() * R_EARTH), case.bw, case.kernel))
            b = b + dw.sum() * 2 * MM / W
            r.near_antipodal += int(near.sum())
        r.bound[s] = b.astype(np.float64)
    return r


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, group, name, xy, X, metric="euclidean", kernel="bisquare", bw=6.0, first=0, count=None, zero=False,
                 antipodal=False, unweighted=False):
        self.group, self.name = group, f"{group}-{name}"
        self.xy = np.ascontiguousarray(xy, np.float64)
        self.X = np.ascontiguousarray(X, np.float32)
        self.metric, self.kernel, self.bw = metric, kernel, float(bw)
        self.first, self.count = first, self.X.shape[0] - first if count is None else count
        self.zero = zero                 # every C_i == 0 and tv == 0 exactly
        self.antipodal = antipodal       # the haversine term of the module docstring is added to the bound
        self.unweighted = unweighted     # every weight is 1 up to max |1 - w|: also against the global covariance
        self.n, self.p = self.X.shape
        assert self.xy.shape == (self.n, 2)

    def __repr__(self):
        return self.name


def box(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 20.0, (n, 2))


def make_field(xy, p, seed, offset=0.0):
    """test_gpu_gwpca.field (locally structured, clear local gaps); plain noise at p = 1, which that one cannot make"""
    if p >= 2:
        return gwp.field(xy, p, seed, offset)
    return (np.random.default_rng(seed).normal(size=(xy.shape[0], 1)) * 3.0 + offset).astype(np.float32)


def sphere_set(n, seed):
    """n locations across the dateline (longitudes 150 .. 210 written in [-180, 180)), a tenth of them in a cap around the north
    pole with the pole itself; no pair further apart than 170 degrees, so 1 - a >= 1e-6 everywhere"""
    rng = np.random.default_rng(seed)
    lon = rng.uniform(150.0, 210.0, n)
    lat = rng.uniform(-55.0, 60.0, n)
    m = n // 10
    lat[:m] = rng.uniform(84.0, 90.0, m)
    lon[:m] = rng.uniform(0.0, 360.0, m)
    lat[0] = 90.0
    return np.stack([np.where(lon >= 180.0, lon - 360.0, lon), lat], 1)


def antipodal_set():
    """both poles at several longitudes, one generic exactly antipodal pair, and 30 locations around them"""
    rng = np.random.default_rng(71)
    xy = np.stack([rng.uniform(-180.0, 180.0, 40), rng.uniform(-70.0, 70.0, 40)], 1)
    xy[0:3] = [(0.0, 90.0), (117.0, 90.0), (-45.0, 90.0)]
    xy[3:6] = [(10.0, -90.0), (-170.0, -90.0), (90.0, -90.0)]
    xy[6], xy[7] = (10.0, 30.0), (-170.0, -30.0)
    xy[8], xy[9] = (100.0, 0.0), (-80.0, 0.0)
    return xy


def grid8():
    g0, g1 = np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij")
    return np.stack([g0.reshape(-1), g1.reshape(-1)], 1)


FEATURE_COUNTS = [1, 2, 3, 7, 14, 15, 16, 63, 64, 65, 127, 255, 256]
LOCATION_COUNTS = [1, 2, 15, 16, 17, 31, 32, 33, 47]
RANGES = [(0, 1), (99, 1), (5, 1), (3, 16), (10, 50), (7, 93), (0, 100)]
SPHERE_BW = {"bisquare": 3000.0, "gaussian": 1500.0, "exponential": 1000.0}
BOX_BW = {"bisquare": 6.0, "gaussian": 3.0, "exponential": 2.0}


def build_cases():
    out = []
    for p in FEATURE_COUNTS:
        xy = box(40, 100 + p)
        out.append(Case("features", f"p{p}", xy, make_field(xy, p, 200 + p)))
    for n in LOCATION_COUNTS:
        xy = box(n, 300 + n)
        out.append(Case("locations", f"n{n}", xy, make_field(xy, 5, 400 + n), zero=n == 1))
    sph = sphere_set(100, 51)
    sph360 = np.stack([sph[:, 0] % 360.0, sph[:, 1]], 1)
    assert sph360[:, 0].max() > 180.0 and sph[:, 0].min() < -150.0
    b100 = box(100, 52)
    for kernel in ("bisquare", "gaussian", "exponential"):
        out.append(Case("kernels", f"euclidean-{kernel}", b100, make_field(b100, 9, 53), "euclidean", kernel, BOX_BW[kernel]))
        out.append(Case("kernels", f"haversine-{kernel}", sph, make_field(sph, 9, 54), "haversine", kernel, SPHERE_BW[kernel]))
        out.append(Case("kernels", f"haversine360-{kernel}", sph360, make_field(sph, 9, 54), "haversine", kernel,
                        SPHERE_BW[kernel]))
    Xr = make_field(b100, 9, 55)
    for first, count in RANGES:
        out.append(Case("ranges", f"{first}+{count}", b100, Xr, first=first, count=count))
    # geometry
    one = np.tile([[12.5, -3.0]], (40, 1))
    out.append(Case("geometry", "one-point", one, make_field(box(40, 60), 6, 61), unweighted=True))
    line = box(40, 62)
    line[:, 1] = 7.25
    out.append(Case("geometry", "one-line", line, make_field(line, 6, 63)))
    twice = np.concatenate([box(20, 64)] * 2)
    out.append(Case("geometry", "duplicates", twice, make_field(box(40, 65), 6, 66)))
    g = grid8()
    Xg = make_field(g, 6, 67)
    out.append(Case("geometry", "grid-bw5", g, Xg, bw=5.0))
    out.append(Case("geometry", "grid-bw5-", g, Xg, bw=np.nextafter(5.0, 0.0)))
    out.append(Case("geometry", "grid-alone", g, Xg, bw=0.01, zero=True))
    for kernel in ("bisquare", "gaussian", "exponential"):
        out.append(Case("geometry", f"global-{kernel}", b100[:40], make_field(b100[:40], 6, 68), kernel=kernel, bw=1e9,
                        unweighted=True))
    anti = antipodal_set()
    out.append(Case("geometry", "antipodal", anti, make_field(anti, 6, 69), "haversine", "gaussian", 5000.0, antipodal=True))
    # shift
    rng = np.random.default_rng(70)
    xs = box(40, 72)
    out.append(Case("shift", "constant-1e4", xs, 1e4 + rng.normal(size=(40, 7))))
    out.append(Case("shift", "field-1e3", xs, gwp.field(xs, 7, 73, offset=1e3)))
    return out


CASES = build_cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
GWPCA_P = [1, 2, 15, 63, 64]


def passes(p):
    """gw_run: the grid's second dimension, ceil(16 (p + 1)(p + 2) / 2 / 2048)"""
    return -(-((p + 1) * (p + 2) // 2) // 128)


# ------------------------------------------------------------------------------------------------ the checks
SHARES = {}


def check_covariance(case, cov, tv):
    """cov [count, p, p], tv [count] float64 against the reference within the bound -> the largest share of the bound used"""
    ref = reference(case)
    assert cov.shape == ref.C.shape and tv.shape == ref.tv.shape
    assert np.isfinite(cov).all() and np.isfinite(tv).all()
    err = np.abs(cov.astype(LD) - ref.C).astype(np.float64)
    terr = np.abs(tv.astype(LD) - ref.tv).astype(np.float64)
    tbound = np.einsum("iaa->i", ref.bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(ref.bound > 0, err / ref.bound, 0.0).max()
        tshare = np.where(tbound > 0, terr / tbound, 0.0).max()
    print(f"share of the bound: {case.name}: cov {share:.3g}, tv {tshare:.3g}, N {ref.N.min()}..{ref.N.max()}")
    SHARES[case.name] = max(share, tshare)
    assert np.all(err <= ref.bound), (case.name, share, np.argwhere(err > ref.bound)[:3])
    assert np.all(terr <= tbound), (case.name, tshare)
    if case.zero:
        assert np.all(cov == 0.0) and np.all(tv == 0.0)
    if case.unweighted:         # every weight is 1 within delta: C is the global covariance within 4 delta M_a M_b
        w, _, _ = ref_weights(case.xy, case.metric, case.kernel, case.bw)
        delta = float(np.abs(1 - w).max())
        assert delta < 1e-7
        y = case.X.astype(LD) - case.X.astype(LD).mean(0)
        G = y.T @ y / case.n
        slack = 4 * delta * ref.M[:, None] * ref.M[None, :]
        assert np.all(np.abs(ref.C - G).astype(np.float64) <= slack + 1e-17 * ref.M[:, None] * ref.M[None, :])
        assert np.all(np.abs(cov.astype(LD) - G).astype(np.float64) <= ref.bound + slack)
    return max(share, tshare)


def check_invariants(case, cov, tv):
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    trace = np.einsum("iaa->i", cov)
    assert np.all(np.abs(tv - trace) <= case.p * EPS * tv), np.abs(tv - trace).max()


def run_cov(ctx, mat, case):
    from xeofs_amd import engine

    out = engine.gw_cov(ctx, mat, case.xy, case.metric, case.kernel, case.bw, case.first, case.count)
    return out[0], out[0].cpu().numpy(), out[1].cpu().numpy(), out[2]


def spectrum(cov):
    """numpy's float64 eigenpairs of the device's covariances: descending, signed by the rule"""
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[:, ::-1], vec[:, :, ::-1]
    sign = np.where(np.abs(vec.max(axis=1)) >= np.abs(vec.min(axis=1)), 1.0, -1.0)
    return lam, vec * sign[:, None, :]


def check_syev(A, w, V, k):
    """one matrix: the k largest eigenpairs at the tolerances of test_batched_syev_vs_numpy"""
    p = A.shape[0]
    ref = np.linalg.eigvalsh(A)[::-1]
    scale = max(1.0, np.abs(ref).max())
    assert w.shape == (k,) and V.shape == (p, k)
    np.testing.assert_allclose(w, np.maximum(ref[:k], 0), atol=1e-12 * scale * p, rtol=0)
    assert np.abs(V.T @ V - np.eye(k)).max() < 1e-12 * max(p, 4)
    assert np.abs(A @ V - V * ref[:k]).max() < 1e-11 * scale * p         # ref, not w: a clamped value is not an eigenvalue
    assert np.all(np.diff(w) <= 0) and np.all(w >= 0)
    assert np.all(np.abs(V.max(0)) >= np.abs(V.min(0)))


def check_gwpca(ctx, mat, case, cov, tv, k, chunk=None):
    """engine.gwpca (the sorted plan, its own tiling) against numpy's spectrum of the gw_cov covariances"""
    from xeofs_amd import engine

    ref = reference(case)
    p = case.p
    V, ev, tv2, st = engine.gwpca(ctx, mat, case.xy, k, case.bw, case.metric, case.kernel, chunk=chunk)
    assert V.shape == (case.n, p, k) and V.dtype == np.float32 and ev.shape == (case.n, k) and tv2.shape == (case.n,)
    lam, vec = spectrum(cov)
    lam1 = np.maximum(lam[:, 0], 0.0)
    tol = 1e-12 * p * lam1 + p * ref.bound.reshape(case.n, -1).max(1)
    assert np.all(np.abs(ev - np.maximum(lam[:, :k], 0.0)) <= tol[:, None]), np.abs(ev - np.maximum(lam[:, :k], 0.0)).max()
    assert np.all(np.abs(tv2 - tv) <= np.einsum("iaa->i", ref.bound))
    assert np.all(np.diff(ev, axis=1) <= 0) and np.all(ev >= 0)
    orth = np.einsum("npk,npl->nkl", V.astype(np.float64), V.astype(np.float64))
    assert np.abs(orth - np.eye(k)).max() < 1e-5
    if case.zero:
        assert np.all(ev == 0.0) and np.array_equal(V, np.broadcast_to(np.eye(p, k, dtype=np.float32), V.shape))
    else:
        gwp.check_parity(ev, V, tv2, lam, vec[:, :, :k], tv, k)
    return st


def upload(ctx, case):
    from xeofs_amd import engine

    mat = engine.from_dense(ctx, case.X)
    assert (mat.n, mat.p) == (case.n, case.p)
    return mat


# ------------------------------------------------------------------------------------------------ covariance
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_covariance(ctx, case):
    import torch

    from xeofs_amd import _lib, engine

    mat = upload(ctx, case)
    try:
        assert np.array_equal(mat.download(), case.X)              # the reference's rows are the engine's own
        cov_t, cov, tv, st = run_cov(ctx, mat, case)
        assert cov.shape == (case.count, case.p, case.p) and tv.shape == (case.count,)
        check_covariance(case, cov, tv)
        check_invariants(case, cov, tv)
        _, cov2, tv2, _ = run_cov(ctx, mat, case)
        assert np.array_equal(cov, cov2) and np.array_equal(tv, tv2)
        assert st["tiles"] == -(-case.count // GW_T) and st["chunks"] == 1
        if case.name == "geometry-grid-alone":
            assert st["tile_pairs_visited"] == st["tiles"] == 4
        if case.group == "ranges":                                  # nothing written past `count` rows
            big = torch.full((case.count + 2, case.p, case.p), -7.5, dtype=torch.float64, device=cov_t.device)
            tbig = torch.full((case.count + 2,), -7.5, dtype=torch.float64, device=cov_t.device)
            rc = ctx.lib.eofx_gw_cov_f64(ctx.handle, mat.handle, case.xy.ctypes.data, engine.GW_METRICS[case.metric],
                                         engine.GW_KERNELS[case.kernel], case.bw, case.first, case.count, _lib.ptr(big),
                                         _lib.ptr(tbig), None)
            assert rc == _lib.EOFX_OK
            torch.cuda.synchronize()
            big, tbig = big.cpu().numpy(), tbig.cpu().numpy()
            assert np.array_equal(big[:case.count], cov) and np.array_equal(tbig[:case.count], tv)
            assert np.all(big[case.count:] == -7.5) and np.all(tbig[case.count:] == -7.5)
        if case.p <= 64 and case.count == case.n:
            w, V = ctx_syev(ctx, cov_t, case.p)
            for i in range(case.n):
                check_syev(cov[i], w[i], V[i], case.p)
            check_gwpca(ctx, mat, case, cov, tv, min(case.p, 3))
    finally:
        mat.free()


def ctx_syev(ctx, A, k):
    from xeofs_amd import engine

    w, V = engine.batched_syev(ctx, A, k)
    return w.cpu().numpy(), V.cpu().numpy()


@pytest.mark.parametrize("p", GWPCA_P + [65])
def test_gwpca_three_chunks(ctx, p):
    """k = 1 and k = p in chunks of 16 sorted positions (three chunks, the last with 8 locations): float32 components and
    out_index at every feature count where the eigen route changes (p = 65: the library eigensolver, chunks of gw_cov)"""
    case = CASE[f"features-p{p}"]
    assert case.n == 40
    mat = upload(ctx, case)
    try:
        _, cov, tv, _ = run_cov(ctx, mat, case)
        for k in sorted({1, p}):
            st = check_gwpca(ctx, mat, case, cov, tv, k, chunk=16)
            assert st["chunks"] == 3
    finally:
        mat.free()


# ------------------------------------------------------------------------------------------------ the eigensolver
SYEV_P = [3, 31, 32, 33, 63]


def rotation(p, rng):
    Q, _ = np.linalg.qr(rng.normal(size=(p, p)))
    return Q


def syev_matrix(kind, p):
    rng = np.random.default_rng(1000 + p)
    Q = rotation(p, rng)
    if kind == "spd":
        B = rng.normal(size=(p, p))
        A = B @ B.T + 0.1 * np.eye(p)
    elif kind == "graded":              # 14 orders of magnitude
        A = (Q * 10.0 ** (-14.0 * np.arange(p) / (p - 1))) @ Q.T
    elif kind == "pairs":               # lambda (1 +- 1e-10): clusters of two (and a single value when p is odd)
        lam = np.repeat(np.linspace(3.0, 1.0, (p + 1) // 2), 2)[:p] * (1.0 + 1e-10 * (-1.0) ** np.arange(p))
        A = (Q * lam) @ Q.T
    else:
        assert kind == "indefinite"
        A = (Q * np.linspace(2.0, -1.5, p)) @ Q.T
    return (A + A.T) / 2


@pytest.mark.parametrize("p", SYEV_P)
@pytest.mark.parametrize("kind", ["spd", "graded", "pairs", "indefinite"])
def test_batched_syev_edges(ctx, kind, p):
    import torch

    A = syev_matrix(kind, p)
    if kind == "indefinite":
        assert (np.linalg.eigvalsh(A) < -0.1).sum() >= p // 3
    batch = torch.as_tensor(np.stack([A, 0.5 * A, A]), device="cuda")
    full = None
    for k in sorted({1, p - 1, p}):
        w, V = ctx_syev(ctx, batch, k)
        assert w.shape == (3, k) and V.shape == (3, p, k)
        check_syev(A, w[0], V[0], k)
        check_syev(0.5 * A, w[1], V[1], k)
        assert np.array_equal(w[0], w[2]) and np.array_equal(V[0], V[2])
        if k == p:
            full = w, V
    for k in sorted({1, p - 1}):        # k < p: the leading columns of the full answer, bit for bit
        w, V = ctx_syev(ctx, batch, k)
        assert np.array_equal(w, full[0][:, :k]) and np.array_equal(V, full[1][:, :, :k])


@pytest.mark.parametrize("p", SYEV_P)
def test_batched_syev_nan_matrix_stays_alone(ctx, p):
    """{A, NaN, A}: one workgroup per matrix, so the clean rows are the clean batch's bit for bit; the NaN row is NaN (the
    loop is bounded by max_sweeps)"""
    import torch

    A = syev_matrix("spd", p)
    clean = ctx_syev(ctx, torch.as_tensor(np.stack([A, A, A]), device="cuda"), p)
    w, V = ctx_syev(ctx, torch.as_tensor(np.stack([A, np.full((p, p), np.nan), A]), device="cuda"), p)
    for b in (0, 2):
        assert np.array_equal(w[b], clean[0][b]) and np.array_equal(V[b], clean[1][b])
    assert np.isnan(w[1]).all() and np.isnan(V[1]).all()


@pytest.mark.parametrize("p", SYEV_P)
def test_batched_syev_power_of_two_scaling(ctx, p):
    """2^300 A and 2^-300 A: every operation of the sweep scales exactly (no square leaves the normal range: the smallest
    off-diagonal entries the loop sees before it ends are 1e-40 of the largest, 2^-866 after squaring at 2^-300)"""
    import torch

    A = syev_matrix("spd", p)
    s = 2.0 ** 300
    w, V = ctx_syev(ctx, torch.as_tensor(np.stack([A, s * A, A / s]), device="cuda"), p)
    check_syev(A, w[0], V[0], p)
    assert np.array_equal(w[1], s * w[0]) and np.array_equal(w[2], w[0] / s)
    assert np.array_equal(V[1], V[0]) and np.array_equal(V[2], V[0])
