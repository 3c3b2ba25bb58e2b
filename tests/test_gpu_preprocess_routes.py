"""The preprocessing statistics (Scaler + Sanitizer), route by route and FEATURE BY FEATURE against a two-pass reference.

reference     `reference()` below: numpy, np.longdouble, two passes over the float32 field (mean, then the squares of the
              deviations).  Never another path of the engine, never a max-norm over the features.
routes        `colstats_plan`, `summary_blocks`, `apply_plan`, `fit_plan` restate the choices of run_colstats,
              run_feature_summary, sanitize_and_apply and the fused fit (the plans of the same names and atb_plan in
              csrc/eofx_plans.hpp; tests/test_plans_cpu.py compares them with the header itself).  They only choose shapes
              and say which layout a case must end in; tests/test_preprocess_model_host.py proves without a GPU that CASES,
              FIT_CASES and RESAMPLE_CASES reach every route listed there.

Error model (u = 2^-53, e = 2^-24 the unit roundoff of float32, k valid samples of the feature; a = mean |x|,
q2 = mean x^2, M2 = sum (x - mean)^2 -- all from the reference).  MARGIN = 2 on every statistics term: it covers the
difference between the association the bound was derived for and the one a kernel uses (the transposing kernel adds 16 row
groups, the splits are added in order).

two-step path (colstats_shift_kernel, colstats*_kernel, colstats_finalize_kernel: one pass of float64 sums about a
    provisional shift c -- the first finite value among nine probe rows --, d = x - c, s = sum d, q = sum d^2,
    mean = c + s / k, M2 = q - s (s / k))
    d carries one rounding, a float64 sum of k terms at most (k - 1) u sum|t|, the quotient and the final sum one each, and
    the reference's own cast to float64 half of one:
        |mean - ref|  <= (k + 2) u mean|x - c| + 2 u |mean|
    q: d^2 carries 3 u (two from d, one of its own) and the sum k - 1: (k + 2) u sum d^2; s (s / k): (2 k + 2) u s^2 / k, and
    s^2 / k <= sum d^2; the difference one more:
        |M2 - ref|    <= 3 (k + 2) u sum (x - c)^2
    This is the issue's one-pass model 2 (k + 4) u k q2 with the second moment taken about c instead of 0: the term
    |mean|^2 / var of the unshifted sums is gone (sum (x - c)^2 = M2 + k (mean - c)^2, and c is a sample of the feature).
    The test asserts it in the form that stays meaningful when var -> 0 (constant features):
        sqrt(max(M2 - B, 0) / k) <= std <= sqrt((M2 + B) / k),  both ends clipped at float32 eps like the reference's std,
    with B = MARGIN * 3 (k + 2) u sum (x - c)^2 and 4 u of slack for the division and the root.
fused fit (eofx_fit.hpp; c = the float32 mean of nine probe rows, v = (x - c) a_scale one fused multiply-add)
    S1 = sum (x - c) is the ones column of the split-fp16 matrix product: v carries e, its two-term fp16 split 4 e
    (2^-22), the float32 accumulator of a split at most one rounding per row (r rows per split):
        |mean - ref|  <= (5 + r) e mean|x - c|                                   (+ the float64 terms above, negligible)
    q = sum v^2: v^2 carries 2 e from v and e of its own, a float32 partial sum of FIT_FLUSH slabs (128 terms) 128 e
    before it moves to float64; the re-read last row is subtracted with the kernel's own expression:
        |q / a^2 - sum (x - c)^2| <= 131 e sum (x - c)^2
        |M2 - ref|    <= 131 e sum (x - c)^2 + (2 |S1| dS1 + dS1^2) / k,   dS1 = (5 + r) e sum|x - c|
matrix elements (aff_split / aff_map, csrc/eofx_kernels.hpp: ((x - hi) - lo) * (float) scale with hi + lo the float pair
    of the float64 shift): hi = fl(sh) and lo = fl(sh - hi) leave |sh - hi - lo| <= 2^-48 |sh|; fl(x - hi) is off by
    e |x - hi| <= e |x - sh| + 2^-48 |sh|; the second subtraction, the cast of the scale and the product one e each:
        |y - (x - sh) sc| <= 5 e |(x - sh) sc| + 2^-47 |sh| |sc|                 (4 roundings, 5 with the second order)
    and the statistics propagate through (x - mean) * scale:  + dmean |sc| + |y| dstd / std.
norms         | ||a|| - ||b|| | <= ||a - b||: the 2-norm of the element bounds of the column (row), plus (k + 2) u of its own.
total variance  sum_c scale_c^2 M2_c / (k - 1): the interval the bounds on M2 and std leave, summed over the features.
Hilbert stage  its own arithmetic is not the subject here: 2e-5 per element (the figure test_hilbert_stage_vs_oracle uses)
              times the larger of max|x + i H x| and max|x| of the field that enters -- a float32 transform errs in
              proportion to its INPUT, and an uncentred standardised field enters with its offset (hundreds) while the
              oracle's analytic signal is re-centred (units); a wrong sample-contiguous raw copy (colstats_tr_kernel's Xt) is
              wrong by whole values.

The cancellation family (|mean| / std = R up to 1e6, n up to 60000) asserts this model AND the 2e-6 the suite promises
elsewhere for std on all four ratios and both paths.  Summed about 0 (the code before this file existed) the two-step path
measured 8e-7 at R = 3e4 and 9e-4 at R = 1e6.  Every case prints error / bound.

A device field 4 bytes off a 16-byte boundary is NOT copied by the wrapper: run_colstats takes the one-feature-per-thread
kernel, sanitize_and_apply the written layouts through apply_kernel<false> (raw and in-place requests fall back).
"""

import zlib
from collections import namedtuple

import numpy as np
import pytest

from test_gpu_product_routes import ATB_BM, ATB_KG, _up, atb_splits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
E32 = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 2.0
FIT_FLUSH = 16            # csrc/eofx_fit.hpp
FLUSH_ROWS = FIT_FLUSH * 16
LD = np.longdouble


# --------------------------------------------------------------------------- #
# the routes, restated                                                          #
# --------------------------------------------------------------------------- #
def colstats_plan(n, P, aligned=True, ld=None, sample_raw=False, row_map=False):
    """run_colstats -> dict(kernel 'scalar' | 'vec4' | 'tr', RS, rps, last (rows of the last split))"""
    ld = ld or P
    vec4 = P % 4 == 0 and ld % 4 == 0 and aligned
    gxs = (P + 255) // 256
    gx = (P // 4 + 255) // 256 if vec4 else gxs
    RS = max(1, (2048 + gx - 1) // gx)
    RS = min(RS, max(1, n // 64))
    rps = (n + RS - 1) // RS
    if sample_raw and not row_map:
        rps = _up(rps, 64)
    RS = (n + rps - 1) // rps
    tr = vec4 and sample_raw and not row_map and _up(n, ATB_BM) <= 8192 and rps % 64 == 0
    return dict(kernel="tr" if tr else "vec4" if vec4 else "scalar", RS=RS, rps=rps, last=n - (RS - 1) * rps)


def summary_blocks(P):
    """workgroups of feature_summary_kernel"""
    return max(1, min((P + 4095) // 4096, 256))


def apply_plan(n, P, pv, ns, mode, aligned=True):
    """sanitize_and_apply -> dict(layout 'written' | 'raw' | 'in_place' | 'masked', apply 'scalar' | 'vec' | None)
    mode: the layout asked for (0 written, 1 keep_raw, 2 in_place, 3 in_place + allow_masked)"""
    raw_ok = mode >= 1 and ns == n and P % 4 == 0 and aligned
    masked = raw_ok and mode == 3 and pv < P and 10 * pv >= 6 * P and n < pv
    raw_mode = (raw_ok and pv == P) or masked
    if raw_mode and mode >= 2:
        return dict(layout="masked" if masked else "in_place", apply=None)
    if raw_mode:
        return dict(layout="raw", apply="vec")
    return dict(layout="written", apply="vec" if pv == P and P % 4 == 0 and aligned else "scalar")


def fit_plan(n, P, l):
    """the statistics-carrying first pass -> dict(NB, S, kps (rows per split), extra (re-read last rows))"""
    assert n < P and 0 < l < n and l % 32 != 0 and _up(l, 32) <= 64 and P % 4 == 0       # fit_first_eligible
    L, K = _up(l, 32), _up(n, ATB_KG)
    S = atb_splits(_up(P, ATB_BM), K, L, False)
    return dict(NB=L // 32, S=S, kps=_up((K + S - 1) // S, ATB_KG), extra=K - n)


# --------------------------------------------------------------------------- #
# cases                                                                         #
# --------------------------------------------------------------------------- #
# family: noise | nan_lo (all-NaN features, < 40 %) | nan_hi (> 40 %) | missing (all-NaN samples + a few all-NaN features)
#         | const | weights;  mode: see apply_plan;  inp: host | device | misaligned;  hilbert: the sample-raw statistics pass
Case = namedtuple("Case", "id n P family mode inp hilbert", defaults=(False,))
CASES = [
    Case("scalar_rs1_tiny", 2, 3, "noise", 0, "host"),
    Case("scalar_rs1_n63", 63, 126, "noise", 0, "device"),
    Case("scalar_rs1_n64", 64, 5, "noise", 1, "host"),               # P % 4 != 0: the raw request falls back
    Case("scalar_rs1_n65_nb2", 65, 4099, "nan_lo", 0, "host"),
    Case("scalar_split", 1000, 1001, "noise", 0, "device"),
    Case("scalar_split_missing", 1000, 1001, "missing", 0, "host"),
    Case("scalar_misaligned", 300, 128, "noise", 2, "misaligned"),
    Case("vec4_rs1_p4", 2, 4, "noise", 0, "host"),
    Case("vec4_rs1_raw", 63, 128, "noise", 1, "device"),
    Case("vec4_rs1_const", 120, 64, "const", 0, "host"),
    Case("vec4_rs1_weights", 120, 260, "weights", 2, "host"),
    Case("vec4_split", 5000, 260, "noise", 0, "host"),
    Case("vec4_split_in_place", 5000, 260, "noise", 2, "device"),
    Case("vec4_split_missing", 5000, 260, "missing", 2, "host"),       # missing samples: the in-place request falls back
    Case("vec4_nb3_compact", 130, 8200, "nan_lo", 0, "host"),
    Case("vec4_nb3_masked", 130, 8200, "nan_lo", 3, "device"),
    Case("vec4_masked", 100, 1300, "nan_lo", 3, "host"),
    Case("vec4_masked_falls_back", 100, 1300, "nan_hi", 3, "host"),
    Case("vec4_compact_hi", 100, 1300, "nan_hi", 0, "device"),
    Case("tr_rs1", 100, 200, "noise", 2, "host", True),
    Case("tr_split", 700, 1300, "noise", 2, "device", True),
    Case("tr_split_weights", 700, 1300, "weights", 2, "host", True),
]
# (center, standardize, weights): each of the three on and off
OPTS = [(True, False, False), (True, True, True), (False, True, False), (False, False, True)]

# the one-call fit: (id, n, P, k, n_oversamples)
FitCase = namedtuple("FitCase", "id n P k over std")
FIT_CASES = [
    FitCase("nb1_short", 120, 132, 6, 10, False),         # n below one flush, 8 re-read rows
    FitCase("nb1_short_std", 120, 132, 6, 10, True),
    FitCase("nb2_mid", 1000, 1028, 8, 32, False),         # NB = 2, 24 re-read rows
    FitCase("nb2_mid_std", 1000, 1028, 8, 32, True),
    FitCase("nb1_long", 6000, 12000, 6, 10, False),       # 288 rows per split: more than FLUSH_ROWS, two float64 flushes
    FitCase("nb2_long_std", 6000, 12000, 20, 20, True),
]

# resample: (id, n, P, n_rows)
ResCase = namedtuple("ResCase", "id n P n_rows")
RESAMPLE_CASES = [
    ResCase("vec4_rs1", 90, 64, 100),
    ResCase("scalar_rs1", 90, 61, 63),
    ResCase("vec4_split", 400, 260, 1000),
    ResCase("scalar_split", 400, 1001, 333),
]

CANCEL_RATIOS = (30.0, 1e3, 3e4, 1e6)
CANCEL_N = (120, 5000, 60000)
CANCEL_P = 16                  # two-step: four features per ratio
CANCEL_FUSED_N = (120, 5000)   # the fused pass needs n < P: (120, 128) and (5000, 5004)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def dead_features(case):
    """all-NaN features: the first, the last, runs across the 4-, 64-, 256- and 512-feature boundaries, two singles"""
    P = case.P
    if case.family == "missing":
        return np.array(sorted({0, P - 1, 130, 131} & set(range(P))))
    if case.family not in ("nan_lo", "nan_hi"):
        return np.zeros(0, np.int64)
    dead = {0, P - 1, 9, 37}
    for b in (4, 64, 256, 512, 4096):
        if b + 2 < P:
            dead.update(range(b - 2, b + 2))
    if case.family == "nan_hi":
        dead.update(range(P // 3, P // 3 + P // 2))
    return np.array(sorted(d for d in dead if d < P))


def missing_rows(case):
    """all-NaN samples: the first row, the last row, and every row of the second row split"""
    if case.family != "missing":
        return np.zeros(0, np.int64)
    plan = colstats_plan(case.n, case.P, case.inp != "misaligned", sample_raw=case.hilbert)
    run = range(plan["rps"], min(2 * plan["rps"], case.n - 1)) if plan["RS"] > 2 else range(0)
    return np.array(sorted({0, case.n - 1} | set(run)))


def case_weights(case, use_w):
    if case.family == "weights":          # exact zeros, five decades
        rng = _rng(case.id + "w")
        w = 10.0 ** rng.uniform(-3, 2, case.P)
        w[::5] = 0.0
        return w
    return _rng(case.id + "w").uniform(0.3, 1.5, case.P) if use_w else None


def make_field(case):
    rng = _rng(case.id)
    n, P = case.n, case.P
    X = rng.standard_normal((n, P)) * rng.uniform(0.5, 3.0, P) + rng.uniform(-50.0, 300.0, P)
    X = X.astype(np.float32)
    if case.family == "const":
        X[:, 1::7] = 3.5
        X[:, 2::7] = 0.0
        X[:, 3::7] = np.float32(3.7)      # 24 significant bits: the one-pass sums round
        X[:, 5::7] = -2.0
    dead, rows = dead_features(case), missing_rows(case)
    if dead.size:
        X[:, dead] = np.nan
    if rows.size:
        X[rows] = np.nan
    return X


def cancel_field(n, P, seed):
    """feature j: unit-variance noise around an offset of CANCEL_RATIOS[j % 4] (as float32 holds it)"""
    rng = np.random.default_rng(seed)
    R = np.array([CANCEL_RATIOS[j % 4] for j in range(P)])
    X = (rng.standard_normal((n, P)) + R * np.where(np.arange(P) % 8 < 4, 1.0, -1.0)).astype(np.float32)
    return X, R


# --------------------------------------------------------------------------- #
# reference and bounds                                                          #
# --------------------------------------------------------------------------- #
def reference(X32, center, standardize, w):
    """two passes in np.longdouble over the float32 field -> dict; per-feature arrays have length P (NaN where invalid)"""
    n, P = X32.shape
    nan = np.isnan(X32)
    vf = ~nan.all(0)
    vs = ~nan[:, vf].all(1)
    Xv = X32[vs][:, vf].astype(LD)
    assert not np.isnan(Xv).any()          # the families hold whole features and whole samples only
    k = int(vs.sum())
    mean = Xv.sum(0) / k
    d = Xv - mean
    M2 = (d * d).sum(0) - d.sum(0) ** 2 / k          # (corrected two-pass)
    std = np.maximum(np.sqrt(M2 / k), LD(EPS32))
    wv = (np.ones(P) if w is None else np.asarray(w, np.float64))[vf].astype(LD)
    shift = mean if center else np.zeros_like(mean)
    scale = (1 / std if standardize else np.ones_like(std)) * wv
    Y = (Xv - shift) * scale
    full = lambda a: np.where(vf, 0, np.nan) + np.bincount(np.flatnonzero(vf), np.asarray(a, np.float64), P)
    return dict(k=k, vf=vf, vs=vs, mean=np.asarray(mean, np.float64), M2=np.asarray(M2, np.float64),
                std=np.asarray(std, np.float64), shift=np.asarray(shift, np.float64), scale=np.asarray(scale, np.float64),
                Y=np.asarray(Y, np.float64), a=np.asarray(np.abs(Xv).mean(0), np.float64),
                q2=np.asarray((Xv * Xv).mean(0), np.float64), Xv=Xv, w=np.asarray(wv, np.float64),
                mean_full=full(mean), c=stats_shift(X32)[vf], tv=float((scale * scale * M2).sum() / max(k - 1, 1)))


def stats_shift(X32):
    """colstats_shift_kernel: per feature the first finite value among the nine probe rows (0 if there is none)"""
    n = X32.shape[0]
    c = np.zeros(X32.shape[1], np.float32)
    todo = np.ones(X32.shape[1], bool)
    for r in [n - 1 if t == 8 else (n * t) // 8 for t in range(9)]:
        take = todo & np.isfinite(X32[r])
        c[take] = X32[r, take]
        todo &= ~take
    return c


def two_step_bounds(ref):
    """(dmean, dM2) of the one-pass float64 statistics about the provisional shift, without MARGIN"""
    k = ref["k"]
    d = ref["Xv"] - ref["c"].astype(LD)
    return ((k + 2) * U * np.asarray(np.abs(d).mean(0), np.float64) + 2 * U * np.abs(ref["mean"]),
            3 * (k + 2) * U * np.asarray((d * d).sum(0), np.float64))


def fused_bounds(ref, cshift, rows_per_split):
    """(dmean, dM2) of the statistics of the fused first pass, without MARGIN; cshift: the float32 probe means"""
    k = ref["k"]
    d = ref["Xv"] - cshift.astype(LD)
    sabs, ssq, s1 = (np.asarray(v, np.float64) for v in (np.abs(d).sum(0), (d * d).sum(0), d.sum(0)))
    dS1 = (5 + rows_per_split) * E32 * sabs
    dm2 = 131 * E32 * ssq + (2 * np.abs(s1) * dS1 + dS1 * dS1) / k
    dmean, dM2 = two_step_bounds(ref)
    return dS1 / k + dmean, dm2 + dM2 * 1e-3      # (the float64 steps of fit_finalize_kernel: a handful of roundings)


def probe_shift(X32):
    """fit_probe_kernel: the float32 mean of nine rows, summed in order and multiplied by float32(1/9)"""
    n = X32.shape[0]
    rows = [n - 1 if t == 8 else (n * t) // 8 for t in range(9)]
    c = np.zeros(X32.shape[1], np.float32)
    for r in rows:
        c = (c + X32[r]).astype(np.float32)
    return (c * np.float32(1.0 / 9.0)).astype(np.float32)


def std_interval(ref, dM2):
    """[lo, hi] the model leaves for std, both clipped at float32 eps"""
    k, B = ref["k"], MARGIN * dM2
    lo = np.maximum(np.sqrt(np.maximum(ref["M2"] - B, 0.0) / k) * (1 - 4 * U), EPS32)
    hi = np.maximum(np.sqrt((ref["M2"] + B) / k) * (1 + 4 * U), EPS32)
    return lo, hi


def element_bound(ref, dmean, dM2, center, standardize):
    """per-element bound on the matrix against ref['Y']"""
    sc = np.abs(ref["scale"])
    Y = np.abs(ref["Y"])
    b = 5 * E32 * Y + 2.0 ** -47 * np.abs(ref["shift"]) * sc
    if center:
        b = b + MARGIN * dmean * sc
    if standardize:
        lo, hi = std_interval(ref, dM2)
        rel = np.maximum(hi / ref["std"], ref["std"] / lo) - 1.0
        b = b + Y * rel * (1 + 5 * E32)
    return b


def tv_interval(ref, dM2, standardize):
    k, B = ref["k"], MARGIN * dM2
    m_lo, m_hi = np.maximum(ref["M2"] - B, 0.0), ref["M2"] + B
    if standardize:
        s_lo, s_hi = std_interval(ref, dM2)
        lo, hi = ref["w"] ** 2 * m_lo / s_hi ** 2, ref["w"] ** 2 * m_hi / s_lo ** 2
    else:
        lo, hi = ref["w"] ** 2 * m_lo, ref["w"] ** 2 * m_hi
    slack = (lo.size + 8) * U
    return lo.sum() / (k - 1) * (1 - slack), hi.sum() / (k - 1) * (1 + slack)


def _ratio(key, err, bound):
    """largest error / bound; every figure is printed (they feed the table of DESIGN.md section 2a)"""
    r = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if np.size(err) else 0.0
    print(f"RATIO {key[0]} {key[1]} {key[2]} {r:.3g}")
    return r


def check_stats(tag, name, st, ref, dmean, dM2, standardize, n_total=None):
    """every statistic of the `stats` dict against the reference, per feature"""
    vf = ref["vf"]
    assert np.array_equal(st["valid_feature"], vf)
    assert np.array_equal(st["valid_sample"], ref["vs"])
    assert st["n"] == ref["k"] and st["p"] == int(vf.sum())
    assert np.isnan(st["mean"][~vf]).all() and np.isnan(st["std"][~vf]).all()
    r = _ratio((tag, name, "mean"), np.abs(st["mean"][vf] - ref["mean"]), MARGIN * dmean)
    assert r <= 1.0, (name, "mean", r)
    lo, hi = std_interval(ref, dM2)
    sd = st["std"][vf]
    half = np.maximum(hi - ref["std"], ref["std"] - lo)
    r = _ratio((tag, name, "std"), np.abs(sd - ref["std"]), half)
    assert np.all((sd >= lo) & (sd <= hi)), (name, "std", r)
    if ref["k"] > 1:
        t_lo, t_hi = tv_interval(ref, dM2, standardize)
        tv = st["total_variance"]
        _ratio((tag, name, "tv"), np.abs(tv - ref["tv"]), max(t_hi - ref["tv"], ref["tv"] - t_lo, 0.0))
        assert t_lo <= tv <= t_hi, (name, "total_variance", tv, t_lo, t_hi)


def check_matrix(ctx, tag, name, mat, ref, bound):
    """download, feature norms and sample norms of a resident matrix against ref['Y'], per element"""
    from xeofs_amd import engine

    D = mat.download()
    assert D.shape == ref["Y"].shape, (D.shape, ref["Y"].shape)
    r = _ratio((tag, name, "matrix"), np.abs(D.astype(np.float64) - ref["Y"]), bound)
    assert r <= 1.0, (name, "matrix", r)
    for what, axis, got in (("feature_norms", 0, engine.feature_norms(ctx, mat)), ("sample_norms", 1, engine.sample_norms(ctx, mat))):
        nr = np.sqrt((ref["Y"] ** 2).sum(axis))
        nb = np.sqrt((bound ** 2).sum(axis)) + (ref["Y"].shape[axis] + 2) * U * nr
        r = _ratio((tag, name, what), np.abs(got - nr), nb)
        assert got.shape == nr.shape and r <= 1.0, (name, what, r)
    return D


def as_input(X, inp):
    """host array, device tensor, or a contiguous device view 4 bytes off a 16-byte boundary"""
    if inp == "host":
        return X
    import torch

    if inp == "device":
        return torch.from_numpy(X).cuda()
    buf = torch.empty(X.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(X.shape)
    view.copy_(torch.from_numpy(X))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _layout_kw(mode):
    return dict(keep_raw=mode == 1, in_place=mode >= 2, allow_masked=mode == 3)


def _same_stats(a, b):
    return all(np.array_equal(a[key], b[key], equal_nan=True) for key in ("mean", "std", "valid_feature", "valid_sample")) and \
        (a["total_variance"] == b["total_variance"] or (np.isnan(a["total_variance"]) and np.isnan(b["total_variance"])))


# --------------------------------------------------------------------------- #
# tests                                                                         #
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "c%d_s%d_w%d" % tuple(int(v) for v in o))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_preprocess_route(ctx, case, opts):
    from oracle import eof_oracle as orc
    from xeofs_amd import engine

    center, standardize, use_w = opts
    X = make_field(case)
    w = case_weights(case, use_w)
    ref = reference(X, center, standardize, w)
    dmean, dM2 = two_step_bounds(ref)
    Xin = as_input(X, case.inp)
    name = f"{case.id}/c{int(center)}s{int(standardize)}w{int(w is not None)}"
    mat, st = engine.preprocess(ctx, Xin, center, standardize, w, **_layout_kw(case.mode))
    check_stats("preprocess", name, st, ref, dmean, dM2, standardize)
    plan = apply_plan(case.n, case.P, int(ref["vf"].sum()), ref["k"], case.mode, case.inp != "misaligned")
    has_x, has_raw = mat.layout()
    assert mat.masked == (plan["layout"] == "masked")
    assert has_raw == (plan["layout"] != "written") and has_x == (plan["layout"] == "written")
    assert mat.has_sample_layout() == (plan["layout"] in ("written", "raw"))
    assert mat.shape == ref["Y"].shape
    bound = element_bound(ref, dmean, dM2, center, standardize)
    D = check_matrix(ctx, "preprocess", name, mat, ref, bound)
    if case.family == "const" and center:
        const = np.isin(np.arange(case.P) % 7, (1, 2, 3, 5))
        assert np.all(D[:, const] == 0.0)                      # x - mean is exact for a constant feature
        if standardize:
            assert np.all(st["std"][const] == EPS32)           # the sums about the shift are exact zeros: std clips
    mat.free()
    # the same call again: bit-identical statistics; on the sample-raw route the Hilbert stage follows at once and reads
    # the raw copy the statistics pass wrote
    mat2, st2 = engine.preprocess(ctx, Xin, center, standardize, w, for_hilbert=case.hilbert, **_layout_kw(case.mode))
    if case.hilbert:
        assert colstats_plan(case.n, case.P, sample_raw=True)["kernel"] == "tr"
        check_stats("preprocess_tr", name, st2, ref, dmean, dM2, standardize)
        B, _ = engine.hilbert(ctx, mat2, "exp", 0.2)
        href = orc.hilbert_transform(ref["Y"], padding="exp", decay_factor=0.2)
        r = _ratio(("preprocess_tr", name, "hilbert"), np.abs(B.download() - href.imag), np.full(href.shape, 2e-5 * max(np.abs(href).max(), np.abs(ref["Y"]).max())))
        assert r <= 1.0, (name, "hilbert", r)
        B.free()
        mat3, st4 = engine.preprocess(ctx, Xin, center, standardize, w, for_hilbert=True, **_layout_kw(case.mode))
        assert _same_stats(st2, st4)
        mat3.free()
    else:
        assert _same_stats(st, st2)
    mat2.free()


def test_single_sample_is_rejected_when_centred(ctx):
    """n = 1: the variance with ddof = 1 does not exist.  The engine stops a centred or standardised fit with a ValueError --
    its total variance is 0 / 0, which sanitize_and_apply treats like an infinity in the field; the reference itself would go
    on with a NaN total variance, so only the exception type is pinned.  The plain map goes through, with NaN as its total
    variance."""
    from xeofs_amd import engine

    X = np.arange(1, 9, dtype=np.float32)[None, :]
    with pytest.raises(ValueError):
        engine.preprocess(ctx, X, True, False)
    w = np.linspace(0.5, 2.0, 8)
    mat, st = engine.preprocess(ctx, X, False, False, w)
    assert np.array_equal(st["mean"], X[0].astype(np.float64)) and np.all(st["std"] == EPS32)
    assert st["n"] == 1 and st["p"] == 8 and np.isnan(st["total_variance"])
    ref = X.astype(np.float64) * w
    assert np.all(np.abs(mat.download() - ref) <= 5 * E32 * np.abs(ref))
    mat.free()


@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: c.id)
def test_fused_fit_statistics(ctx, case):
    from xeofs_amd import engine

    rng = _rng(case.id)
    n, P, standardize = case.n, case.P, case.std
    X = (rng.standard_normal((n, P)) * rng.uniform(0.5, 3.0, P) + rng.uniform(-50.0, 300.0, P)).astype(np.float32)
    w = rng.uniform(0.3, 1.5, P) if standardize else None
    plan = fit_plan(n, P, case.k + case.over)
    ref = reference(X, True, standardize, w)
    dmean, dM2 = fused_bounds(ref, probe_shift(X), plan["kps"])
    name = case.id
    runs = []
    for _ in range(2):
        mat, st, Us, s, V = engine.fit(ctx, X, case.k, True, standardize, w, n_oversamples=case.over, random_state=5)
        assert st["fused"], engine.fit_info(ctx)
        runs.append(st)
        if len(runs) == 1:
            check_stats("fit", name, st, ref, dmean, dM2, standardize)
            check_matrix(ctx, "fit", name, mat, ref, element_bound(ref, dmean, dM2, True, standardize))
        mat.free()
    assert _same_stats(runs[0], runs[1])


@pytest.mark.parametrize("n", CANCEL_N)
def test_cancellation_two_step(ctx, n):
    """|mean| / std in CANCEL_RATIOS through the one-pass float64 sums about the provisional shift: the model per feature and
    the 2e-6 on std, on all four ratios"""
    from xeofs_amd import engine

    for P, inp in ((CANCEL_P, "host"), (CANCEL_P - 1, "device")):      # vec4 and scalar kernels
        X, R = cancel_field(n, P, seed=n + P)
        ref = reference(X, True, True, None)
        dmean, dM2 = two_step_bounds(ref)
        mat, st = engine.preprocess(ctx, as_input(X, inp), True, True, None)
        for ratio in CANCEL_RATIOS:
            sel = R == ratio
            rel = np.abs(st["std"][sel] - ref["std"][sel]) / ref["std"][sel]
            lo, hi = std_interval(ref, dM2)
            print(f"CANCEL two_step n={n} P={P} R={ratio:g} std_rel_err={rel.max():.3g} model_rel={((hi - lo) / 2 / ref['std'])[sel].max():.3g}")
            assert rel.max() <= 2e-6, (n, ratio, rel.max())
        name = f"n{n}_P{P}"
        check_stats("cancel_two_step", name, st, ref, dmean, dM2, True)
        check_matrix(ctx, "cancel_two_step", name, mat, ref, element_bound(ref, dmean, dM2, True, True))
        mat.free()


@pytest.mark.parametrize("n", CANCEL_FUSED_N)
def test_cancellation_fused(ctx, n):
    """the same offsets through the one-call fit, which must stay fused: its provisional shift removes the cancellation"""
    from xeofs_amd import engine

    P = _up(n + 4, 4)
    X, R = cancel_field(n, P, seed=n)
    ref = reference(X, True, False, None)
    mat, st, Us, s, V = engine.fit(ctx, X, 6, True, False, None, random_state=5)
    assert st["fused"], engine.fit_info(ctx)
    dmean, dM2 = fused_bounds(ref, probe_shift(X), fit_plan(n, P, 16)["kps"])
    for ratio in CANCEL_RATIOS:
        sel = R == ratio
        rel = np.abs(st["std"][sel] - ref["std"][sel]) / ref["std"][sel]
        print(f"CANCEL fit fused={st['fused']} n={n} R={ratio:g} std_rel_err={rel.max():.3g}")
        assert rel.max() <= 2e-6, (n, ratio, rel.max())
    check_stats("cancel_fit", f"n{n}", st, ref, dmean, dM2, False)
    check_matrix(ctx, "cancel_fit", f"n{n}", mat, ref, element_bound(ref, dmean, dM2, True, False))
    mat.free()


APPLY_CASES = [("compact", 150, 1001, "nan_lo", 0), ("vector", 150, 260, "noise", 0), ("masked", 100, 1300, "nan_lo", 3),
               ("in_place", 150, 260, "noise", 2)]


@pytest.mark.parametrize("wscale", [1e-3, 1e3], ids=["w_small", "w_large"])
@pytest.mark.parametrize("route,n,P,family,mode", APPLY_CASES, ids=[c[0] for c in APPLY_CASES])
def test_apply_fitted_state_to_new_data(ctx, route, n, P, family, mode, wscale):
    """transform(): a fitted mean / std / weights / mask on a different field, per element against float64; the maximum the
    engine derives for the fp16 scaling (fitted_absmax_kernel) through a product with a panel of ones.  The matrix exposes no
    maximum, so the product is the witness: the fitted weights put max|X'| 2^10 above (w_large) or below (w_small) the raw
    maximum of the new field, which the statistics pass of eofx_apply_f32 leaves in the same slot -- taken for the fitted one
    it overflows fp16 (w_large) or leaves the operand 12 of its 22 bits (w_small: 2^-12 against the 1e-5 asserted)."""
    import torch

    from xeofs_amd import engine

    fitted = Case("apply_fit_" + route, n, P, family, mode, "host")
    new = Case("apply_new_" + route, n - 7, P, family, mode, "host")
    w = _rng(route).uniform(0.3, 1.5, P) * wscale
    fit_ref = reference(make_field(fitted), True, True, w)
    vf = fit_ref["vf"]
    mean, std = fit_ref["mean_full"], np.where(vf, 0, np.nan) + np.bincount(np.flatnonzero(vf), fit_ref["std"], P)
    Xn = make_field(new) * np.float32(1.5) + np.float32(2.0)
    Y = (Xn[:, vf].astype(np.float64) - mean[vf]) * (w[vf] / std[vf])
    apart = np.abs(Y).max() / np.nanmax(np.abs(Xn))
    assert apart >= 2.0 ** 4 or apart <= 2.0 ** -4, apart
    mat, vs = engine.apply(ctx, Xn, mean, std, w, vf, **{k_: v for k_, v in _layout_kw(mode).items() if k_ != "keep_raw"})
    plan = apply_plan(new.n, P, int(vf.sum()), new.n, mode)
    assert vs.all() and mat.masked == (plan["layout"] == "masked") and mat.layout()[1] == (plan["layout"] != "written")
    bound = 5 * E32 * np.abs(Y) + 2.0 ** -47 * np.abs(mean[vf]) * (w[vf] / std[vf])
    # max |X'| as the products see it: understated by 2^4 the fp16 operand overflows, overstated it loses the low bits
    Z = torch.ones((mat.n_pad, 32), dtype=torch.float32, device="cuda")
    Z[mat.n:] = 0
    Yp = engine.panel_tmul(ctx, mat, Z, prec="f16x3").cpu().numpy().astype(np.float64)
    Yp = Yp[mat.valid_index] if mat.masked else Yp[:mat.p]
    colsum, colabs = Y.sum(0), np.abs(Y).sum(0)
    r = _ratio(("apply", f"{route}_w{wscale:g}", "ones_product"), np.abs(Yp[:, 0] - colsum), 1e-5 * colabs + 2.0 ** -37 * np.abs(Y).max() * mat.n)
    assert np.isfinite(Yp).all() and r <= 1.0, (route, r)
    D = mat.download()
    r = _ratio(("apply", f"{route}_w{wscale:g}", "matrix"), np.abs(D - Y), bound)
    assert D.shape == Y.shape and r <= 1.0, (route, r)
    mat.free()
    other = vf.copy()
    other[3] = not other[3]
    with pytest.raises(ValueError, match="different locations"):
        engine.apply(ctx, Xn, mean, std, w, other)


@pytest.mark.parametrize("case", RESAMPLE_CASES, ids=lambda c: c.id)
def test_resample_member_statistics(ctx, case):
    """bootstrap member: rows drawn with replacement (repeats, n_rows != n) through the row map of the statistics kernels"""
    from xeofs_amd import engine

    rng = _rng("res" + case.id)
    X = (rng.standard_normal((case.n, case.P)) * rng.uniform(0.5, 3.0, case.P) + rng.uniform(-5.0, 30.0, case.P)).astype(np.float32)
    src = engine.from_dense(ctx, X)
    rows = rng.integers(0, case.n, case.n_rows)
    rows[:3] = rows[3]                                       # repeats for certain
    ref = reference(X[rows], True, False, None)
    dmean, dM2 = two_step_bounds(ref)
    outs = []
    for _ in range(2):
        mem, mean, tv = engine.resample(ctx, src, rows, center=True)
        outs.append((mean.copy(), tv))
        if len(outs) == 1:
            r = _ratio(("resample", case.id, "mean"), np.abs(mean - ref["mean"]), MARGIN * dmean)
            assert r <= 1.0, (case.id, "mean", r)
            t_lo, t_hi = tv_interval(ref, dM2, False)
            _ratio(("resample", case.id, "tv"), np.abs(tv - ref["tv"]), max(t_hi - ref["tv"], ref["tv"] - t_lo))
            assert t_lo <= tv <= t_hi
            check_matrix(ctx, "resample", case.id, mem, ref, element_bound(ref, dmean, dM2, True, False))
        mem.free()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    for bad in (-1, case.n):
        with pytest.raises(ValueError, match="out of range"):
            engine.resample(ctx, src, np.array([0, bad, 1]))
    src.free()
