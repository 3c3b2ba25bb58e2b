"""The probe table of tests/test_gpu_fresh_context.py: one or more small calls per entry of the C ABI (include/eofx.h), each
with a "main" and an "alt" variant, so that a test can ask whether an entry returns the same bits as the first call of a fresh
context, on a context other calls have used before, and between calls of the same entry with every other size.

A probe is `Probe(name, group, entries, cfg, fn, check)`:
  entries   the C ABI names the probe calls
  cfg       {"main": {...}, "alt": {...}}: every parameter that could be part of a size or of a cache key (n, p, L, k, ld, tau,
            embedding, padding, decay, bandwidth, ntau, h, hop ...) differs between the two
  run(ctx, variant) -> a tuple of host numpy arrays: every output, the integer ones, iteration counts and status words among them
  cfg["near"] (where the entry takes a value that is no size: a decay, a seed, a power, a step ...) is "main" with the sizes kept and
            that value changed -- the predecessor that a cache keyed by shape alone would confuse with "main"
  check     (optional) the float64 check of the "main" result, for the probes whose route depends on the state of the context
            (the bounds are those of the entry's own tests, named at each check)

Inputs come from a generator seeded by the probe's name and the variant; the values of "alt" are scaled by 2^10.  This module
imports without a GPU: torch and the engine are imported inside the functions.  EXEMPT names the entries without a result to
compare.  tests/test_fresh_probes_cpu.py holds the table against include/eofx.h.
"""

from __future__ import annotations

import ctypes as C
import types
import zlib

import numpy as np

ALT_SCALE = 2.0 ** 10
VARIANTS = ("main", "alt")


class Gen:
    """the seeded inputs of (probe, variant)"""

    def __init__(self, name: str, variant: str):
        self.rng = np.random.default_rng(zlib.crc32(f"{name}/{variant}".encode()))
        self.scale = ALT_SCALE if variant == "alt" else 1.0

    def normal(self, *shape, dtype=np.float32):
        return (self.rng.standard_normal(shape) * self.scale).astype(dtype)

    def field(self, n, p, rank=6, offset=3.0, noise=0.5):
        """a low-rank signal with a decaying spectrum, noise and an offset, float32 [n x p]"""
        amp = 4.0 * 0.7 ** np.arange(rank)
        X = (self.rng.standard_normal((n, rank)) * amp) @ self.rng.standard_normal((rank, p))
        X = X + noise * self.rng.standard_normal((n, p)) + offset
        return (X * self.scale).astype(np.float32)

    def panel(self, rows_pad, rows, L, l=None):
        """a zero-padded float32 panel [rows_pad x L] with `rows` x `l` live entries"""
        l = L if l is None else l
        P = np.zeros((rows_pad, L), np.float32)
        P[:rows, :l] = self.rng.standard_normal((rows, l)) * self.scale
        return P


class Probe:
    def __init__(self, name, group, entries, cfg, fn, check=None):
        self.name, self.group, self.entries, self.cfg, self.fn, self.check = name, group, tuple(entries), cfg, fn, check

    def params(self, variant):
        return types.SimpleNamespace(**self.cfg[variant])

    def shape(self, variant):
        """the parameters of the variant as a sorted tuple"""
        return tuple(sorted((k, v if isinstance(v, (int, float, str, bool)) else tuple(v)) for k, v in self.cfg[variant].items()))

    def run(self, ctx, variant):
        import torch

        out = host(self.fn(ctx, self.params(variant), Gen(self.name, variant)))
        torch.cuda.synchronize(ctx.device)
        return out

    def verify(self, out):
        """the float64 check of the "main" result (nothing for a probe without a route that depends on the context)"""
        if self.check is not None:
            self.check(out, self.params("main"), Gen(self.name, "main"))


def host(x):
    """outputs -> a flat tuple of host numpy arrays (device tensors are copied, scalars become 0-d arrays)"""
    if x is None:
        return ()
    if isinstance(x, dict):
        return tuple(a for key in sorted(x) for a in host(x[key]))
    if isinstance(x, (tuple, list)):
        return tuple(a for item in x for a in host(item))
    if hasattr(x, "detach"):
        return (np.ascontiguousarray(x.detach().cpu().numpy()),)
    if isinstance(x, (bool, np.bool_)):
        return (np.asarray(int(x), np.int64),)
    if isinstance(x, (int, np.integer)):
        return (np.asarray(x, np.int64),)
    if isinstance(x, float):
        return (np.asarray(x, np.float64),)
    return (np.ascontiguousarray(np.asarray(x)).copy(),)


def bits(a: np.ndarray) -> np.ndarray:
    """the raw bits of an array, so that NaNs and signed zeros compare as what they are"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind in "fc":
        return a.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])
    if a.dtype.kind == "b":
        return a.view(np.uint8)
    return a


def same_bits(a, b) -> bool:
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))
                                    for x, y in zip(a, b))


def first_difference(a, b) -> str:
    """where two results of a probe first differ (for the assertion message)"""
    if len(a) != len(b):
        return f"{len(a)} outputs against {len(b)}"
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"output {i}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        d = np.flatnonzero(bits(x).reshape(-1) != bits(y).reshape(-1))
        if d.size:
            j = int(d[0]) // max(1, bits(x).size // max(1, x.size))
            return (f"output {i} ({x.dtype}{x.shape}): {d.size} words differ, first at flat index {j}: "
                    f"{x.reshape(-1)[j]!r} against {y.reshape(-1)[j]!r}")
    return "equal"


def _dev(ctx, a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{ctx.device}")


def _up(x, m):
    return (int(x) + m - 1) // m * m


def _stats(st):
    return [st[key] for key in ("mean", "std", "valid_feature", "valid_sample", "n", "p", "total_variance")]


def _weights(p):
    return np.sqrt(np.cos(np.linspace(-1.2, 1.2, p)))


# ------------------------------------------------------------------------------------------------------------------------------
# field entries
# ------------------------------------------------------------------------------------------------------------------------------
def _nan_columns(X, g, every):
    X[:, ::every] = np.nan
    return X


def _preprocess(mode):
    def fn(ctx, c, g):
        from xeofs_amd import engine

        X = g.field(c.n, c.p)
        if mode in ("copy", "masked"):
            _nan_columns(X, g, c.every)
        kw = dict(copy={}, in_place=dict(in_place=True), masked=dict(in_place=True, allow_masked=True), raw=dict(keep_raw=True))[mode]
        mat, st = engine.preprocess(ctx, _dev(ctx, X) if mode != "copy" else X, True, bool(c.standardize), _weights(c.p), **kw)
        out = _stats(st) + [mat.n, mat.p, mat.n_pad, mat.p_pad, int(mat.masked), mat.layout(), mat.download(), mat.sumsq()]
        if mode == "raw":       # X^T Z streams the raw field through the Scaler map until the field is released
            Z = _dev(ctx, g.panel(mat.n_pad, mat.n, 32))
            out += [engine.panel_tmul(ctx, mat, Z, prec="f16x3")]
            mat.release_raw()
            out += [mat.layout(), engine.panel_tmul(ctx, mat, Z, prec="f16x3"), mat.download()]
        if mode == "in_place":  # the sample-contiguous layout comes and goes on demand
            Y = _dev(ctx, g.panel(mat.p_pad, mat.p, 32))
            mat.release_sample_layout()
            out += [mat.has_sample_layout(), engine.panel_mul(ctx, mat, Y, prec="f16x3")]
            out += [mat.ensure_sample_layout(only_if_room=False), mat.has_sample_layout(), engine.panel_mul(ctx, mat, Y, prec="f16x3")]
            mat.release_sample_layout()
            out += [mat.has_sample_layout(), mat.layout()]
        mat.free()
        return out
    return fn


_PRE_ENTRIES = ("eofx_preprocess_f32", "eofx_mat_download_f32", "eofx_mat_sumsq_f64", "eofx_mat_shape", "eofx_mat_masked", "eofx_mat_layout",
                "eofx_mat_destroy")


def _apply(ctx, c, g):
    from xeofs_amd import engine

    X = _nan_columns(g.field(c.n, c.p), g, c.every)
    mat, st = engine.preprocess(ctx, X, True, True, None)
    Xn = _nan_columns(g.field(c.m, c.p), g, c.every)
    out = []
    for in_place in (False, True):
        m2, vs = engine.apply(ctx, Xn, st["mean"], st["std"], None, st["valid_feature"], in_place=in_place, allow_masked=in_place)
        out += [m2.download(), vs]
        m2.free()
    mat.free()
    return out


def _from_dense(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    mat = engine.from_dense(ctx, X)
    out = [mat.download(), mat.n_pad, mat.p_pad]
    mat.free()
    return out


def _resample(ctx, c, g):
    from xeofs_amd import engine

    mat = engine.from_dense(ctx, g.field(c.n, c.p))
    rows = g.rng.integers(0, c.n, size=c.m)
    m2, mean, tv = engine.resample(ctx, mat, rows, center=True)
    out = [m2.download(), mean, tv]
    m2.free(); mat.free()
    return out


def _panel_bootstrap(ctx, c, g):
    from xeofs_amd import engine

    rows_pad = _up(c.n, 512)
    idx = g.rng.integers(0, c.n, size=c.n).astype(np.int64)
    order = np.argsort(idx, kind="stable").astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=c.n))]).astype(np.int64)
    P = _dev(ctx, g.panel(rows_pad, c.n, c.L))
    di, do, dr = (_dev(ctx, a) for a in (idx, order, rowptr))
    return [engine.panel_bootstrap(ctx, P, c.n, di, do, dr, t) for t in (False, True)]


def _norms(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    out = []
    for in_place in (False, True):
        mat, _ = engine.preprocess(ctx, _dev(ctx, X) if in_place else X, in_place=in_place)
        out += [mat.sumsq(), engine.feature_norms(ctx, mat), engine.sample_norms(ctx, mat)]
        mat.free()
    return out


def _gram(ctx, c, g):
    from xeofs_amd import engine

    X, Y = g.field(c.n, c.p), g.field(c.n, c.p, offset=-1.0)
    out = []
    for in_place in (False, True):
        mx, _ = engine.preprocess(ctx, _dev(ctx, X) if in_place else X, in_place=in_place)
        my, _ = engine.preprocess(ctx, _dev(ctx, Y) if in_place else Y, in_place=in_place)
        out += [mx.gram(0), mx.gram(1), mx.cross_gram(my, 0), mx.cross_gram(my, 1)]
        mx.free(); my.free()
    return out


def _vec_dot(ctx, c, g):
    from xeofs_amd import engine

    return [engine.vec_dot(ctx, _dev(ctx, g.normal(c.n)), _dev(ctx, g.normal(c.n)))]


# ------------------------------------------------------------------------------------------------------------------------------
# products
# ------------------------------------------------------------------------------------------------------------------------------
def _products(prec):
    def fn(ctx, c, g):
        from xeofs_amd import engine

        out = []
        for n, p in c.shapes:
            X = g.field(n, p)
            for in_place in (False, True):
                mat = engine.preprocess(ctx, _dev(ctx, X), in_place=True)[0] if in_place else engine.from_dense(ctx, X)
                Z = _dev(ctx, g.panel(mat.n_pad, n, c.L))
                Y = _dev(ctx, g.panel(mat.p_pad, p, c.L))
                out += [engine.panel_tmul(ctx, mat, Z, prec=prec), engine.panel_mul(ctx, mat, Y, prec=prec)]
                mat.free()
        return out
    return fn


def _tmul_nt_inputs(c, g):
    X = g.normal(c.n, c.p)
    Z = np.zeros((_up(c.n, 512), c.L), np.float32)
    Z[:c.n] = g.normal(c.n, c.L)
    return X, Z


def _tmul_nt(ctx, c, g):
    from xeofs_amd import engine

    X, Z = _tmul_nt_inputs(c, g)
    mat = engine.from_dense(ctx, X)
    Y = engine.panel_tmul(ctx, mat, _dev(ctx, Z), prec="f16x3")
    mat.free()
    return [Y]


def _tmul_nt_check(out, c, g):
    """the bound of test_wide_feature_side_product_on_a_fresh_context (tests/test_gpu_gram.py)"""
    X, Z = _tmul_nt_inputs(c, g)
    want = X.astype(np.float64).T @ Z[:c.n].astype(np.float64)
    assert np.abs(out[0][:c.p] - want).max() <= 3e-6 * np.sqrt(c.n) * 4.0 * 4.0
    assert not out[0][c.p:].any()


def _project_reconstruct(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    V = np.linalg.qr(g.rng.standard_normal((c.p, c.k)))[0].astype(np.float32)
    out = []
    for in_place in (False, True):
        mat, _ = engine.preprocess(ctx, _dev(ctx, X) if in_place else X, in_place=in_place)
        S = engine.project(ctx, mat, V)
        out += [S, engine.reconstruct(ctx, S, V)]
        mat.free()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# panel helpers
# ------------------------------------------------------------------------------------------------------------------------------
def _panel_gram(ctx, c, g):
    from xeofs_amd import engine

    return [engine.panel_gram(ctx, _dev(ctx, g.panel(c.rows_pad, c.rows, c.L, c.l)))]


def _cholqr(ctx, c, g):
    from xeofs_amd import engine

    P = _dev(ctx, g.panel(c.rows_pad, c.rows, c.L, c.l))
    G = engine.panel_gram(ctx, P)
    return [G, engine.panel_rinv(ctx, G, c.l), engine.panel_cholqr(ctx, P, c.l, G)]


def _cholqr_check(out, c, g):
    """Q orthonormal over its l columns at the bound of test_panel_gram_cholqr (tests/test_gpu_parity.py), zeros beyond them"""
    Q = out[2].astype(np.float64)
    assert np.isfinite(Q).all() and not Q[:, c.l:].any() and not Q[c.rows:].any()
    assert np.abs(Q[:, :c.l].T @ Q[:, :c.l] - np.eye(c.l)).max() < 5e-5


def _rinv_inputs(c, scale):
    import orth_reference as oref

    G, _ = oref.design_gram(c.l, seed=c.l)
    return oref.embed(G * scale * scale, c.L, fill=0.0)


def _rinv(ctx, c, g):
    from xeofs_amd import engine

    return [engine.panel_rinv(ctx, _dev(ctx, _rinv_inputs(c, g.scale)), c.l)]


def _rinv_check(out, c, g):
    """structure and forward error as test_rinv_blocked_and_host_routes (tests/test_gpu_orth_chain.py): 32 x numpy's error"""
    import orth_reference as oref

    Gp, X, l = _rinv_inputs(c, g.scale), out[0], c.l
    assert np.isfinite(X).all() and not np.tril(X, -1).any() and not X[l:].any() and not X[:, l:].any()
    assert [j for j in range(l) if X[j, j] == 0.0] == []
    Xref = oref.chol_rinv_ref(Gp, l, [])[:l, :l]
    E = oref.scaled_error(X[:l, :l], Xref, Gp[:l, :l])
    En = oref.scaled_error(oref.numpy_rinv(Gp[:l, :l]), Xref, Gp[:l, :l])
    assert E <= 32 * max(En, 2.0 ** -53), (E, En)


def _matmul_inputs(c, g):
    P = (g.rng.standard_normal((c.rows, c.L)) * np.exp(g.rng.uniform(-3, 3, size=c.L)) * g.scale).astype(np.float32)
    M = g.rng.standard_normal((c.L, c.Lo)) / np.sqrt(c.L)
    return P, M


def _matmul(ctx, c, g):
    from xeofs_amd import engine

    P, M = _matmul_inputs(c, g)
    return [engine.panel_matmul(ctx, _dev(ctx, P), _dev(ctx, M))]


def _matmul_nt_check(out, c, g):
    """the bound of test_wide_panel_matmul_through_the_nt_kernel (tests/test_gpu_gram.py)"""
    P, M = _matmul_inputs(c, g)
    ref = P.astype(np.float64) @ M
    assert np.abs(out[0] - ref).max() <= 3e-6 * np.abs(ref).max()


def _colminmax(ctx, c, g):
    from xeofs_amd import engine

    P = _dev(ctx, g.panel(c.rows_pad, c.rows, c.L))
    return [engine.panel_colminmax(ctx, P, c.rows), engine.panel_colargminmax(ctx, P, c.rows)]


def _export_import(ctx, c, g):
    from xeofs_amd import engine

    src = g.normal(c.rows, c.l)
    P = engine.panel_import(ctx, src, c.rows_pad, c.L)
    sign = np.where(g.rng.random(c.k) < 0.5, -1.0, 1.0)
    return [P, engine.panel_export(ctx, P, c.rows, c.k, sign), engine.panel_export(ctx, P, c.rows, c.k, None, device_out=True)]


def _rownorm(ctx, c, g):
    from xeofs_amd import engine

    P = _dev(ctx, g.panel(c.rows_pad, c.rows, c.L))
    return [engine.panel_rownorm(ctx, P, c.rows), engine.panel_row_normalize(ctx, P)]


def _rot_step(ctx, c, g):
    from xeofs_amd import engine

    X = g.panel(c.rows, c.rows, c.L, c.m) / g.scale            # (normalised loadings: values of order one)
    R = np.zeros((c.L, c.L))
    R[:c.m, :c.m] = np.linalg.qr(g.rng.standard_normal((c.m, c.m)))[0]
    b = X[:, :c.m].astype(np.float64) @ R[:c.m, :c.m]
    aux0 = np.zeros(c.L); aux0[:c.m] = (b ** 2).sum(0) / c.rows
    aux1 = np.ones(c.L); aux1[:c.m] = np.abs(b).max(0)
    Xd, Rd = _dev(ctx, X), _dev(ctx, R)
    return [engine.panel_rot_step(ctx, Xd, Rd, _dev(ctx, aux0), 0), engine.panel_rot_step(ctx, Xd, Rd, _dev(ctx, aux1), 1, c.power)]


def _cpanel(ctx, c, g):
    from xeofs_amd import engine

    P1, P2 = (_dev(ctx, g.panel(c.rows_pad, c.rows, c.L)) for _ in range(2))
    return [engine.cpanel_combine(ctx, P1, P2, False), engine.cpanel_combine(ctx, P1, P2, True), engine.cpanel_colabsmax(ctx, P1, c.rows)]


# ------------------------------------------------------------------------------------------------------------------------------
# real drivers
# ------------------------------------------------------------------------------------------------------------------------------
def _centred(X):
    return X - X.mean(axis=0, dtype=np.float64).astype(np.float32)


def _orthonormal(Q, k, tol=2e-5):
    Q = Q.astype(np.float64)
    assert np.isfinite(Q).all() and np.abs(Q.T @ Q - np.eye(k)).max() < tol


def _rsvd(ctx, c, g):
    from xeofs_amd import engine

    mat = engine.from_dense(ctx, _centred(g.field(c.n, c.p, rank=12)))
    out = engine.rsvd(ctx, mat, c.k, random_state=c.seed)
    mat.free()
    return list(out)


def _rsvd_check(out, c, g):
    """singular values against the float64 oracle on the same sketch and orthonormal factors: test_rsvd_vs_oracle
    (tests/test_gpu_parity.py); a full-width sketch against the exact SVD: test_rsvd_rank_error_and_wide_sketch"""
    from oracle import eof_oracle as orc

    U, s, V = out
    X64 = _centred(g.field(c.n, c.p, rank=12)).astype(np.float64)
    if c.k + 10 >= min(c.n, c.p):
        se = np.linalg.svd(X64, compute_uv=False)[:c.k]
        assert np.abs(s - se).max() <= 2e-5 * se[0]
    else:
        _, so, _ = orc.decomposer_fit(X64, c.k, random_state=c.seed, solver="randomized")
        assert np.abs(s - so).max() <= 1e-5 * so[0], (s, so)
    _orthonormal(U, c.k); _orthonormal(V, c.k)


def _fit_field(c, g):
    X = g.field(c.n, c.p, rank=12)
    if getattr(c, "every", 0):
        _nan_columns(X, g, c.every)
    return X


def _fit(ctx, c, g):
    from xeofs_amd import engine

    mat, st, U, s, V = engine.fit(ctx, _fit_field(c, g), c.k, random_state=c.seed, allow_masked=bool(getattr(c, "every", 0)))
    info = engine.fit_info(ctx)
    out = _stats(st) + [st["fused"], info["fused"], info["reason"], mat.n, mat.p, int(mat.masked), U, s, V]
    mat.free()
    return out


def _fit_check(out, c, g):
    """singular values and total variance against the float64 oracle at 1e-5, as smoke() and test_world1_masked_field_stays_on_the_
    sharded_entry; orthonormal factors at 2e-5 (test_rsvd_vs_oracle)"""
    from oracle import eof_oracle as orc

    U, s, V = out[-3:]
    ref = orc.eof_fit(_fit_field(c, g).astype(np.float64), c.k, random_state=c.seed)
    assert np.all(np.abs(s - ref["norms"]) <= 1e-5 * ref["norms"][0]), (s, ref["norms"])
    assert abs(float(out[6]) - ref["total_variance"]) <= 1e-5 * ref["total_variance"]
    assert bool(out[7]) == bool(c.fused)
    _orthonormal(U, c.k); _orthonormal(V, c.k)


def _fit_first(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    Z = _dev(ctx, g.panel(_up(c.n, 512), c.n, c.L, c.l))
    mat, st, Yp = engine.fit_first(ctx, _dev(ctx, X), Z, c.l)
    out = _stats(st) + [st["fused"], Yp, mat.download()]
    mat.free()
    return out


def _fit_first_check(out, c, g):
    """Yp = X'^T Z at the elementwise bound of test_panel_tmul_mul (tests/test_gpu_parity.py): 1e-5 sum |x| |z|"""
    X = g.field(c.n, c.p).astype(np.float64)
    Z = g.panel(_up(c.n, 512), c.n, c.L, c.l)[:c.n].astype(np.float64)
    Xc = X - X.mean(0)
    assert np.all(np.abs(out[8][:c.p] - Xc.T @ Z) <= 1e-5 * (np.abs(Xc).T @ np.abs(Z)) + 1e-30)


def _cross_fields(c, g):
    T = g.rng.standard_normal((c.n, 8)) * (4.0 * 0.7 ** np.arange(8))
    X = ((T @ g.rng.standard_normal((8, c.p1)) + g.rng.standard_normal((c.n, c.p1))) * g.scale).astype(np.float32)
    Y = ((T @ g.rng.standard_normal((8, c.p2)) + g.rng.standard_normal((c.n, c.p2))) * g.scale).astype(np.float32)
    return X, Y


_CROSS_KEYS = ("Q1", "s", "Q2", "scores1", "scores2", "norm1", "norm2", "total_squared_covariance")


def _cross(form):
    def fn(ctx, c, g):
        from xeofs_amd import engine
        from xeofs_amd._lib import ptr, raise_for

        X, Y = _cross_fields(c, g)
        in_place = bool(c.in_place)
        mx, _ = engine.preprocess(ctx, _dev(ctx, X) if in_place else X, in_place=in_place)
        my, _ = engine.preprocess(ctx, _dev(ctx, Y) if in_place else Y, in_place=in_place)
        if form == "lazy":
            res = engine.crosscov_rsvd(ctx, mx, my, c.k, random_state=c.seed)
        elif form == "sharded":
            engine.comm_set_callback(ctx, lambda buf, count, dtype, op, stream: 0, 1, 0)
            try:
                res = engine.crosscov_rsvd_sharded(ctx, mx, my, c.k, c.p1, 0, c.p2, 0, random_state=c.seed)
            finally:
                engine.comm_clear(ctx)
        else:           # the entry that takes the sketch itself
            om = engine.sketch_matrix(min(c.p1, c.p2), c.k + 10, c.seed)
            o = engine._CrossOut(mx, my, c.k)
            raise_for(ctx.lib.eofx_crosscov_rsvd_f32(ctx.handle, mx.handle, my.handle, c.k, 10, -1, ptr(om), 1, *o.args, C.byref(o.tsc)),
                      ctx.handle)
            res = o.as_dict()
        mx.free(); my.free()
        return [res[key] for key in _CROSS_KEYS]
    return fn


def _cross_check(out, c, g):
    """singular values and the total squared covariance against the float64 oracle: test_crosscov_vs_oracle (tests/test_gpu_parity.py)"""
    from oracle import eof_oracle as orc

    X, Y = _cross_fields(c, g)
    ref = orc.mca_fit(X.astype(np.float64), Y.astype(np.float64), c.k, random_state=c.seed, solver="randomized")
    res = dict(zip(_CROSS_KEYS, out))
    so = ref["singular_values"]
    assert np.all(np.abs(res["s"] - so) <= 1e-5 * so + 2e-6 * so[0]), (res["s"], so)
    tsc = ref["total_squared_covariance"]
    assert abs(float(res["total_squared_covariance"]) - tsc) <= 1e-5 * tsc
    _orthonormal(res["Q1"], c.k); _orthonormal(res["Q2"], c.k)


def _fit_sharded(ctx, c, g):
    from xeofs_amd import engine

    engine.comm_set_callback(ctx, lambda buf, count, dtype, op, stream: 0, 1, 0)
    try:
        res = engine.fit_sharded(ctx, _fit_field(c, g), c.k, c.p, random_state=c.seed)
    finally:
        engine.comm_clear(ctx)
    assert res is not None, "the sharded entry voted for the panel-level driver"
    mat, st, U, s, V = res
    out = [st["mean"], st["std"], st["valid_feature"], st["valid_sample"], st["n"], st["p"], st["total_variance"], True, True, 0, mat.n, mat.p,
           int(mat.masked), U, s, V]
    mat.free()
    return out


# ---- null modes on a long factor ------------------------------------------------------------------------------------------
def null_field(c, g):
    """the recipe of test_more_modes_than_numerical_rank_real_path (tests/test_gpu_parity.py): exactly rank r, offset 4"""
    X = (g.rng.standard_normal((c.n, c.r)) * 2.0 ** -np.arange(c.r)) @ g.rng.standard_normal((c.r, c.p)) + 4.0
    return (X * g.scale).astype(np.float32)


def null_singular_values(c, g):
    X = null_field(c, g).astype(np.float64)
    return np.linalg.svd(X - X.mean(0), compute_uv=False)[:c.k]


def _null(entry):
    def fn(ctx, c, g):
        from xeofs_amd import engine

        X = null_field(c, g)
        if entry == "rsvd":
            mat, _ = engine.preprocess(ctx, X, True, False, None)
            U, s, V = engine.rsvd(ctx, mat, c.k, random_state=1)
        else:
            mat, st, U, s, V = engine.fit(ctx, X, c.k, random_state=1)
        mat.free()
        return [U, s, V]
    return fn


def _null_check(out, c, g):
    """the assertions of test_more_modes_than_numerical_rank_real_path (tests/test_gpu_parity.py)"""
    U, s, V = out
    k = c.k
    assert np.isfinite(U).all() and np.isfinite(V).all() and np.isfinite(s).all()
    assert np.abs(U.T.astype(np.float64) @ U - np.eye(k)).max() < 2e-5
    assert np.abs(V.T.astype(np.float64) @ V - np.eye(k)).max() < 2e-5
    X = null_field(c, g).astype(np.float64)
    Xc = X - X.mean(0)
    se = np.linalg.svd(Xc, compute_uv=False)[:k]
    good = se > 1e-4 * se[0]
    assert good.sum() == min(c.r, k)
    assert np.all(np.abs(s - se)[good] <= 2e-5 * se[0])
    assert np.all(s[~good] <= 1e-5 * se[0])
    n_good = int(good.sum())
    R = Xc @ V[:, :n_good].astype(np.float64) - U[:, :n_good].astype(np.float64) * s[:n_good]
    assert np.abs(R).max() <= 5e-5 * se[0]


# ------------------------------------------------------------------------------------------------------------------------------
# complex / Hilbert
# ------------------------------------------------------------------------------------------------------------------------------
def _waves(c, g):
    tt, xx = np.arange(c.n)[:, None], np.linspace(0, 2 * np.pi, c.p)[None, :]
    X = sum(a * np.cos(w * tt - m * xx + ph) for a, w, m, ph in ((3.0, 0.21, 2, 0.0), (1.7, 0.37, -3, 0.4), (0.9, 0.11, 1, 1.0)))
    return ((X + 0.3 * g.rng.standard_normal((c.n, c.p))) * g.scale).astype(np.float32)


def _hilbert(ctx, c, g):
    from xeofs_amd import engine

    X = _waves(c, g)
    out = []
    for padding in ("exp", "none"):
        mat, _ = engine.preprocess(ctx, X)
        B, A2 = engine.hilbert(ctx, mat, padding, c.decay, want_real=True)
        out += [B.download(), A2.download()]
        B.free(); A2.free(); mat.free()
        mat, _ = engine.preprocess(ctx, _dev(ctx, X), in_place=True, for_hilbert=True)
        B, _ = engine.hilbert(ctx, mat, padding, c.decay)
        out += [B.download()]
        B.free(); mat.free()
    return out


def _hilbert_small(ctx, c, g):
    from xeofs_amd import engine

    mat, _ = engine.preprocess(ctx, _dev(ctx, _waves(c, g)), in_place=True, for_hilbert=True)
    out = [engine.hilbert_sumsq(ctx, mat, padding, c.decay) for padding in ("exp", "none")]
    out += [engine.hilbert_operator(ctx, c.n, padding, c.decay) for padding in ("exp", "none")]
    mat.free()
    return out


def _cmat_mul(ctx, c, g):
    from xeofs_amd import engine

    X = _waves(c, g)
    A, _ = engine.preprocess(ctx, _dev(ctx, X), in_place=True)
    B, _ = engine.hilbert(ctx, A, "exp", c.decay)
    Ps, Pf = _dev(ctx, g.panel(A.n_pad, c.n, c.L)), _dev(ctx, g.panel(A.p_pad, c.p, c.L))
    out = []
    for conj_left, P in ((True, Ps), (False, Pf)):
        for final in (False, True):
            out += [engine.cmat_mul(ctx, A, B, P, conj_left, final), engine.hilbert_cmat_mul(ctx, A, P, conj_left, "exp", c.decay, final)]
    A.free(); B.free()
    return out


def _rsvd_complex(form):
    def fn(ctx, c, g):
        from xeofs_amd import engine

        X = _waves(c, g)
        operator = form in ("operator", "operator_sharded")
        A, _ = engine.preprocess(ctx, _dev(ctx, X), in_place=True, for_hilbert=operator)
        B = None
        if operator:
            tv = engine.hilbert_sumsq(ctx, A, "exp", c.decay)
        else:
            B, _ = engine.hilbert(ctx, A, "exp", c.decay)
            tv = B.sumsq()
        if form.endswith("sharded"):
            engine.comm_set_callback(ctx, lambda buf, count, dtype, op, stream: 0, 1, 0)
        try:
            if form == "operator":
                res = engine.rsvd_hilbert_c64(ctx, A, c.k, "exp", c.decay, random_state=c.seed)
            elif form == "two_part":
                res = engine.rsvd_c64(ctx, A, B, c.k, random_state=c.seed)
            elif form == "operator_sharded":
                res = engine.rsvd_hilbert_sharded_c64(ctx, A, c.k, c.p, "exp", c.decay, random_state=c.seed)
            else:
                res = engine.rsvd_sharded_c64(ctx, A, B, c.k, c.p, random_state=c.seed)
        finally:
            if form.endswith("sharded"):
                engine.comm_clear(ctx)
        its = engine.last_iterations(ctx)
        A.free()
        if B is not None:
            B.free()
        return [tv, its] + list(res)
    return fn


def _complex_check(out, c, g):
    """singular values against the exact float64 SVD of the analytic signal and orthonormal factors: the bounds of
    tests/test_gpu_complex.py (|s - se| <= 1e-5 se + 2e-6 se[0]; orthonormality as the real drivers)"""
    from oracle import eof_oracle as orc

    U, s, V = out[2:]
    X = _waves(c, g).astype(np.float64)
    Xc = X - X.mean(0)
    Z = Xc + 1j * orc.hilbert_transform(Xc, padding="exp", decay_factor=c.decay).imag
    se = np.linalg.svd(Z, compute_uv=False)[:c.k]
    assert np.all(np.abs(s - se) <= 2e-5 * se[0]), (s, se)
    for Q in (U, V):
        Q = Q.astype(np.complex128)
        assert np.abs(Q.conj().T @ Q - np.eye(c.k)).max() < 2e-5


# ------------------------------------------------------------------------------------------------------------------------------
# lag operator
# ------------------------------------------------------------------------------------------------------------------------------
def _lag(ctx, c, g):
    from xeofs_amd import engine

    mat, _ = engine.preprocess(ctx, g.field(c.n, c.p))
    nprime = engine.lag_samples(mat, c.tau, c.embedding)
    mean, tv = engine.lag_stats(ctx, mat, c.tau, c.embedding)
    Z = _dev(ctx, g.panel(_up(nprime, 512), nprime, c.L))
    Ye = engine.lag_tmul(ctx, mat, c.tau, c.embedding, mean, Z)
    W = engine.lag_mul(ctx, mat, c.tau, c.embedding, mean, Ye, prec="f16x3")
    E = engine.lag_embed(ctx, mat, c.tau, c.embedding)
    out = [mean, tv, Ye, W, E]
    mat.free()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the model kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _gw(ctx, c, g):
    from xeofs_amd import engine

    mat = engine.from_dense(ctx, _centred(g.field(c.n, c.p)))
    xy = g.rng.uniform(0.0, 10.0, size=(c.n, 2))
    cov, tv, _ = engine.gw_cov(ctx, mat, xy, "euclidean", c.kernel, c.bandwidth, c.first, c.count)
    comps, ev, tv2, _ = engine.gwpca(ctx, mat, xy, c.k, c.bandwidth, metric="euclidean", kernel=c.kernel)
    w, V = engine.batched_syev(ctx, cov, c.k)
    mat.free()
    return [cov, tv, comps, ev, tv2, w, V]


def _spca_loop(ctx, c, g):
    from xeofs_amd import spca
    from xeofs_amd._lib import ptr, raise_for
    import torch

    V = np.linalg.qr(g.rng.standard_normal((c.p, c.l)))[0]
    D = np.ascontiguousarray(3.0 * 0.9 ** np.arange(c.l) * g.scale)
    Vd = spca._dev64(ctx, V)
    B = torch.zeros((c.p, c.k), dtype=torch.float64, device=Vd.device)
    Qa, dt, obj, it = np.zeros((c.l, c.k)), np.zeros(c.k), np.zeros(c.iters), C.c_int(-1)
    raise_for(ctx.lib.eofx_spca_loop_f64(ctx.handle, ptr(Vd), c.p, c.l, ptr(D), c.k, float(c.alpha), 1e-3, spca.SPCA_REGULARIZERS[c.reg],
                                         c.iters, 0.0, 1, ptr(B), ptr(Qa), ptr(dt), ptr(obj), C.byref(it)), ctx.handle)
    return [B, Qa, dt, obj, it.value]


def _spca_small(ctx, c, g):
    from xeofs_amd import spca

    X, Y = spca._dev64(ctx, g.normal(c.rows, c.a, dtype=np.float64)), spca._dev64(ctx, g.normal(c.rows, c.b, dtype=np.float64))
    M = g.rng.standard_normal((c.a, c.b))
    return [spca.spca_gram(ctx, X, Y), spca.spca_rowmul(ctx, X, M), spca.spca_prox(ctx, X, None, 0.0, "l1", c.kappa * g.scale),
            spca.spca_prox(ctx, X[:, :min(c.a, c.b)].contiguous(), Y[:, :min(c.a, c.b)].contiguous(), 0.5, "l0", c.kappa * g.scale)]


def _lagcov(ctx, c, g):
    from xeofs_amd import engine

    S = g.normal(c.n, c.p)
    return [engine.lagcov(ctx, S, 0.9 ** np.arange(ntau)) for ntau in c.ntaus]


def _lowpass(ctx, c, g):
    from xeofs_amd import engine

    S = g.normal(c.n, c.p)
    w = np.hanning(2 * c.h + 3)[c.h + 1:-1]
    w = w / (w[0] + 2 * w[1:].sum())
    trend = np.stack([S.mean(0, dtype=np.float64), g.rng.standard_normal(c.p) * 1e-2 * g.scale])
    return [engine.lowpass_cov(ctx, S, w, trend, return_filtered=True), engine.lowpass_cov(ctx, S, w), engine.lowpass(ctx, S, w, trend)]


def _orderpos(ctx, c, g):
    from xeofs_amd import engine

    out = []
    for n in c.lengths:
        T = g.normal(c.p, n)
        ties = np.arange(0, n - 1, 7)
        T[:, ties] = T[:, ties + 1]                             # equal values: the order among them is part of the result
        out += list(engine.order_positions(ctx, T, scale=g.rng.uniform(0.5, 2.0, c.p) * g.scale, want="both"))
    return out


def _rank_matrix(ctx, c, g):
    from xeofs_amd import engine

    mat, _ = engine.preprocess(ctx, g.field(c.n, c.p))
    Z = engine.rank_matrix(ctx, mat, weights=g.rng.uniform(0.5, 2.0, c.p) * g.scale)
    out = [Z.download(), Z.n_pad, Z.p_pad]
    Z.free(); mat.free()
    return out


def _colquad(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    A = g.normal(c.n, c.n) / g.scale
    mat, _ = engine.preprocess(ctx, X)
    out = [engine.colquad(ctx, np.ascontiguousarray(X.T), A), engine.mat_colquad(ctx, mat, A)]
    mat.free()
    return out


def _pairmin(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p, offset=0.0)
    w = (1.0 / np.linalg.norm(X.astype(np.float64), axis=0)).astype(np.float32)
    w[::11] = 0.0
    mat = engine.from_dense(ctx, X)
    out = [engine.pairmin(ctx, np.ascontiguousarray(X.T), w), engine.mat_pairmin(ctx, mat, w)]
    mat.free()
    return out


def _simplex_rows(ctx, c, g):
    from xeofs_amd import engine

    out = []
    for m in c.widths:
        V, G = g.normal(c.r, m), g.normal(c.r, m)
        out += [engine.simplex_rows(ctx, V), engine.simplex_rows(ctx, V, G, c.step)]
    return out


def _simplex_pg(ctx, c, g):
    from xeofs_amd import engine

    Zm = g.rng.standard_normal((c.k, c.q)) * g.scale
    X = g.rng.dirichlet(np.ones(c.k), size=c.n) @ Zm
    A0 = g.rng.dirichlet(np.ones(c.k), size=c.n).astype(np.float32)
    M = Zm @ Zm.T
    return [engine.simplex_pg(ctx, A0, (X @ Zm.T).astype(np.float32), M, 1.0 / np.linalg.eigvalsh(M)[-1], c.iters)]


def _kmeans(ctx, c, g):
    from xeofs_amd import engine

    Z = g.normal(c.n, c.q) + np.repeat(g.normal(c.k, c.q) * 3.0, -(-c.n // c.k), axis=0)[:c.n]
    C0 = np.stack([Z[g.rng.choice(c.n, c.k, replace=False)] for _ in range(c.R)])
    return engine.kmeans_lloyd(ctx, Z.astype(np.float32), C0, c.max_iter, want_mind2=True)


def _fastica(ctx, c, g):
    from xeofs_amd import engine
    import torch

    S = g.rng.laplace(size=(c.n, c.q))
    Zw = np.linalg.qr(S - S.mean(0))[0] * np.sqrt(c.n) * g.scale          # white columns (scaled in "alt")
    Z = _dev(ctx, Zw.astype(np.float32))
    out = []
    for fun in c.funs:
        W = _dev(ctx, np.stack([np.linalg.qr(g.rng.standard_normal((c.q, c.q)))[0] for _ in range(c.R)]))
        status = torch.zeros(c.R, dtype=torch.int32, device=Z.device)
        iters = torch.zeros(c.R, dtype=torch.int32, device=Z.device)
        res = engine.fastica(ctx, Z, W, status, iters, fun=fun, alpha=c.alpha, tol=1e-6, max_iter=c.max_iter)
        out += [W, status, iters, res]
    return out


def _spectral(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    t = np.arange(c.nfft)
    B = np.concatenate([np.cos(2 * np.pi * np.outer(np.arange(c.ncoef // 2), t) / c.nfft),
                        np.sin(2 * np.pi * np.outer(np.arange(c.ncoef - c.ncoef // 2), t) / c.nfft)]).astype(np.float32)
    nblk = (c.n - c.nfft) // c.hop + 1
    mat = engine.from_dense(ctx, X)
    Q = engine.blockxform(ctx, np.ascontiguousarray(X.T), B, c.hop, nblk)
    Qm = engine.mat_blockxform(ctx, mat, B, c.hop, nblk)
    G = engine.rowgram(ctx, Q)
    W = g.normal(c.ncoef, c.q, nblk) / g.scale
    mat.free()
    return [Q, Qm, G, engine.slabmul(ctx, W, Q)]


def _pcmul(ctx, c, g):
    import torch

    from xeofs_amd import engine

    M = g.rng.standard_normal((c.a, c.b))
    X32, X64 = g.normal(c.rows, c.a), g.normal(c.rows, c.a, dtype=np.float64)
    return [engine.pcmul(ctx, X32, M), engine.pcmul(ctx, X64, M), engine.pcmul(ctx, X32, M, out_dtype=torch.float32),
            engine.pcmul(ctx, _dev(ctx, X64), _dev(ctx, M), out_dtype=torch.float32)]


def _viewcov(ctx, c, g):
    from xeofs_amd import engine

    Z = g.normal(c.n, c.offsets[-1])
    return [engine.viewcov(ctx, Z, c.offsets), engine.viewcov(ctx, Z, c.offsets, center=False, keep_diag=True)]


def _gaps(ctx, c, g):
    from xeofs_amd import engine

    X = g.field(c.n, c.p)
    X[g.rng.random((c.n, c.p)) < 0.2] = np.nan
    F = _dev(ctx, X)
    gbits, count = engine.gap_mask(ctx, F)
    sums = engine.lrfill(ctx, F, gbits, g.normal(c.n, c.k), g.normal(c.p, c.k) / g.scale)
    return [gbits, count, sums, F]


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
def _p(name, group, entries, main, alt, fn, check=None, near=None):
    cfg = {"main": main, "alt": alt}
    if near:        # "main" with the sizes kept and one or two VALUES changed: what a cache keyed by shape alone would confuse
        cfg["near"] = dict(main, **near)
    return Probe(name, group, entries, cfg, fn, check)


_MAT = ("eofx_mat_from_dense_f32", "eofx_mat_shape", "eofx_mat_masked", "eofx_mat_destroy")
_C64 = ("eofx_preprocess_f32", "eofx_ctx_last_iterations", "eofx_hilbert_sumsq_f64", "eofx_hilbert_f32")

PROBES = [
    # ---- field entries
    _p("preprocess_copy", "field", _PRE_ENTRIES, dict(n=120, p=700, every=9, standardize=1), dict(n=90, p=530, every=7, standardize=0),
       _preprocess("copy"), near=dict(standardize=0)),
    _p("preprocess_in_place", "field", _PRE_ENTRIES + ("eofx_mat_ensure_sample_layout", "eofx_mat_release_sample_layout", "eofx_panel_mul_f32"),
       dict(n=130, p=800, standardize=0), dict(n=75, p=1100, standardize=1),
       _preprocess("in_place"), near=dict(standardize=1)),
    _p("preprocess_masked", "field", _PRE_ENTRIES, dict(n=100, p=900, every=5, standardize=0), dict(n=140, p=1300, every=8, standardize=1),
       _preprocess("masked"), near=dict(standardize=1, every=3)),
    _p("preprocess_raw", "field", _PRE_ENTRIES + ("eofx_mat_release_raw", "eofx_panel_tmul_f32"),
       dict(n=110, p=640, standardize=1), dict(n=200, p=452, standardize=0), _preprocess("raw"), near=dict(standardize=0)),
    _p("apply", "field", ("eofx_apply_f32", "eofx_preprocess_f32"), dict(n=80, m=30, p=600, every=6), dict(n=60, m=45, p=410, every=4), _apply),
    _p("from_dense_download", "field", _MAT + ("eofx_mat_download_f32",), dict(n=70, p=530), dict(n=513, p=33), _from_dense),
    _p("resample", "field", ("eofx_resample_f32",), dict(n=90, m=90, p=520), dict(n=140, m=100, p=300), _resample),
    _p("panel_bootstrap", "field", ("eofx_panel_bootstrap_f32",), dict(n=300, L=32), dict(n=700, L=64), _panel_bootstrap),
    _p("norms", "field", ("eofx_mat_sumsq_f64", "eofx_mat_feature_norms_f64", "eofx_mat_sample_norms_f64"), dict(n=150, p=900),
       dict(n=64, p=1700), _norms),
    _p("gram", "field", ("eofx_mat_gram_f32", "eofx_mat_cross_gram_f32"), dict(n=200, p=1100), dict(n=330, p=600), _gram),
    _p("vec_dot", "field", ("eofx_vec_dot_f64",), dict(n=100003), dict(n=4099), _vec_dot),
    # ---- products
    _p("products_f32", "product", ("eofx_panel_tmul_f32", "eofx_panel_mul_f32"), dict(shapes=((1000, 520), (64, 3000)), L=64),
       dict(shapes=((600, 1032), (130, 2100)), L=32), _products("f32")),
    _p("products_f16x3", "product", ("eofx_panel_tmul_f32", "eofx_panel_mul_f32"), dict(shapes=((1000, 520), (64, 3000)), L=64),
       dict(shapes=((600, 1032), (130, 2100)), L=96), _products("f16x3")),
    _p("products_f64", "product", ("eofx_panel_tmul_f32", "eofx_panel_mul_f32"), dict(shapes=((1000, 520), (64, 3000)), L=64),
       dict(shapes=((600, 1032), (130, 2100)), L=32), _products("f64")),
    _p("tmul_nt", "product", ("eofx_panel_tmul_f32",), dict(n=700, p=3000, L=512), dict(n=640, p=2500, L=544), _tmul_nt, _tmul_nt_check),
    _p("project_reconstruct", "product", ("eofx_project_f32", "eofx_reconstruct_f32"), dict(n=150, p=1000, k=7), dict(n=220, p=612, k=12),
       _project_reconstruct),
    # ---- panel helpers
    _p("panel_gram", "panel", ("eofx_panel_gram_f64",), dict(rows_pad=5120, rows=5000, L=64, l=60), dict(rows_pad=1536, rows=1100, L=32, l=20),
       _panel_gram),
    _p("cholqr_narrow", "panel", ("eofx_panel_cholqr_f32", "eofx_panel_rinv_f64", "eofx_panel_gram_f64"),
       dict(rows_pad=2048, rows=2000, L=64, l=60), dict(rows_pad=1024, rows=700, L=32, l=25), _cholqr),
    _p("cholqr_blocked", "panel", ("eofx_panel_cholqr_f32", "eofx_panel_rinv_f64", "eofx_panel_gram_f64"),
       dict(rows_pad=2048, rows=2000, L=96, l=70), dict(rows_pad=1536, rows=1500, L=160, l=130), _cholqr, _cholqr_check),
    _p("rinv_blocked", "panel", ("eofx_panel_rinv_f64",), dict(l=70, L=96), dict(l=130, L=160), _rinv, _rinv_check),
    _p("matmul_narrow", "panel", ("eofx_panel_matmul_f32",), dict(rows=1029, L=64, Lo=32), dict(rows=700, L=96, Lo=130), _matmul),
    _p("matmul_nt", "panel", ("eofx_panel_matmul_f32",), dict(rows=1024, L=512, Lo=260), dict(rows=1280, L=544, Lo=256), _matmul,
       _matmul_nt_check),
    _p("colminmax", "panel", ("eofx_panel_colminmax_f32", "eofx_panel_colargminmax_f32"), dict(rows_pad=1536, rows=1300, L=64),
       dict(rows_pad=1024, rows=513, L=32), _colminmax),
    _p("export_import", "panel", ("eofx_panel_export_f32", "eofx_panel_import_f32"), dict(rows_pad=1024, rows=900, L=64, l=50, k=40),
       dict(rows_pad=1536, rows=1100, L=32, l=30, k=30), _export_import),
    _p("rownorm", "panel", ("eofx_panel_rownorm_f64", "eofx_panel_row_normalize_f32"), dict(rows_pad=1024, rows=800, L=32),
       dict(rows_pad=512, rows=300, L=64), _rownorm),
    _p("rot_step_narrow", "panel", ("eofx_panel_rot_step_f64",), dict(rows=1024, L=32, m=10, power=3.0), dict(rows=1500, L=64, m=40, power=2.0),
       _rot_step, near=dict(power=4.0)),
    _p("rot_step_wide", "panel", ("eofx_panel_rot_step_f64",), dict(rows=1024, L=128, m=100, power=3.0), dict(rows=700, L=256, m=130, power=2.0),
       _rot_step, near=dict(power=4.0)),
    _p("cpanel", "panel", ("eofx_cpanel_combine_f32", "eofx_cpanel_colabsmax_f32"), dict(rows_pad=1024, rows=900, L=64),
       dict(rows_pad=1536, rows=1400, L=128), _cpanel),
    # ---- real drivers
    _p("rsvd_wide", "driver", ("eofx_rsvd_f32",) + _MAT, dict(n=300, p=2000, k=10, seed=42), dict(n=210, p=1300, k=6, seed=5), _rsvd,
       _rsvd_check, near=dict(seed=43)),
    _p("rsvd_tall", "driver", ("eofx_rsvd_f32",), dict(n=2500, p=700, k=20, seed=42), dict(n=1300, p=400, k=8, seed=3), _rsvd, _rsvd_check, near=dict(seed=43)),
    _p("rsvd_l70", "driver", ("eofx_rsvd_f32",), dict(n=300, p=2000, k=60, seed=42), dict(n=400, p=1500, k=90, seed=2), _rsvd, _rsvd_check, near=dict(seed=43)),
    _p("rsvd_full_width", "driver", ("eofx_rsvd_f32",), dict(n=40, p=600, k=35, seed=0), dict(n=700, p=24, k=20, seed=1), _rsvd, _rsvd_check),
    _p("fit_fused", "driver", ("eofx_fit_f32", "eofx_ctx_fit_info"), dict(n=320, p=2048, k=6, seed=3, fused=1),
       dict(n=200, p=3000, k=12, seed=4, fused=1), _fit, _fit_check, near=dict(seed=9)),
    _p("fit_fallback", "driver", ("eofx_fit_f32", "eofx_ctx_fit_info"), dict(n=300, p=2000, k=60, seed=3, fused=0),
       dict(n=250, p=1400, k=80, seed=4, fused=0), _fit, _fit_check, near=dict(seed=9)),
    _p("fit_masked", "driver", ("eofx_fit_f32", "eofx_ctx_fit_info"), dict(n=300, p=2400, k=7, seed=4, every=4, fused=1),
       dict(n=180, p=1900, k=5, seed=6, every=3, fused=1), _fit, _fit_check, near=dict(seed=9, every=5)),
    _p("fit_first", "driver", ("eofx_fit_first_f32",), dict(n=320, p=2048, L=32, l=20), dict(n=200, p=3000, L=64, l=50), _fit_first,
       _fit_first_check),
    _p("cross_gram_route", "driver", ("eofx_crosscov_rsvd_lazy_f32",), dict(n=300, p1=1300, p2=900, k=6, seed=7, in_place=1),
       dict(n=200, p1=700, p2=1500, k=4, seed=8, in_place=1), _cross("lazy"), _cross_check, near=dict(seed=11)),
    _p("cross_plain_route", "driver", ("eofx_crosscov_rsvd_lazy_f32",), dict(n=1000, p1=600, p2=1400, k=6, seed=7, in_place=0),
       dict(n=900, p1=1200, p2=520, k=5, seed=9, in_place=0), _cross("lazy"), _cross_check, near=dict(seed=11)),
    _p("cross_given_sketch", "driver", ("eofx_crosscov_rsvd_f32",), dict(n=300, p1=900, p2=1400, k=6, seed=7, in_place=0),
       dict(n=260, p1=1500, p2=800, k=8, seed=2, in_place=1), _cross("plain"), _cross_check, near=dict(seed=11)),
    _p("cross_sharded", "driver", ("eofx_crosscov_rsvd_sharded_f32",), dict(n=300, p1=1300, p2=900, k=6, seed=7, in_place=1),
       dict(n=200, p1=700, p2=1500, k=4, seed=8, in_place=1), _cross("sharded"), _cross_check, near=dict(seed=11)),
    _p("fit_sharded", "driver", ("eofx_fit_sharded_f32",), dict(n=320, p=2048, k=6, seed=3, fused=1), dict(n=200, p=3000, k=12, seed=4, fused=1),
       _fit_sharded, _fit_check, near=dict(seed=9)),
    # ---- null modes on a long factor
    _p("null_rsvd", "null", ("eofx_rsvd_f32",), dict(n=64, p=40000, r=3, k=40), dict(n=48, p=30000, r=2, k=33), _null("rsvd"), _null_check),
    _p("null_fit", "null", ("eofx_fit_f32",), dict(n=64, p=40000, r=3, k=40), dict(n=48, p=30000, r=2, k=33), _null("fit"), _null_check),
    # ---- complex
    _p("hilbert", "complex", ("eofx_hilbert_f32",), dict(n=300, p=700, decay=0.2),
       dict(n=210, p=1100, decay=0.35), _hilbert, near=dict(decay=0.5)),
    _p("hilbert_small", "complex", ("eofx_hilbert_sumsq_f64", "eofx_hilbert_operator_f32"), dict(n=300, p=700, decay=0.2),
       dict(n=210, p=1100, decay=0.35), _hilbert_small, near=dict(decay=0.5)),
    _p("cmat_mul", "complex", ("eofx_cmat_mul_f32", "eofx_hilbert_cmat_mul_f32"), dict(n=300, p=1500, L=64, decay=0.2),
       dict(n=210, p=2100, L=128, decay=0.35), _cmat_mul, near=dict(decay=0.5)),
    _p("rsvd_c64", "complex", ("eofx_rsvd_c64",) + _C64, dict(n=400, p=2600, k=6, seed=3, decay=0.2), dict(n=250, p=1500, k=4, seed=5, decay=0.3),
       _rsvd_complex("two_part"), _complex_check, near=dict(decay=0.5, seed=4)),
    _p("rsvd_hilbert_c64", "complex", ("eofx_rsvd_hilbert_c64",) + _C64, dict(n=400, p=2600, k=6, seed=3, decay=0.2),
       dict(n=250, p=1500, k=4, seed=5, decay=0.3), _rsvd_complex("operator"), _complex_check, near=dict(decay=0.5, seed=4)),
    _p("rsvd_sharded_c64", "complex", ("eofx_rsvd_sharded_c64",), dict(n=400, p=2600, k=6, seed=3, decay=0.2),
       dict(n=250, p=1500, k=4, seed=5, decay=0.3), _rsvd_complex("two_part_sharded"), _complex_check, near=dict(decay=0.5, seed=4)),
    _p("rsvd_hilbert_sharded_c64", "complex", ("eofx_rsvd_hilbert_sharded_c64",), dict(n=400, p=2600, k=6, seed=3, decay=0.2),
       dict(n=250, p=1500, k=4, seed=5, decay=0.3), _rsvd_complex("operator_sharded"), _complex_check, near=dict(decay=0.5, seed=4)),
    # ---- lag
    _p("lag", "lag", ("eofx_lag_stats_f64", "eofx_lag_tmul_f32", "eofx_lag_mul_f32", "eofx_lag_embed_f32"),
       dict(n=400, p=600, tau=3, embedding=4, L=32), dict(n=300, p=1030, tau=2, embedding=3, L=64), _lag, near=dict(tau=2)),
    # ---- the model kernels
    _p("gw", "model", ("eofx_gw_cov_f64", "eofx_gwpca_f64", "eofx_batched_syev_f64"),
       dict(n=300, p=12, k=3, bandwidth=3.0, kernel="bisquare", first=10, count=100),
       dict(n=210, p=33, k=5, bandwidth=2.0, kernel="gaussian", first=0, count=64), _gw, near=dict(bandwidth=4.5, kernel="exponential")),
    _p("spca_loop_l1", "model", ("eofx_spca_loop_f64",), dict(p=300, l=8, k=4, reg="l1", alpha=1e-3, iters=5),
       dict(p=4099, l=16, k=7, reg="l1", alpha=1e-4, iters=3), _spca_loop, near=dict(alpha=1e-2, iters=2)),
    _p("spca_loop_l0", "model", ("eofx_spca_loop_f64",), dict(p=300, l=8, k=4, reg="l0", alpha=1e-4, iters=5),
       dict(p=129, l=16, k=7, reg="l0", alpha=1e-5, iters=3), _spca_loop, near=dict(alpha=1e-3, iters=2)),
    _p("spca_loop_lds", "model", ("eofx_spca_loop_f64",), dict(p=1000, l=128, k=30, reg="l1", alpha=1e-3, iters=3),
       dict(p=700, l=120, k=40, reg="l1", alpha=1e-4, iters=2), _spca_loop, near=dict(alpha=1e-2, iters=1)),
    _p("spca_small", "model", ("eofx_spca_gram_f64", "eofx_spca_rowmul_f64", "eofx_spca_prox_f64"), dict(rows=3000, a=12, b=7, kappa=0.3),
       dict(rows=1300, a=5, b=20, kappa=0.1), _spca_small, near=dict(kappa=1.0)),
    _p("lagcov", "model", ("eofx_lagcov_f64",), dict(n=500, p=70, ntaus=(12, 70)), dict(n=300, p=130, ntaus=(5, 90)), _lagcov, near=dict(ntaus=(13, 66))),
    _p("lowpass", "model", ("eofx_lowpass_cov_f64",), dict(n=400, p=70, h=12), dict(n=260, p=130, h=5), _lowpass, near=dict(h=7)),
    _p("orderpos", "model", ("eofx_orderpos_f32",), dict(p=70, lengths=(1000, 4096)), dict(p=33, lengths=(513, 2100)), _orderpos),
    _p("rank_matrix", "model", ("eofx_mat_orderpos_f32",), dict(n=300, p=600), dict(n=1100, p=200), _rank_matrix),
    _p("colquad", "model", ("eofx_colquad_f32", "eofx_mat_colquad_f32"), dict(n=200, p=600), dict(n=130, p=1030), _colquad),
    _p("pairmin", "model", ("eofx_pairmin_f32", "eofx_mat_pairmin_f32"), dict(n=200, p=600), dict(n=130, p=1030), _pairmin),
    _p("simplex_rows", "model", ("eofx_simplex_rows_f32",), dict(r=200, widths=(300, 1500), step=0.1), dict(r=70, widths=(33, 2100), step=0.5),
       _simplex_rows, near=dict(step=0.7)),
    _p("simplex_pg", "model", ("eofx_simplex_pg_f32",), dict(n=500, k=6, q=20, iters=10), dict(n=300, k=11, q=8, iters=4), _simplex_pg, near=dict(iters=3)),
    _p("kmeans_lloyd", "model", ("eofx_kmeans_lloyd_f32",), dict(n=2000, q=6, k=4, R=3, max_iter=20), dict(n=900, q=11, k=7, R=5, max_iter=8),
       _kmeans, near=dict(max_iter=2)),
    _p("fastica", "model", ("eofx_fastica_f32",), dict(n=3000, q=5, R=3, funs=("logcosh", "exp", "cube"), alpha=1.0, max_iter=8),
       dict(n=1300, q=8, R=2, funs=("cube", "logcosh"), alpha=1.5, max_iter=3), _fastica, near=dict(alpha=2.0, max_iter=2)),
    _p("spectral", "model", ("eofx_blockxform_f32", "eofx_mat_blockxform_f32", "eofx_rowgram_f32", "eofx_slabmul_f32"),
       dict(n=400, p=600, nfft=64, hop=32, ncoef=10, q=3), dict(n=300, p=1030, nfft=48, hop=20, ncoef=7, q=5), _spectral, near=dict(hop=16)),
    _p("pcmul", "model", ("eofx_pcmul_f64",), dict(rows=3000, a=20, b=70), dict(rows=1030, a=33, b=12), _pcmul),
    _p("viewcov", "model", ("eofx_viewcov_f64",), dict(n=300, offsets=(0, 40, 100, 130)), dict(n=210, offsets=(0, 70, 90, 200, 260)), _viewcov, near=dict(offsets=(0, 30, 90, 130))),
    _p("gaps", "model", ("eofx_gapmask_f32", "eofx_lrfill_f32"), dict(n=300, p=700, k=6), dict(n=130, p=1030, k=11), _gaps),
]

BY_NAME = {p.name: p for p in PROBES}
GROUPS = tuple(dict.fromkeys(p.group for p in PROBES))

# Entries without a result to compare, each with its reason.
_LIFE = "context lifecycle: the fixtures create, synchronise, trim and destroy the contexts the probes run on"
_SET = "a setter or getter of context state with no device result of its own (the probes that depend on it call it)"
_COMM = "communicator plumbing: the sharded probes attach and clear the host-callback communicator; RCCL needs its own process group"
_HOST = "host-only: no context, no device state"
EXEMPT = {
    "eofx_abi_version": _HOST, "eofx_orth_tall_rule": _HOST, "eofx_peaked_spectrum": _HOST, "eofx_sketch_gaussian_f32": _HOST,
    "eofx_sketch_cache_drop": _HOST, "eofx_host_eigh_f64": _HOST, "eofx_host_zheigh_top_f64": _HOST,
    "eofx_ctx_create": _LIFE, "eofx_ctx_destroy": _LIFE, "eofx_ctx_synchronize": _LIFE, "eofx_ctx_trim": _LIFE,
    "eofx_ctx_set_stream": _SET, "eofx_ctx_set_layout": _SET, "eofx_ctx_set_sample_raw": _SET, "eofx_ctx_set_precision": _SET, "eofx_ctx_profile": _SET, "eofx_ctx_profile_read": _SET,
    "eofx_ctx_profile_by_kernel": _SET, "eofx_ctx_plane_stats": _SET + "; its counters run from the last read, i.e. they ARE history",
    "eofx_axb_planes_probe_f32": "a test entry that answers only under the EOFX_AXB_DMA route switch, read once per context; no test here sets an "
                                 "environment variable (tests/test_gpu_plane_producers.py runs it on contexts of its own)",
    "eofx_comm_unique_id": _COMM, "eofx_ctx_comm_init_rccl": _COMM, "eofx_ctx_comm_set_callback": _COMM, "eofx_ctx_comm_clear": _COMM,
    "eofx_ctx_comm_stats": _COMM, "eofx_ctx_comm_selftest": _COMM, "eofx_ctx_comm_probe": _COMM, "eofx_ctx_comm_allreduce_f64": _COMM,
}
