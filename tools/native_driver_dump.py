"""Every array the native SVD drivers return (plus `engine.last_iterations`) on fixed synthetic fields, into one .npz -- to
compare two builds of libeofx.so bit for bit where the host algebra between the GPU passes is touched
(`native_driver_dump.py OUT.npz`, with EOFX_LIB naming the library; then `--compare A.npz B.npz`, or
`--compare3 A1.npz A2.npz B.npz`: what differs between two runs of the SAME build is listed and held to the tolerance of its
existing test instead (TOLERANCE), everything else must be equal between A1 and B).  The sibling of cross_surface_dump.py one level down: engine.rsvd tall / wide / with a sketch
beyond 64 columns on either route of the Cholesky inverse / with more modes than rank / on a peaked spectrum over a tall panel
above 16 MiB, engine.crosscov_rsvd with more modes than rank, the branches of the real drivers those cases do not reach (`real_branches`),
engine.rsvd_c64 at the edge cases of
tests/test_gpu_complex.py with and without the block-Krylov recurrence and on the branches those do not reach (`c64_branches`),
engine.rsvd_hilbert_c64 under both rules, and the two host eigen-solvers.  With EOFX_C64_TRACE set, stderr holds the complex
driver's trace, one `# key` line after the lines of each case: two builds that take the same branches print the same text
once the milliseconds of the host-solve lines are removed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from cross_surface_dump import compare


# relative tolerance (of max |array|) at which the existing test of each driver compares it with float64: what an array that
# is not reproducible from run to run is held to (tests/test_gpu_complex.py, test_gpu_pca.py, test_host_logic.py)
TOLERANCE = (("rsvd_c64.n_iter_1", 2e-3), ("rsvd_c64.n_iter_2", 1e-4), ("host_", 1e-12), ("", 1e-5))


def compare3(a1, a2, b):
    A1, A2, B = np.load(a1), np.load(a2), np.load(b)

    def differ(P, Q):
        return sorted(set(P.files) ^ set(Q.files)) + [k for k in sorted(set(P.files) & set(Q.files))
                                                      if P[k].dtype != Q[k].dtype or not np.array_equal(P[k], Q[k], equal_nan=P[k].dtype.kind in "fc")]
    unstable = differ(A1, A2)
    bad = [k for k in differ(A1, B) if k not in unstable]
    print(f"native_driver_dump: {len(A1.files)} arrays; {len(unstable)} differ between two runs of the same build"
          + (": " + ", ".join(unstable) if unstable else "") + f"; of the other {len(A1.files) - len(unstable)}, {len(bad)} differ"
          + (": " + ", ".join(bad) if bad else ""))
    for k in unstable:          # not reproducible: held to the tolerance of its test instead
        tol = next(t for prefix, t in TOLERANCE if k.startswith(prefix))
        ok = k in B.files and B[k].shape == A1[k].shape
        if ok:
            scale = max(float(np.abs(A1[k]).max()), 1e-300)
            d12, d1b = np.abs(A1[k] - A2[k]).max() / scale, np.abs(A1[k] - B[k]).max() / scale
            ok = bool(d1b <= tol)
            print(f"  {k}: max |A1 - A2| = {d12:.3e}, max |A1 - B| = {d1b:.3e} of max |A1|, tolerance {tol:.0e}: {'ok' if ok else 'DIFFERS'}")
        if not ok:
            bad.append(k)
    return 1 if bad else 0


def low_rank(rng, n, p, rank, decay, noise, cplx=False):
    def g(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)
    X = (g(n, rank) * (6.0 * decay ** np.arange(rank))) @ g(rank, p) / np.sqrt(p)
    if noise:
        X = X + noise * g(n, p) / np.sqrt(p)
    return X


def with_env(name, value, fn):
    old = os.environ.pop(name, None)
    if value is not None:
        os.environ[name] = value
    try:
        return fn()
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


def real_branches(record):
    """The branches of the real drivers: engine.fit fused / falling back before and after the first pass / ineligible / masked in
    place / with more modes than the field has rank / refused by the two-step path (the message is recorded), engine.fit_first
    fused and falling back, engine.rsvd with a full-width sketch, engine.crosscov_rsvd on the Gram route in both orientations,
    with the route switched off, without the total squared covariance, with n above both widths, with the identity sketch, a
    SketchFuture and no sign rule, and engine.fit_sharded / engine.crosscov_rsvd_sharded over a one-rank RCCL communicator."""
    from xeofs_amd import engine

    ctx = engine.default_context()

    def field(n, p, seed, rank=9, noise=0.3):
        return (low_rank(np.random.default_rng(seed), n, p, rank, 0.7, noise) + 2.0).astype(np.float32)

    def fitted(key, res, fused=None):
        mat, st, U, s, V = res
        assert fused is None or bool(st["fused"]) == fused, (key, engine.fit_info(ctx))
        record(key, [U, s, V])
        record(key + ".stats", st)
        out[key] = engine.fit_info(ctx)["reason"]
        mat.free()

    def refused(key, fn):
        try:
            fn()
        except Exception as e:
            record(key, [np.frombuffer(f"{type(e).__name__}: {e}".encode(), np.uint8)])
        else:
            raise AssertionError(f"{key}: no error")

    def rccl1(fn):
        engine.comm_init_rccl(ctx, engine.comm_unique_id(), 1, 0)
        try:
            return fn()
        finally:
            engine.comm_clear(ctx)

    out = {}
    n, P, k = 300, 2048, 6
    X = field(n, P, 1)
    nan_feature, outlier, masked, rank4 = X.copy(), X.copy(), X.copy(), field(n, P, 2, rank=4, noise=0.0)
    nan_feature[:, 900] = np.nan                    # seen by the probe of the sampled rows: back to the two-step path before the pass
    outlier[200, 77] = 3.0e7                        # not in a sampled row: the provisional fp16 range overflows during the pass
    masked[:, np.random.default_rng(5).random(P) < 0.25] = np.nan
    # --- engine.fit
    fitted("fit.fused", engine.fit(ctx, X, k, random_state=4), fused=True)
    fitted("fit.fallback_nan_feature", engine.fit(ctx, nan_feature, k, random_state=4), fused=False)
    fitted("fit.fallback_outlier", engine.fit(ctx, outlier, k, random_state=4), fused=False)
    fitted("fit.ineligible_l32", engine.fit(ctx, X, 22, random_state=4), fused=False)
    fitted("fit.masked", engine.fit(ctx, masked, k, random_state=4, allow_masked=True), fused=True)
    fitted("fit.null_modes", engine.fit(ctx, rank4, 9, random_state=4))
    fitted("fit.no_flip", engine.fit(ctx, X, k, random_state=4, flip=False), fused=True)
    # (more modes than a 40 x 2048 field has rank: the two-step path's decomposition refuses, the matrix goes, the message stays)
    refused("fit.more_modes_than_rank", lambda: engine.fit(ctx, X[:40], 50, random_state=4))
    # --- engine.fit_first
    for tag, F, fused in (("fused", X, True), ("fallback", nan_feature, False)):
        Z = engine.panel_import(ctx, engine.sketch_matrix(n, k + 10, 4), (n + 511) // 512 * 512, 32)
        mat, st, Yp = engine.fit_first(ctx, F, Z, k + 10)
        assert bool(st["fused"]) == fused, (tag, engine.fit_info(ctx))
        record(f"fit_first.{tag}", [Yp.cpu().numpy()])
        record(f"fit_first.{tag}.stats", st)
        mat.free()
    # --- engine.rsvd, a sketch cut to the rank: 60 x 12, k = 4, l = r = 12 (the identity)
    mat = engine.from_dense(ctx, field(60, 12, 3, rank=12))
    record("rsvd.full_width", engine.rsvd(ctx, mat, 4, random_state=5))
    mat.free()
    # --- engine.crosscov_rsvd
    def pair(n, p1, p2, seed, in_place=True, nan1=None):
        rng = np.random.default_rng(seed)
        t = rng.standard_normal((n, 8)) * (5.0 * 0.8 ** np.arange(8))
        A = (t @ rng.standard_normal((8, p1)) + rng.standard_normal((n, p1))).astype(np.float32)
        B = (t @ rng.standard_normal((8, p2)) + rng.standard_normal((n, p2))).astype(np.float32)
        if nan1 is not None:
            A[:, rng.random(p1) < nan1] = np.nan
        return (engine.preprocess(ctx, A, in_place=in_place, allow_masked=nan1 is not None)[0], engine.preprocess(ctx, B, in_place=in_place)[0])

    for p1, p2 in ((1300, 900), (900, 1300)):
        mx, my = pair(300, p1, p2, 6)
        tag = f"crosscov_rsvd.wide_{p1}_{p2}"
        gram = engine.crosscov_rsvd(ctx, mx, my, k, random_state=7)
        record(tag + ".gram", gram)
        plain = with_env("EOFX_CROSS_NO_GRAM", "1", lambda: engine.crosscov_rsvd(ctx, mx, my, k, random_state=7))
        record(tag + ".no_gram", plain)
        out[tag + ".routes_differ"] = int(not np.array_equal(gram["Q1"], plain["Q1"]))
        record(tag + ".no_tsc", engine.crosscov_rsvd(ctx, mx, my, k, random_state=7, want_tsc=False))
        if p1 > p2:
            small = min(mx.p, my.p)
            record(tag + ".future", engine.crosscov_rsvd(ctx, mx, my, k, omega=engine.SketchFuture(small, k + 10, 7)))
            record(tag + ".no_flip", engine.crosscov_rsvd(ctx, mx, my, k, random_state=7, flip=False))
        mx.free()
        my.free()
    mx, my = pair(700, 50, 40, 8, in_place=False)
    record("crosscov_rsvd.tall", engine.crosscov_rsvd(ctx, mx, my, k, random_state=7))
    record("crosscov_rsvd.identity", engine.crosscov_rsvd(ctx, mx, my, 30, random_state=7))       # k + 10 = min(p1, p2)
    mx.free()
    my.free()
    # --- one rank over RCCL
    fitted("fit_sharded.plain", rccl1(lambda: engine.fit_sharded(ctx, X, k, P, random_state=4)))
    fitted("fit_sharded.masked", rccl1(lambda: engine.fit_sharded(ctx, masked, k, P, random_state=4, allow_masked=True)))
    fitted("fit_sharded.null_modes", rccl1(lambda: engine.fit_sharded(ctx, rank4, 9, P, random_state=4)))
    fitted("fit_sharded.no_flip", rccl1(lambda: engine.fit_sharded(ctx, X, k, P, random_state=4, flip=False)))
    mx, my = pair(300, 1300, 900, 6, nan1=0.25)
    assert mx.masked and not my.masked
    for flip in (True, False):
        record(f"crosscov_rsvd_sharded.masked.flip{int(flip)}",
               rccl1(lambda: engine.crosscov_rsvd_sharded(ctx, mx, my, k, mx.p, 0, my.p, 0, random_state=7, flip=flip)))
    record("crosscov_rsvd_sharded.no_tsc", rccl1(lambda: engine.crosscov_rsvd_sharded(ctx, mx, my, k, mx.p, 0, my.p, 0, random_state=7, want_tsc=False)))
    mx.free()
    my.free()
    T = np.random.default_rng(9).standard_normal((80, 3))       # more modes than rank: both sharded factors are repaired
    mx = engine.from_dense(ctx, (T @ np.random.default_rng(10).standard_normal((3, 50))).astype(np.float32))
    my = engine.from_dense(ctx, (T @ np.random.default_rng(11).standard_normal((3, 40))).astype(np.float32))
    record("crosscov_rsvd_sharded.null_modes", rccl1(lambda: engine.crosscov_rsvd_sharded(ctx, mx, my, 6, 50, 0, 40, 0, random_state=5)))
    mx.free()
    my.free()
    record("real_branches.reasons", [np.asarray([out[key] for key in sorted(out)])])
    print("native_driver_dump: real_branches: " + ", ".join(f"{key} = {out[key]}" for key in sorted(out)))


def c64_branches(record):
    """The branches of the complex driver that the edge cases of the test do not reach: a thick restart (l = 52: 7 blocks fit
    below order 384; scikit-learn's count is 4 products at this k, so 7 products and "converge" are the cases that restart),
    the lean layout, a masked in-place real part, no sign rule, outputs left on the device, the two sharded entries over a
    one-rank RCCL communicator, and one pass of eofx_cmat_mul_f32 in both directions, lean and not."""
    import torch

    from xeofs_amd import engine

    ctx = engine.default_context()

    def waves(n, p, seed, noise=0.3):
        rng = np.random.default_rng(seed)
        tt, xx = np.arange(n)[:, None], np.linspace(0, 2 * np.pi, p)[None, :]
        X = sum(a * np.cos(w * tt - m * xx + ph) for a, w, m, ph in ((3.0, 0.21, 2, 0.0), (1.7, 0.37, -3, 0.4), (0.9, 0.11, 1, 1.0)))
        return (X + noise * rng.standard_normal((n, p)) + 3.0).astype(np.float32)

    # (120 samples hold two blocks of 52 columns and a rest: that space is exhausted at the third product, before it is full;
    # 400 samples hold the 7 blocks)
    for n, n_iter, noise in ((120, "auto", 0.02), (120, "converge", 0.3), (400, 7, 0.02), (400, "converge", 0.3)):
        Z = low_rank(np.random.default_rng(11), n, 600, 9, 0.6, noise, cplx=True).astype(np.complex64)
        A = engine.from_dense(ctx, np.ascontiguousarray(Z.real))
        B = engine.from_dense(ctx, np.ascontiguousarray(Z.imag))
        record(f"rsvd_c64.thick_restart.n{n}.{n_iter}", engine.rsvd_c64(ctx, A, B, 42, random_state=2, n_iter=n_iter), iters=True)
        A.free()
        B.free()
    # lean: Re raw in place, Im in the sample-contiguous layout only; then the same field with every layout written
    X = waves(300, 1536, 7)
    for lean in (True, False):
        A, _ = engine.preprocess(ctx, X, in_place=lean)
        B, _ = engine.hilbert(ctx, A, "exp", 0.2)
        tag = "lean" if lean else "written"
        record(f"rsvd_c64.{tag}", engine.rsvd_c64(ctx, A, B, 6, random_state=3), iters=True)
        if not lean:
            record("rsvd_c64.no_flip", engine.rsvd_c64(ctx, A, B, 6, random_state=3, flip=False))
            record("rsvd_c64.device_out", [t if isinstance(t, np.ndarray) else t.cpu().numpy()
                                           for t in engine.rsvd_c64(ctx, A, B, 6, random_state=3, device_out=True)])
        gen = torch.Generator().manual_seed(5)
        for conj_left in (True, False):
            P = torch.randn((A.n_pad if conj_left else A.p_pad, 64), generator=gen).to(f"cuda:{ctx.device}")
            for final in (False, True):
                record(f"cmat_mul.{tag}.conj{int(conj_left)}.final{int(final)}",
                       [engine.cmat_mul(ctx, A, B, P, conj_left, final=final).cpu().numpy()])
        A.free()
        B.free()
    # masked in place: 30 % all-NaN grid points stay as zero columns of the real part
    X = waves(300, 1600, 9)
    X[:, np.random.default_rng(1600).choice(1600, size=480, replace=False)] = np.nan
    A, _ = engine.preprocess(ctx, X, in_place=True, allow_masked=True)
    assert A.masked
    B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    record("rsvd_c64.masked", engine.rsvd_c64(ctx, A, B, 6, random_state=3), iters=True)
    A.free()
    B.free()
    # the sharded entries, world size 1 (ncclAllReduce really runs)
    n, p, k = 400, 2600, 6
    X = waves(n, p, 4)
    for route in ("operator", "two_part"):
        A, _ = engine.preprocess(ctx, X, in_place=True, for_hilbert=(route == "operator"))
        if route == "operator":
            engine.hilbert_sumsq(ctx, A, "exp", 0.2)
        else:
            B, _ = engine.hilbert(ctx, A, "exp", 0.2)
        engine.comm_init_rccl(ctx, engine.comm_unique_id(), 1, 0)
        try:
            if route == "operator":
                got = engine.rsvd_hilbert_sharded_c64(ctx, A, k, p, "exp", 0.2, random_state=3)
            else:
                got = engine.rsvd_sharded_c64(ctx, A, B, k, p, random_state=3)
        finally:
            engine.comm_clear(ctx)
        record(f"rsvd_sharded_c64.{route}", got, iters=True)
        A.free()
        if route != "operator":
            B.free()


def main(out_path):
    from xeofs_amd import _lib, engine

    ctx = engine.default_context()
    out = {}

    def record(key, obj, iters=False):
        if os.environ.get("EOFX_C64_TRACE"):        # closes the driver's trace lines of this case on stderr
            print(f"# {key}", file=sys.stderr, flush=True)
        if isinstance(obj, dict):
            obj = [obj[name] for name in sorted(obj) if isinstance(obj[name], (np.ndarray, float, int, np.generic))]
        for i, o in enumerate(obj):
            out[f"{key}.{i}"] = np.asarray(o)
        if iters:
            out[f"{key}.iterations"] = np.asarray(engine.last_iterations(ctx))

    rng = np.random.default_rng(2024)
    # --- engine.rsvd
    for tag, n, p, k, kw, field in (
            ("tall", 700, 60, 5, {}, dict(rank=8, decay=0.7, noise=0.3)),
            ("wide", 60, 700, 5, {}, dict(rank=8, decay=0.7, noise=0.3)),
            ("l100", 300, 1500, 90, {}, dict(rank=40, decay=0.9, noise=0.3)),
            ("null_modes", 60, 700, 8, {}, dict(rank=4, decay=0.7, noise=0.0)),
            ("peaked", 200, 140000, 5, {}, dict(rank=6, decay=0.2, noise=0.02))):
        X = low_rank(rng, n, p, **field)
        mat = engine.from_dense(ctx, (X - X.mean(axis=0)).astype(np.float32))
        for host in ((None, "1") if tag == "l100" else (None,)):
            record(f"rsvd.{tag}" + (".host_rinv" if host else ""),
                   with_env("EOFX_HOST_RINV", host, lambda: engine.rsvd(ctx, mat, k, random_state=5, **kw)))
        mat.free()
    # --- engine.crosscov_rsvd, more modes than rank
    T = rng.standard_normal((80, 3))
    xm = engine.from_dense(ctx, (T @ rng.standard_normal((3, 50))).astype(np.float32))
    ym = engine.from_dense(ctx, (T @ rng.standard_normal((3, 40))).astype(np.float32))
    record("crosscov_rsvd.null_modes", engine.crosscov_rsvd(ctx, xm, ym, 6, random_state=5))
    xm.free()
    ym.free()
    real_branches(record)
    # --- engine.rsvd_c64: the cases of tests/test_gpu_complex.py::test_complex_rsvd_krylov_edge_cases
    for case in ("wide_sketch", "full_width", "rank_deficient", "n_iter_1", "n_iter_2", "converge", "feature_side"):
        crng = np.random.default_rng(11)
        n, p, k, n_iter, noise = 300, 900, 6, "auto", 0.02
        if case == "wide_sketch":
            n, p, k = 60, 400, 28
        elif case == "full_width":
            n, p, k = 24, 300, 14
        elif case == "n_iter_1":
            n_iter = 1
        elif case == "n_iter_2":
            n_iter = 2
        elif case == "converge":
            n_iter, noise = "converge", 0.3
        elif case == "feature_side":
            n, p = 900, 260
        r = 5 if case == "rank_deficient" else 9
        Z = low_rank(crng, n, p, r, 0.6, 0.0 if case == "rank_deficient" else noise, cplx=True).astype(np.complex64)
        A = engine.from_dense(ctx, np.ascontiguousarray(Z.real))
        B = engine.from_dense(ctx, np.ascontiguousarray(Z.imag))
        for krylov in (None, "0"):
            record(f"rsvd_c64.{case}.krylov{int(krylov is None)}",
                   with_env("EOFX_C64_KRYLOV", krylov, lambda: engine.rsvd_c64(ctx, A, B, k, random_state=2, n_iter=n_iter)), iters=True)
        A.free()
        B.free()
    c64_branches(record)
    # --- engine.rsvd_hilbert_c64
    X = low_rank(rng, 300, 900, 9, 0.6, 0.3)
    mat = engine.from_dense(ctx, (X - X.mean(axis=0)).astype(np.float32))
    for rule in ("auto", "converge"):
        record(f"rsvd_hilbert_c64.{rule}", engine.rsvd_hilbert_c64(ctx, mat, 6, random_state=2, n_iter=rule), iters=True)
    mat.free()
    # --- the host eigen-solvers
    for n in (1, 60, 120):
        S = rng.standard_normal((n, n))
        record(f"host_eigh.{n}", engine.host_eigh(S + S.T))
    m, nev = 240, 30
    Hm = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    Hm = Hm @ Hm.conj().T
    Hr, Hi = np.ascontiguousarray(Hm.real), np.ascontiguousarray(Hm.imag)
    w, Xr, Xi = np.zeros(nev), np.zeros((m, nev)), np.zeros((m, nev))
    rc = _lib.load().eofx_host_zheigh_top_f64(Hr.ctypes.data, Hi.ctypes.data, m, nev, w.ctypes.data, Xr.ctypes.data, Xi.ctypes.data)
    assert rc == 0
    record(f"host_zheigh_top.{m}.{nev}", (w, Xr, Xi))
    np.savez(out_path, **out)
    print(f"native_driver_dump: wrote {len(out)} arrays to {out_path}")
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:4]))
    sys.exit(compare3(*sys.argv[2:5]) if sys.argv[1] == "--compare3" else main(sys.argv[1]))
