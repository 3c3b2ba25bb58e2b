"""Every array the public surface of the cross models and their rotators returns, on fixed synthetic fields, into one
.npz -- to compare two checkouts bit for bit (`cross_surface_dump.py OUT.npz`, then `--compare A.npz B.npz`).
Fits CPCCA over alpha x use_pca, MCA / CCA / RDA, ComplexCPCCA / ComplexMCA, HilbertMCA with and without padding, and a
rotator (power 1 and 2) on one model of each kind; EOF / ComplexEOF ride along for `inverse_transform`; then the panel-level
complex drivers (`panel_level`)."""
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ACCESSORS = ["singular_values", "squared_covariance", "total_squared_covariance", "squared_covariance_fraction",
             "cross_correlation_coefficients", "correlation_coefficients_X", "correlation_coefficients_Y",
             "fraction_variance_X_explained_by_X", "fraction_variance_Y_explained_by_Y", "fraction_variance_Y_explained_by_X",
             "covariance_fraction_CD95", "homogeneous_patterns", "heterogeneous_patterns", "rotation_matrix", "phi_matrix",
             "explained_variance", "explained_variance_ratio"]
NORMALIZED = ["components", "scores", "components_amplitude", "components_phase", "scores_amplitude", "scores_phase"]


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    bad += [k for k in sorted(set(A.files) & set(B.files))
            if A[k].dtype != B[k].dtype or not np.array_equal(A[k], B[k], equal_nan=A[k].dtype.kind in "fc")]
    print(f"cross_surface_dump: {len(A.files)} / {len(B.files)} arrays, {len(bad)} differ" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def panel_level(record, rng):
    """The drivers under the complex models that work on [Re | Im] panels (xeofs_amd/cpanel.py) and that the models above reach
    only at one width and orientation: the Python panel route of the complex decomposition at both orientations, both panel
    widths and with more modes than rank (the null-mode repair), the complex PCA pre-reduction with either side small, and
    the complex rotation with its finishing step at 32 and 64 columns per half."""
    from xeofs_amd import engine, rotation
    from xeofs_amd.complex_svd import complex_rsvd
    from xeofs_amd.cpca import ComplexResidentPCA

    ctx = engine.default_context()

    def resident(n, p, rank, noise):
        def c(*shape):
            return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        Z = (c(n, rank) * (5.0 * 0.8 ** np.arange(rank))) @ c(rank, p) + noise * c(n, p)
        Z = Z - Z.mean(axis=0)
        return [engine.from_dense(ctx, np.ascontiguousarray(part, dtype=np.float32)) for part in (Z.real, Z.imag)]

    for n, p, k, over, rank, noise in ((60, 700, 5, 10, 6, 0.3), (700, 60, 5, 10, 6, 0.3), (60, 700, 30, 10, 6, 0.3),
                                       (60, 700, 20, None, 8, 0.0)):
        A, B = resident(n, p, rank, noise)
        kw = {} if over is None else dict(n_oversamples=over)
        U, s, V = complex_rsvd(ctx, A, B, k, random_state=11, **kw)
        record(f"complex_rsvd.{n}x{p}.k{k}", (U, s, V))
        if not noise:
            print(f"cross_surface_dump: complex_rsvd {n}x{p} k={k}: {int((s <= 3e-6 * s[0]).sum())} null modes repaired")
        A.free()
        B.free()
    for n, p in ((50, 400), (400, 50)):
        A, B = resident(n, p, 6, 0.3)
        pca = ComplexResidentPCA(ctx).fit(A, B)
        Q = rng.standard_normal((pca.m, 4)) + 1j * rng.standard_normal((pca.m, 4))
        record(f"ComplexResidentPCA.{n}x{p}", (pca.scores(), pca.s, pca.singular_values_all, pca.transform(A, B),
                                               pca.back_project(Q), pca.components()))
        A.free()
        B.free()
    for m in (3, 40):
        p = 333
        load = (rng.standard_normal((p, m)) + 1j * rng.standard_normal((p, m))) * (rng.random_sample((p, m)) < 0.2)
        load = load + 0.05 * (rng.standard_normal((p, m)) + 1j * rng.standard_normal((p, m)))
        for power in (1, 2):
            Xrot, p_, m_, rot_mat, phi = rotation.cpromax_panel(ctx, load, power=power, col_scale=np.linspace(2.0, 1.0, m))
            record(f"cpromax_panel.m{m}.p{power}",
                   (Xrot[:p].cpu().numpy(), rot_mat, phi) + rotation.cfinish_on_device(ctx, Xrot, p_, m_))


def main(out_path):
    import xeofs_amd as xe
    from xeofs_amd import labelled

    warnings.simplefilter("ignore")
    out = {}

    def record(key, obj):
        if isinstance(obj, (list, tuple)):
            for i, o in enumerate(obj):
                record(f"{key}.{i}", o)
        elif isinstance(obj, (np.ndarray, float, int, np.generic)):
            out[key] = np.asarray(obj)
        else:
            vals, dims, coords, name, _ = labelled.unpack(obj)
            out[key] = np.asarray(vals)
            out[key + "|dims"] = np.array(list(dims) + [str(name)])
            for d in dims:
                out[f"{key}|{d}"] = np.asarray(coords[d])

    def call(key, fn, *a, **kw):
        try:
            record(key, fn(*a, **kw))
        except NotImplementedError as e:          # part of the surface too: the text must not change
            out[key + "|raises"] = np.array(str(e))

    def surface(tag, m, new=None):
        for name in ACCESSORS:
            if hasattr(m, name):
                call(f"{tag}.{name}", getattr(m, name))
        for name in NORMALIZED:
            for flag in (True, False):
                if hasattr(m, name):
                    call(f"{tag}.{name}.{flag}", getattr(m, name), normalized=flag)
        if new is not None:
            for flag in (True, False):
                call(f"{tag}.transform.{flag}", m.transform, *new, normalized=flag)
            if len(new) == 2:
                call(f"{tag}.transform.Y", m.transform, Y=new[1])
        if hasattr(m, "predict"):
            call(f"{tag}.predict", m.predict, new[0])
        if hasattr(m, "inverse_transform"):
            sc = m.scores()
            if isinstance(sc, tuple):
                call(f"{tag}.inverse", m.inverse_transform, X=sc[0], Y=sc[1])
                call(f"{tag}.inverse.X2", m.inverse_transform, X=sc[0].sel(mode=[2]))
                v, d, c, _, _ = labelled.unpack(sc[1])          # no 'mode' dimension: the cross models read it as mode 1
                c.pop("mode")
                call(f"{tag}.inverse.nomode", m.inverse_transform, Y=xe.DataArray(v[0], d[1:], c))
            else:
                call(f"{tag}.inverse", m.inverse_transform, sc)
                call(f"{tag}.inverse.norm", m.inverse_transform, m.scores(normalized=True).sel(mode=[3, 1]), normalized=True)
                v, d, c, _, _ = labelled.unpack(sc)             # a scalar 'mode' coordinate: EOF reads the mode number from it
                call(f"{tag}.inverse.scalar", m.inverse_transform, xe.DataArray(v[1], d[1:], dict(c, mode=np.array(2))))

    rng = np.random.RandomState(20240)
    n, sx, sy, r = 120, (5, 8), (4, 7), 5
    T = rng.standard_normal((n + 16, r)) * (4.0 * 0.7 ** np.arange(r))

    def field(shape, dims, cplx=False):
        p = shape[0] * shape[1]
        A = T @ rng.standard_normal((r, p)) + 0.3 * rng.standard_normal((n + 16, p)) + 7.0
        if cplx:
            A = A + 1j * (np.roll(T, 3, axis=0) @ rng.standard_normal((r, p)) + 0.3 * rng.standard_normal((n + 16, p)))
        A = A.reshape((n + 16,) + shape)
        return xe.DataArray(A[:n], dims=dims), xe.DataArray(A[n:], dims=dims)

    X, Xn = field(sx, ("time", "lat", "lon"))
    Y, Yn = field(sy, ("time", "y", "x"))
    Zx, Zxn = field(sx, ("time", "lat", "lon"), True)
    Zy, Zyn = field(sy, ("time", "y", "x"), True)
    C = xe.cross
    kw = dict(n_modes=3, random_state=7)
    keep = {}
    for alpha in (0.0, 0.5, [0.0, 1.0], 1.0):
        for pca in (True, False):
            tag = f"CPCCA.a{alpha}.pca{int(pca)}"
            keep[tag] = C.CPCCA(alpha=alpha, use_pca=pca, **kw).fit(X, Y, "time")
            surface(tag, keep[tag], (Xn, Yn))
    for cls in (C.MCA, C.CCA, C.RDA):
        surface(cls.__name__, cls(standardize=True, **kw).fit(X, Y, "time"), (Xn, Yn))
    for cls in (C.ComplexCPCCA, C.ComplexMCA):
        for pca in (True, False):
            tag = f"{cls.__name__}.pca{int(pca)}"
            keep[tag] = cls(use_pca=pca, standardize=True, **kw).fit(Zx, Zy, "time")
            surface(tag, keep[tag], (Zxn, Zyn))
    for pad in ("exp", "none"):
        keep[f"HilbertMCA.{pad}"] = C.HilbertMCA(padding=pad, **kw).fit(X, Y, "time")
        surface(f"HilbertMCA.{pad}", keep[f"HilbertMCA.{pad}"])
    for rot, src, new in ((C.CPCCARotator, "CPCCA.a0.5.pca1", (Xn, Yn)), (C.ComplexCPCCARotator, "ComplexCPCCA.pca1", (Zxn, Zyn)),
                          (C.HilbertMCARotator, "HilbertMCA.exp", None)):
        for power in (1, 2):
            fitted = rot(n_modes=3, power=power).fit(keep[src])
            surface(f"{rot.__name__}.p{power}", fitted, new)
            if new is None:
                call(f"{rot.__name__}.p{power}.transform", fitted.transform, X)
    S = xe.single
    surface("EOF", S.EOF(n_modes=3, random_state=7).fit(X, "time"), (Xn,))
    surface("ComplexEOF", S.ComplexEOF(n_modes=3, random_state=7).fit(Zx, "time"))
    surface("HilbertEOF", S.HilbertEOF(n_modes=3, random_state=7).fit(X, "time"))
    panel_level(record, rng)
    np.savez(out_path, **out)
    print(f"cross_surface_dump: wrote {len(out)} arrays to {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else main(sys.argv[1]))
