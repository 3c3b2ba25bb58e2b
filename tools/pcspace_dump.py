"""Every array of the filter covariances and of the PC-space models built on them, on fixed seeds, into one .npz -- to
compare two checkouts bit for bit (`pcspace_dump.py OUT.npz`, then `--compare A.npz B.npz`, exit status 1 on a difference).
Records engine.lagcov for p in {1, 17, 64, 257}, n = 203, ntau in {1, 65, 66, 202}; engine.lowpass_cov with the filtered
panel for the same p, h in {1, 40, 202}, with and without a trend; and every public accessor, the fitted data, `transform`
and `inverse_transform` (where implemented) of an OPA, an LFCA (detrend on and off) and a POP fit on the first shape of each
model's GPU test."""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

ACCESSORS = ["components", "scores", "filter_patterns", "decorrelation_time", "low_frequency_ratio", "filtered_scores", "eigenvalues",
             "damping_times", "periods", "components_amplitude", "components_phase", "scores_amplitude", "scores_phase",
             "singular_values", "explained_variance", "explained_variance_ratio"]
PRIVATE = ["_U", "_C0", "_R", "_Vq", "_weights", "_half", "_pca_scores", "_pca_components", "_Pq", "_W"]


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    bad += [k for k in sorted(set(A.files) & set(B.files))
            if A[k].dtype != B[k].dtype or not np.array_equal(A[k], B[k], equal_nan=A[k].dtype.kind in "fc")]
    print(f"pcspace_dump: {len(A.files)} / {len(B.files)} arrays, {len(bad)} differ" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def kernels(out):
    import torch

    from xeofs_amd import engine
    from xeofs_amd.single.lfca import linear_trend

    ctx = engine.default_context(0)
    n = 203
    for p in (1, 17, 64, 257):
        rng = np.random.default_rng(1000 + p)
        S = (rng.standard_normal((n, p)) + 0.02 * rng.standard_normal(p) * np.arange(n)[:, None]).astype(np.float32)
        Sd = torch.from_numpy(S).cuda()
        trend = linear_trend(S) * (1.0 + 0.3 * rng.standard_normal((2, p)))
        for ntau in (1, 65, 66, 202):
            w = rng.standard_normal(ntau) * rng.choice([1e-3, 1.0, 10.0], ntau)
            out[f"lagcov.p{p}.ntau{ntau}"] = engine.lagcov(ctx, Sd, w).cpu().numpy()
        for h in (1, 40, 202):
            w = rng.standard_normal(h + 1) * rng.choice([1e-3, 1.0, 10.0], h + 1)
            for name, tr in (("trend", trend), ("plain", None)):
                R, Y = engine.lowpass_cov(ctx, Sd, w, tr, return_filtered=True)
                out[f"lowpass.p{p}.h{h}.{name}.R"], out[f"lowpass.p{p}.h{h}.{name}.Y"] = R.cpu().numpy(), Y.cpu().numpy()


def models(out):
    import test_gpu_lfca as tl
    import test_gpu_opa as to
    import test_gpu_pop as tp
    import xeofs_amd as xe
    from xeofs_amd import labelled

    def record(key, obj):
        if isinstance(obj, (np.ndarray, float, int, np.generic)):
            out[key] = np.asarray(obj)
        else:
            vals, dims, coords, name, _ = labelled.unpack(obj)
            out[key] = np.asarray(vals)
            out[key + "|dims"] = np.array(list(dims) + [str(name)])

    def call(key, fn, *a, **kw):
        try:
            record(key, fn(*a, **kw))
        except (NotImplementedError, AttributeError) as e:          # part of the surface too: the text must not change
            out[key + "|raises"] = np.array(f"{type(e).__name__}: {e}")

    def surface(tag, m, new):
        for name in ACCESSORS:
            if hasattr(m, name):
                call(f"{tag}.{name}", getattr(m, name))
        for name, v in m.data.items():
            record(f"{tag}.data.{name}", v)
        for name in PRIVATE:
            if hasattr(m, name):
                record(f"{tag}.{name}", getattr(m, name))
        for flag in (True, False):
            call(f"{tag}.transform.{flag}", m.transform, new, normalized=flag)
            call(f"{tag}.inverse.{flag}", m.inverse_transform, m.scores(), normalized=flag)
        call(f"{tag}.inverse.modes", m.inverse_transform, m.scores().sel(mode=[2, 1]))

    n, P, q, T, k = to.SHAPES[0]
    X = to.ar1_mixture(n, P)
    surface("OPA", xe.single.OPA(n_modes=k, tau_max=T, n_pca_modes=q, random_state=0).fit(to.da(X), dim="time"),
            to.da(to.ar1_mixture(50, P, seed=1)))
    n, P, q, cutoff, h = tl.SHAPES[0]
    X = tl.trending_mixture(n, P)
    for detrend in (True, False):
        m = xe.single.LFCA(n_modes=tl.K, cutoff=cutoff, window=2 * h + 1, detrend=detrend, n_pca_modes=q, random_state=0)
        surface(f"LFCA.detrend{int(detrend)}", m.fit(tl.da(X), dim="time"), tl.da(tl.trending_mixture(50, P, seed=1)))
    n, P, seed = tp.SHAPES[0]
    X = tp.oscillators(n, P, seed)
    surface("POP", xe.single.POP(n_pca_modes=8, random_state=0).fit(tp.da(X), dim="time"), tp.da(tp.oscillators(50, P, seed + 1)))


def main(out_path):
    warnings.simplefilter("ignore")
    out = {}
    kernels(out)
    models(out)
    np.savez(out_path, **out)
    print(f"pcspace_dump: wrote {len(out)} arrays to {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else main(sys.argv[1]))
