"""GPU tests at the BASELINE.json config sizes, through size-independent properties (the oracle
cannot run at these sizes in seconds): orthonormality, X V = U diag(s), linearity, centring,
bitwise determinism; plus the reference's own CPU-runnable config 1
shape against the oracle and degenerate tiny shapes."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eof_oracle as orc  # noqa: E402


def _device_field(n, nlat, nlon):
    import torch

    import bench

    return bench.make_field(n, nlat, nlon, 0, nlat * nlon, torch.device("cuda:0"))


@pytest.mark.parametrize("layout", ["inplace", "copy"])
@pytest.mark.parametrize("n,nlat,nlon,k", [(5000, 360, 720, 50), (10000, 720, 1440, 50)],
                         ids=["config2_5000x259200", "config4_10000x1036800"])
def test_eof_properties_at_baseline_sizes(ctx, n, nlat, nlon, k, layout):
    """Size-independent properties at BASELINE sizes, in the in-place layout (bench.py's and the EOF model's default:
    both products stream the raw field) and with both layouts written."""
    import torch

    from xeofs_amd import engine

    kw = {"in_place": layout == "inplace"}
    X = _device_field(n, nlat, nlon)
    mat, st = engine.preprocess(ctx, X, want_stats=False, **kw)
    assert mat.has_sample_layout() == (layout == "copy")
    assert (st["n"], st["p"]) == (n, nlat * nlon)
    U, s, V = engine.rsvd(ctx, mat, k, random_state=5, device_out=True)
    Ud, Vd = U.double(), V.double()
    sd = torch.as_tensor(s.astype(np.float64), device=Ud.device)
    eye = torch.eye(k, dtype=torch.float64, device=Ud.device)
    assert float((Ud.T @ Ud - eye).abs().max()) < 1e-6
    assert float((Vd.T @ Vd - eye).abs().max()) < 1e-6
    assert np.all(np.diff(s) <= 0) and s[-1] > 0
    # X V = U diag(s) through the projection kernel (one more pass over the matrix)
    XV = torch.as_tensor(engine.project(ctx, mat, V), device=Ud.device).double()
    assert float((XV - Ud * sd).norm() / (Ud * sd).norm()) < 1e-5
    # explained variance cannot exceed the total variance (reference tests/models/single/test_eof.py:85-100)
    assert (s.astype(np.float64) ** 2).sum() / (n - 1) <= st["total_variance"] * (1 + 1e-5)
    # bitwise determinism under the seed (tests/linalg/test_decomposer.py:164-192)
    U2, s2, V2 = engine.rsvd(ctx, mat, k, random_state=5, device_out=True)
    assert np.array_equal(s, s2) and torch.equal(U, U2) and torch.equal(V, V2)
    # the resident matrix is centred: projecting it on V gives zero-mean scores
    assert float(XV.mean(dim=0).abs().max()) <= 1e-6 * float(sd[0])
    assert mat.has_sample_layout() == (layout == "copy")     # nothing on this path materialised a layout
    mat.free()
    # linearity: decomposing 2 X doubles the singular values and leaves the vectors
    mat2, _ = engine.preprocess(ctx, X * 2.0, want_stats=False, **kw)
    U3, s3, V3 = engine.rsvd(ctx, mat2, k, random_state=5, device_out=True)
    assert np.allclose(s3, 2.0 * s, rtol=1e-6)
    assert float((V3.double() - Vd).abs().max()) < 1e-5
    mat2.free()
    ctx.trim()


def test_masked_config4_in_place(ctx):
    """SURVEY 8d's NaN variant of config 4 -- a 30 % land mask (all-NaN grid points) and cos-lat weights on the
    10000 x (720 x 1440) field -- decomposed IN PLACE (layout mode 3): 1x the field in HBM, nothing written, and the
    size-independent properties of the unmasked run hold on the valid features."""
    import torch

    from xeofs_amd import engine

    n, nlat, nlon, k = 10000, 720, 1440, 50
    X = _device_field(n, nlat, nlon)
    mask = torch.rand(nlat * nlon, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < 0.3
    X[:, mask] = float("nan")
    lat = np.linspace(-89.75, 89.75, nlat)
    w = np.repeat(np.sqrt(np.cos(np.deg2rad(lat)).clip(0, 1)), nlon)
    free0 = torch.cuda.mem_get_info()[0]
    mat, st = engine.preprocess(ctx, X, True, False, w, want_stats=False, in_place=True, allow_masked=True)
    pv = int((~mask).sum())
    assert mat.masked and mat.p == pv == st["p"] and not mat.has_sample_layout()
    assert free0 - torch.cuda.mem_get_info()[0] < 4 << 30          # no copy of the 41 GB field was made
    U, s, V = engine.rsvd(ctx, mat, k, random_state=5, device_out=True)
    assert tuple(V.shape) == (pv, k) and not mat.has_sample_layout()
    Ud, Vd = U.double(), V.double()
    sd = torch.as_tensor(s.astype(np.float64), device=Ud.device)
    eye = torch.eye(k, dtype=torch.float64, device=Ud.device)
    assert float((Ud.T @ Ud - eye).abs().max()) < 1e-6
    assert float((Vd.T @ Vd - eye).abs().max()) < 1e-6
    XV = torch.as_tensor(engine.project(ctx, mat, V), device=Ud.device).double()
    assert float((XV - Ud * sd).norm() / (Ud * sd).norm()) < 1e-5
    assert (s.astype(np.float64) ** 2).sum() / (n - 1) <= st["total_variance"] * (1 + 1e-5)
    U2, s2, V2 = engine.rsvd(ctx, mat, k, random_state=5, device_out=True)
    assert np.array_equal(s, s2) and torch.equal(V, V2)
    mat.free()
    # the same field through the compaction route (three times the memory): same singular values
    del Ud, Vd, XV, U2, V2
    mat2, st2 = engine.preprocess(ctx, X, True, False, w, want_stats=False)
    U3, s3, V3 = engine.rsvd(ctx, mat2, k, random_state=5, device_out=True)
    assert np.allclose(s3, s, rtol=2e-6)
    assert float((V3.double() - V.double()).abs().max()) < 1e-5
    mat2.free()
    ctx.trim()


def test_config1_shape_vs_oracle(ctx):
    """BASELINE config 1: xe.single.EOF(n_modes=10) on the air_temperature shape 2920 x (25 x 53)
    (synthetic stand-in of the same shape), use_coslat as in the README quickstart."""
    import xeofs_amd as xe

    n, nlat, nlon, k = 2920, 25, 53, 10
    X, lat = orc.synthetic_field(n, nlat, nlon, rank=30, seed=0)
    lat = np.linspace(75.0, 15.0, nlat)
    da = xe.DataArray(X.reshape(n, nlat, nlon) + 270.0, dims=("time", "lat", "lon"),
                      coords={"lat": lat, "lon": np.linspace(200, 330, nlon)}, name="air")
    m = xe.single.EOF(n_modes=k, use_coslat=True, random_state=5).fit(da, "time")
    w = np.repeat(orc.sqrt_cos_lat_weights(lat), nlon)
    ref = orc.eof_fit((X + 270.0).astype(np.float64), k, feature_weights=w, random_state=5)
    s = m.singular_values().values
    assert np.all(np.abs(s - ref["norms"]) <= 1e-5 * ref["norms"])
    assert np.allclose(m.explained_variance_ratio().values, ref["explained_variance_ratio"], rtol=3e-5)
    c = m.components().values.reshape(k, -1)
    for j in range(k):
        assert abs(np.dot(c[j], ref["components"][:, j])) >= 1 - 1e-5, j


@pytest.mark.parametrize("n,p,k", [(2, 3, 1), (3, 2, 2), (2, 2, 2), (5, 1, 1), (1, 4, 1)])
def test_tiny_shapes(ctx, n, p, k):
    from xeofs_amd import engine

    X = np.random.default_rng(n * 10 + p).standard_normal((n, p)).astype(np.float32)
    mat = engine.from_dense(ctx, X)
    U, s, V = engine.rsvd(ctx, mat, k, random_state=0)
    se = np.linalg.svd(X.astype(np.float64), compute_uv=False)[:k]
    assert np.allclose(s, se, rtol=2e-5, atol=1e-6)
    rec = (U * s) @ V.T
    best = np.linalg.svd(X.astype(np.float64))
    approx = (best[0][:, :k] * best[1][:k]) @ best[2][:k]
    assert np.abs(rec - approx).max() <= 1e-4


def test_all_nan_and_constant_inputs(ctx):
    from xeofs_amd import engine

    X = np.full((10, 6), np.nan, dtype=np.float32)
    with pytest.raises(ValueError, match="no valid"):
        engine.preprocess(ctx, X)
    X = np.ones((10, 6), dtype=np.float32)           # constant field: zero matrix after centring
    mat, st = engine.preprocess(ctx, X, True, True)   # std clipped at float32 eps (scaler.py:106-108)
    assert not mat.download().any() and st["total_variance"] == 0.0
    U, s, V = engine.rsvd(ctx, mat, 2, random_state=0)
    assert np.all(s == 0) and np.isfinite(U).all() and np.isfinite(V).all()


def test_two_rank_sharded_path_on_one_gpu(ctx):
    """End-to-end multi-rank path with the real HIP kernels: two processes share cuda:0, each holds half
    of the feature axis, collectives over gloo (RCCL needs one GPU per rank; the single-rank RCCL calls are
    covered by test_sharded_world1_equals_driver_bitwise).  The 2-rank singular values must equal the
    1-rank ones to float32 rounding and the global X V = U s identity must hold."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--steps", "1", "--warmup", "1", "--nlat", "90", "--nlon", "180", "--nsamples", "1500", "--modes", "12",
              "--full", "--no-cpu-baseline", "--no-configs"]  # (--full: the parity checks; --no-configs: without the full-size
    #                                                            config-3 / config-5 legs of a multi-rank line)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29517", os.path.join(root, "bench.py"),
                          "--gpus", "2", "--backend", "gloo", "--same-gpu"] + common,
                         capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert two.returncode == 0, two.stderr[-2000:]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True,
                         env=env, timeout=600, cwd=root)
    assert one.returncode == 0, one.stderr[-2000:]
    d2 = json.loads(two.stdout.strip().splitlines()[-1])
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    assert d2["n_gpus"] == 2 and d1["n_gpus"] == 1
    # the two ranks went through the engine's own sharded entry (collectives issued by the engine; here through the
    # host-callback binding, gloo underneath), not through the python driver
    assert d2["config"]["entry"].startswith("eofx_fit_sharded_f32"), d2["config"]["entry"]
    assert d2["comm"]["allreduce_calls_per_fit"] >= 15 and "callback" in d2["comm"]["binding"]
    assert len(two.stdout.strip().splitlines()) == 1 and len(one.stdout.strip().splitlines()) == 1  # ONE JSON line
    assert np.allclose(d2["parity"]["s_head"], d1["parity"]["s_head"], rtol=2e-6)
    assert d2["parity"]["XV_eq_Us_relerr"] < 1e-5 and d2["parity"]["orth_V_maxabs"] < 1e-6
    # the panel-level python driver (torch.distributed collectives between engine calls) is still there and agrees
    py2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29518", os.path.join(root, "bench.py"),
                          "--gpus", "2", "--backend", "gloo", "--same-gpu", "--no-native"] + common,
                         capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert py2.returncode == 0, py2.stderr[-2000:]
    dp = json.loads(py2.stdout.strip().splitlines()[-1])
    assert dp["config"]["entry"].startswith("sharded_fit_first")
    assert np.allclose(dp["parity"]["s_head"], d2["parity"]["s_head"], rtol=1e-6)
    # the same job without an external launcher: `bench.py --gpus 2` starts its own two ranks
    env_nl = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    self2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo",
                            "--same-gpu"] + common, capture_output=True, text=True, env=env_nl, timeout=600, cwd=root)
    assert self2.returncode == 0, self2.stderr[-2000:]
    ds = json.loads([ln for ln in self2.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert ds["n_gpus"] == 2 and np.allclose(ds["parity"]["s_head"], d2["parity"]["s_head"], rtol=1e-7)


def test_bench_plain_run_and_dump_outputs(ctx, tmp_path):
    """A plain bench run is the headline alone (--steps timed steps, ms_per_step, no parity / baseline legs), and
    --dump-outputs writes what its last step returned: the same arguments give the same outputs, and they are a valid
    decomposition (orthonormal factors, descending spectrum)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, p, k = 1500, 90 * 180, 12
    common = ["--steps", "3", "--warmup", "1", "--nlat", "90", "--nlon", "180", "--nsamples", str(n), "--modes", str(k)]
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common + ["--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(r.stdout.strip().splitlines()) == 1
        line = json.loads(r.stdout)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert "parity" not in line and "configs" not in line and line["cpu_baseline"] is None
        assert sorted(os.listdir(d)) == ["U.npy", "V.npy", "s.npy", "total_variance.npy"]
        runs.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    out = runs[0]
    assert out["U"].shape == (n, k) and out["V"].shape == (p, k) and out["s"].shape == (k,)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    for name in out:
        assert np.array_equal(out[name], runs[1][name]), name
    eye = np.eye(k)
    assert np.abs(out["U"].astype(np.float64).T @ out["U"] - eye).max() < 1e-5
    assert np.abs(out["V"].astype(np.float64).T @ out["V"] - eye).max() < 1e-5
    assert np.all(np.diff(out["s"]) <= 0) and out["s"][-1] > 0
    assert (out["s"].astype(np.float64) ** 2).sum() / (n - 1) <= out["total_variance"][0] * (1 + 1e-5)


@pytest.mark.parametrize("nan,pca", [(False, False), (True, False), (False, True)])
def test_two_rank_sharded_mca_and_eof_on_one_gpu(ctx, nan, pca):
    """SURVEY.md §8e (rows C3 + preprocess facts): two processes share cuda:0, each holds half of each
    field's space axis; `sharded_mca_fit` / `sharded_eof_fit` (HIP kernels + gloo all-reduces) against the
    single-GPU drivers on the whole fields.  Tolerances: float32 summation-order differences only."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29519", os.path.join(root, "tools", "sharded_mca_worker.py"),
           "--backend", "gloo", "--same-gpu"] + (["--nan"] if nan else []) + (["--pca"] if pca else [])
    run = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert run.returncode == 0, run.stderr[-3000:]
    d = json.loads([ln for ln in run.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert d["world"] == 2 and d["p_total"] == [d["p1"], d["p2"]]
    if nan:
        assert d["n_valid"] == 699 and d["p1"] < 5000 and d["p2"] < 3600
    assert d["mca_s"] < 2e-5 and d["eof_s"] < 2e-5
    assert d["mca_q1_cos"] > 1 - 1e-5 and d["mca_q2_cos"] > 1 - 1e-5 and d["eof_v_cos"] > 1 - 1e-5
    assert d["mca_scores1"] < 1e-4 and d["mca_scores2"] < 1e-4 and d["eof_scores"] < 1e-4
    assert d["mca_norm1"] < 1e-4 and d["mca_tsc"] < 1e-5 and d["eof_tv"] < 1e-6


@pytest.mark.parametrize("modes", [12, 40])        # 40 + 10 oversamples: the 128-column panels of the wide sketch
def test_two_rank_sharded_hilbert_complex_on_one_gpu(ctx, modes):
    """The multi-rank form of config 5 with the real HIP kernels (tools/sharded_complex_worker.py): two processes share
    cuda:0, each preprocesses and Hilbert-transforms its half of the features and takes part in the feature-sharded
    complex rSVD (one-launch complex passes, all-reduce over gloo).  Singular values equal the single-rank engine
    entry's, the global identity Z V = U s holds, the gathered V is orthonormal and spans the same modes."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29531",
                          os.path.join(root, "tools", "sharded_complex_worker.py"), "--backend", "gloo", "--same-gpu",
                          "--modes", str(modes)], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert run.returncode == 0, run.stderr[-2000:]
    d = json.loads([ln for ln in run.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert d["world"] == 2
    assert d["s_rel"] < 1e-5 and d["zv_us"] < 2e-5
    assert d["orth_v"] < 2e-5 and d["orth_u"] < 2e-5
    if modes == 12:
        assert d["v_cos_min"] > 1 - 1e-4       # (well separated leading modes; the 40-mode run ends in the noise bulk)


def test_mca_properties_at_config3(ctx):
    """BASELINE config 3: MCA(n_modes=20) on two 5000 x (360 x 360) halves, `use_pca=False` semantics, through
    size-independent properties: orthonormal singular vectors, C Q2 = Q1 diag(s) with C = X^T Y / (n - 1) applied
    matrix-free, scores = X Q1, the squared-covariance identity sum(s^2) <= TSC, bitwise determinism."""
    import torch

    from xeofs_amd import engine

    n, nlat, nlon, k = 5000, 360, 720, 20
    F = _device_field(n, nlat, nlon).reshape(n, nlat, nlon)
    X = F[:, :, :360].reshape(n, -1).contiguous()
    Y = F[:, :, 360:].reshape(n, -1).contiguous()
    del F
    mx, _ = engine.preprocess(ctx, X, want_stats=False)
    my, _ = engine.preprocess(ctx, Y, want_stats=False)
    out = engine.crosscov_rsvd(ctx, mx, my, k, random_state=5)
    Q1, Q2, s = out["Q1"].astype(np.float64), out["Q2"].astype(np.float64), out["s"].astype(np.float64)
    assert np.abs(Q1.T @ Q1 - np.eye(k)).max() < 1e-6 and np.abs(Q2.T @ Q2 - np.eye(k)).max() < 1e-6
    assert np.all(np.diff(s) <= 0) and s[-1] > 0
    # C Q2 = X^T (Y Q2) / (n - 1) = Q1 diag(s): two projections and one reconstruction-free product
    YQ2 = engine.project(ctx, my, out["Q2"]).astype(np.float64)                 # n x k
    assert np.allclose(YQ2, out["scores2"], atol=1e-4 * np.abs(YQ2).max())
    XQ1 = engine.project(ctx, mx, out["Q1"]).astype(np.float64)
    assert np.allclose(XQ1, out["scores1"], atol=1e-4 * np.abs(XQ1).max())
    cross = XQ1.T @ YQ2 / (n - 1)                                              # Q1^T C Q2 = diag(s)
    assert np.allclose(np.diag(cross), s, rtol=1e-5)
    assert np.abs(cross - np.diag(np.diag(cross))).max() < 1e-5 * s[0]
    assert np.allclose(out["norm1"], np.linalg.norm(XQ1, axis=0), rtol=1e-5)
    assert (s ** 2).sum() <= out["total_squared_covariance"] * (1 + 1e-6)
    out2 = engine.crosscov_rsvd(ctx, mx, my, k, random_state=5)
    assert np.array_equal(out["s"], out2["s"]) and np.array_equal(out["Q1"], out2["Q1"])
    # swapping the fields transposes C: same singular values, vectors exchanged
    sw = engine.crosscov_rsvd(ctx, my, mx, k, random_state=5, want_tsc=False)
    lead = 5      # the gap-separated modes; the rest sits in the noise bulk, where a randomized solver only
    #               converges to the sketch-dependent subspace (the shared t_j of the synthetic halves)
    assert np.allclose(sw["s"][:lead], out["s"][:lead], rtol=1e-5)
    assert np.abs(np.abs(np.sum(sw["Q1"].astype(np.float64) * Q2, axis=0))[:lead] - 1).max() < 1e-4
    mx.free(); my.free()
    ctx.trim()


def test_hilbert_complex_properties_at_scale(ctx):
    """BASELINE config 5 shape family (Hilbert EOF, padding='exp', decay 0.2) at 4000 x (360 x 720), k = 20:
    the analytic signal's real part is the (centred) input, its spectrum is one-sided (checked on sampled
    features with a host FFT), and the complex rSVD satisfies Z V = U diag(s) with orthonormal U, V."""
    import torch

    from xeofs_amd import engine
    from xeofs_amd.complex_svd import complex_rsvd

    n, nlat, nlon, k = 4000, 360, 720, 20
    X = _device_field(n, nlat, nlon)
    A, st = engine.preprocess(ctx, X, want_stats=False)
    del X
    B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    p = nlat * nlon
    cols = np.array([0, 1, 777, p // 2, p - 1])
    a = A.download()[:, cols].astype(np.float64)
    b = B.download()[:, cols].astype(np.float64)
    ref = orc.hilbert_transform(a, padding="exp", decay_factor=0.2)            # per-feature operation
    assert np.allclose(b, ref.imag, atol=2e-5 * np.abs(ref.imag).max())
    U, s, V = engine.rsvd_c64(ctx, A, B, k, random_state=5)                    # the engine entry bench.py times
    assert np.all(np.diff(s) <= 0) and s[-1] > 0
    Uc, Vc = U.astype(np.complex128), V.astype(np.complex128)
    assert np.abs(Uc.conj().T @ Uc - np.eye(k)).max() < 1e-5
    assert np.abs(Vc.conj().T @ Vc - np.eye(k)).max() < 1e-5
    # Z V = (A + iB) V = U diag(s): four real projections
    Vr, Vi = np.ascontiguousarray(V.real), np.ascontiguousarray(V.imag)
    ZV = (engine.project(ctx, A, Vr) - engine.project(ctx, B, Vi)) + 1j * (engine.project(ctx, A, Vi) + engine.project(ctx, B, Vr))
    Us = Uc * s.astype(np.float64)
    assert np.linalg.norm(ZV - Us) / np.linalg.norm(Us) < 2e-5
    A.free(); B.free()
    ctx.trim()


def test_config5_hilbert_complex_full_size(ctx):
    """BASELINE config 5 at its own size: 8000 x (720 x 1440), Hilbert transform with padding='exp' (decay 0.2), complex
    randomized SVD with n_modes = 20 on ONE GPU.  Size-independent properties: the imaginary part of sampled features is
    the oracle's Hilbert transform of their (centred) real part, U and V are orthonormal, (A + iB) V = U diag(s), the
    spectrum is sorted, the fit (`eofx_rsvd_c64`) is bitwise reproducible and the panel-level Python driver finds the same
    singular values.  Single columns are fetched with one-hot projections
    (nothing of the 33 GB parts crosses PCIe)."""
    import torch

    from xeofs_amd import engine
    from xeofs_amd.complex_svd import complex_rsvd

    n, nlat, nlon, k = 8000, 720, 1440, 20
    p = nlat * nlon
    X = _device_field(n, nlat, nlon)
    A, st = engine.preprocess(ctx, X, want_stats=False, in_place=True)         # lean layout: Re in place, Im^T only
    del X
    torch.cuda.empty_cache()
    B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    assert A.layout() == (False, True) and not A.has_sample_layout() and B.layout()[0] is False
    cols = np.array([0, 1, 4097, p // 2, p - 1])
    E = np.zeros((p, len(cols)), np.float32)
    E[cols, np.arange(len(cols))] = 1.0
    a = engine.project(ctx, A, E).astype(np.float64)
    b = engine.project(ctx, B, E).astype(np.float64)
    ref = orc.hilbert_transform(a, padding="exp", decay_factor=0.2)            # per-feature operation
    assert np.allclose(b, ref.imag, atol=2e-5 * np.abs(ref.imag).max())
    U, s, V = engine.rsvd_c64(ctx, A, B, k, random_state=5)                    # the engine entry bench.py times
    assert np.all(np.diff(s) <= 0) and s[-1] > 0
    Uc, Vc = U.astype(np.complex128), V.astype(np.complex128)
    assert np.abs(Uc.conj().T @ Uc - np.eye(k)).max() < 1e-5
    assert np.abs(Vc.conj().T @ Vc - np.eye(k)).max() < 1e-5
    Vr, Vi = np.ascontiguousarray(V.real), np.ascontiguousarray(V.imag)
    ZV = (engine.project(ctx, A, Vr) - engine.project(ctx, B, Vi)) + 1j * (engine.project(ctx, A, Vi) + engine.project(ctx, B, Vr))
    Us = Uc * s.astype(np.float64)
    assert np.linalg.norm(ZV - Us) / np.linalg.norm(Us) < 2e-5
    U2, s2, V2 = engine.rsvd_c64(ctx, A, B, k, random_state=5)
    assert np.array_equal(s, s2) and np.array_equal(V, V2)
    assert A.layout() == (False, True) and not A.has_sample_layout() and B.layout()[0] is False    # nothing written
    del U2, V2
    _, s3, _ = complex_rsvd(ctx, A, B, k, random_state=5)                      # the panel-level driver: same spectrum
    assert np.allclose(s3, s, rtol=2e-5)
    A.free(); B.free()
    ctx.trim()


def test_hilbert_of_the_config4_field_full_size(ctx):
    """The Hilbert stage on the 10 000 time steps of the config-4 field (circular length 2^15: one feature per workgroup
    through the half-length transform): sampled features against the oracle, the padded buffer holds nothing else
    (sum of squares over the whole buffer = sum over the valid part), bitwise reproducible."""
    import torch

    from xeofs_amd import engine

    n, nlat, nlon = 10000, 720, 1440
    p = nlat * nlon
    X = _device_field(n, nlat, nlon)
    A, st = engine.preprocess(ctx, X, want_stats=False)
    del X
    torch.cuda.empty_cache()
    B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    cols = np.array([0, 1, 2, 77777, p // 2 + 1, p - 2, p - 1])
    E = np.zeros((p, len(cols)), np.float32)
    E[cols, np.arange(len(cols))] = 1.0
    a = engine.project(ctx, A, E).astype(np.float64)
    b = engine.project(ctx, B, E).astype(np.float64)
    ref = orc.hilbert_transform(a, padding="exp", decay_factor=0.2)
    assert np.abs(b - ref.imag).max() <= 2e-6 * np.abs(ref.imag).max()
    ssq = B.sumsq()
    bf = engine.project(ctx, B, E)
    B.free()                                         # (two 83 GB results next to the 83 GB input would crowd the HBM)
    B2, _ = engine.hilbert(ctx, A, "exp", 0.2)
    assert B2.sumsq() == ssq and np.array_equal(engine.project(ctx, B2, E), bf)
    # energy of the transform of centred series is close to the input's (the filter has unit gain away from DC)
    assert 0.5 * A.sumsq() < ssq < 1.5 * A.sumsq()
    A.free(); B2.free()
    ctx.trim()


def test_dominant_mode_field_with_known_singular_values(ctx):
    """A full-size field whose singular values are known exactly: X = T W S^T with T [8000 x 60] red-noise series, geometric
    weights W and S [1 036 800 x 60] Gaussian -- one mode dominates, every sum of the passes is coherent.  The singular values
    of the centred field (and of its analytic signal: the Hilbert stage acts on T alone) follow from two small QR
    factorisations in float64.  Round 5 found the leading value 2.1e-5 low here (truncating hi / lo split + the long float32
    accumulation chains of the in-place X Y pass; eofx_kernels.hpp `cvt_pk_rn`); with the split rounding to nearest the split-fp16
    passes reproduce all 20 values to ~1e-7, in place, for the real and for both complex routes."""
    import torch

    from xeofs_amd import engine

    n, p, r, k = 8000, 720 * 1440, 60, 20
    rng = np.random.default_rng(7)
    T = np.empty((n, r))
    e = rng.standard_normal((n, r))
    T[0] = e[0]
    for i in range(1, n):
        T[i] = 0.8 * T[i - 1] + 0.6 * e[i]
    T[:, :4] += np.cumsum(rng.standard_normal((n, 4)), axis=0) * 0.05          # a few drifting series
    W = 0.93 ** np.arange(r) * 3.0
    dev = torch.device("cuda:0")
    Td = torch.as_tensor((T * W).astype(np.float32), device=dev)
    Sd = torch.randn((p, r), device=dev, dtype=torch.float32, generator=torch.Generator(dev).manual_seed(3))
    X = torch.empty((n, p), dtype=torch.float32, device=dev)
    for c0 in range(0, p, 65536):
        X[:, c0:c0 + 65536] = Td @ Sd[c0:c0 + 65536].T
    # exact values from the factors as the engine sees them (float32-rounded), float64
    T64 = Td.double().cpu().numpy()
    Tc = T64 - T64.mean(0)
    R2 = np.linalg.qr(Sd.double().cpu().numpy(), mode="r")
    s_real = np.linalg.svd(np.linalg.qr(Tc, mode="r") @ R2.T, compute_uv=False)[:k]
    ZT = orc.hilbert_transform(Tc, padding="exp", decay_factor=0.2)
    s_cplx = np.linalg.svd(np.linalg.qr(ZT, mode="r") @ R2.T, compute_uv=False)[:k]
    del Sd
    A, _ = engine.preprocess(ctx, X, want_stats=False, in_place=True, for_hilbert=True)
    _, s, _ = engine.rsvd(ctx, A, k, random_state=5, device_out=True)
    assert np.all(np.abs(s - s_real) <= 2e-6 * s_real), (np.abs(s - s_real) / s_real).max()
    sq = engine.hilbert_sumsq(ctx, A, "exp", 0.2)
    sq_exact = float((np.abs(ZT.imag @ R2.T) ** 2).sum())
    assert abs(sq - sq_exact) <= 2e-6 * sq_exact
    _, s1, _ = engine.rsvd_hilbert_c64(ctx, A, k, "exp", 0.2, random_state=5, device_out=True)
    assert np.all(np.abs(s1 - s_cplx) <= 2e-6 * s_cplx), (np.abs(s1 - s_cplx) / s_cplx).max()
    B, _ = engine.hilbert(ctx, A, "exp", 0.2)
    _, s2, _ = engine.rsvd_c64(ctx, A, B, k, random_state=5, device_out=True)
    assert np.all(np.abs(s2 - s_cplx) <= 2e-6 * s_cplx), (np.abs(s2 - s_cplx) / s_cplx).max()
    A.free(); B.free()
