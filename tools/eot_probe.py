"""The quadratic-form operator of empirical orthogonal teleconnections (engine.mat_colquad, csrc/eofx_colquad.hpp) and a 5-mode
EOT fit, timed at a mid size (n = 2000 samples, p = 129600 grid points) and a large one (n = 8000, p = 259200).
Every shape runs in a fresh child process under its own time limit, and a child that fails ends the probe.  The operator: the
field resident, its sample-contiguous layout built, A = the Gram matrix; warm-up calls first (code objects, the arena), then
ROUNDS calls, each between device synchronisations; median and minimum, achieved TFLOP/s = 2 n^2 p / t beside the 122 TF of an
untuned LDS-tiled float32-MFMA GEMM and the 155 TF peak of the instruction.  The fit: `EOT(n_modes=5)` on the same device
tensor, run twice, the second timed; `model.stats` splits it, and the share of a mode spent outside the kernel is
1 - ms_colquad / (the five per-mode phases).  Prints one JSON line; `--out FILE` also writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2000, 129600), (8000, 259200)]          # n, p
ROUNDS = 5
MODES = 5
CHILD_LIMIT_S = 240
GEMM_UNTUNED_TF, MFMA_F32_PEAK_TF = 122.0, 155.0


def child(n, p):
    import numpy as np
    import torch

    import xeofs_amd as xe
    from xeofs_amd import engine

    ctx = engine.default_context(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.empty((n, p), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 28) // p)
    for a in range(0, n, step):                                     # (filled in blocks: the generator's temporaries stay small)
        X[a:a + step].normal_(generator=g)
    # six planted series on top of the noise, so that the modes are real ones
    S = torch.randn((n, 6), generator=g, device="cuda")
    L = torch.randn((6, p), generator=g, device="cuda") * torch.linspace(2.0, 0.5, 6, device="cuda")[:, None]
    for a in range(0, n, step):
        X[a:a + step] += S[a:a + step] @ L
    del L

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    flops = 2.0 * n * n * p
    res = dict(n=n, p=p, rounds=ROUNDS, flops_per_mode=flops)
    mat, _ = engine.preprocess(ctx, X, True, False, None, in_place=True)
    try:
        A = mat.gram(0)[:n, :n]
        q = torch.empty(p, dtype=torch.float64, device="cuda")
        fn = lambda: engine.mat_colquad(ctx, mat, A, out=q)
        for _ in range(2):
            fn()
        first = q.clone()
        ms = [timed(fn)[0] for _ in range(ROUNDS)]
        res["two_runs_equal"] = bool(torch.equal(first.view(torch.int64), q.view(torch.int64)))
        med = float(np.median(ms))
        tf = flops / (med * 1e-3) / 1e12
        res.update(colquad_ms_median=med, colquad_ms_min=min(ms), colquad_ms_all=ms, achieved_TFLOPs=tf,
                   over_untuned_gemm=tf / GEMM_UNTUNED_TF, over_mfma_peak=tf / MFMA_F32_PEAK_TF)
        del A, q, first
    finally:
        mat.free()
    arr = xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})
    fit_ms = []
    for _ in range(2):
        m = xe.single.EOT(n_modes=MODES)
        m.ctx = ctx
        fit_ms.append(timed(lambda: m.fit(arr, dim="time"))[0])
    st = dict(m.stats)
    per_mode = sum(st[k] for k in ("ms_colquad", "ms_select", "ms_series", "ms_tmul", "ms_deflate"))
    res.update(fit_ms_first=fit_ms[0], fit_ms_second=fit_ms[1], fit_stats=st, modes=MODES,
               share_of_a_mode_outside_the_kernel=1.0 - st["ms_colquad"] / per_mode,
               base_index=[int(b) for b in m.data["base_index"]],
               explained_variance_ratio=[float(v) for v in m.data["explained_variance"] / m.data["total_variance"]])
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(int(args[1]), int(args[2]))), flush=True)
        sys.exit(0)
    shapes = []
    for n, p in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(p)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"shape ({n}, {p}) ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = dict(probe="eot", untuned_gemm_TF=GEMM_UNTUNED_TF, mfma_f32_peak_TF=MFMA_F32_PEAK_TF, shapes=shapes)
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
