"""The FastICA solver of independent component analysis (engine.fastica, csrc/eofx_ica.hpp; xeofs_amd.single.ICA) timed on white
score panels of (n, q, R) = (10000, 32, 1), (10000, 32, 50) and (350000, 20, 1) -- the last the shape of an hourly reanalysis --
against a torch loop of the same arithmetic on the same device (batched float32 matmul, tanh, the moments as float32 matmul, the
decorrelation by torch.linalg.eigh in float64; no test for convergence, which would cost it a synchronisation per iteration) and
against scikit-learn's FastICA(whiten=False) on the CPU from the same starts (one restart timed, times R reported).
Every case runs in a fresh child process under its own time limit, and a child that fails ends the probe.  The panel: q
independent non-Gaussian sources (uniform, Laplace, bimodal, cubed normal, cycled), mixed and whitened on the device.
    ms_per_iteration   a call of ITERS iterations with a tolerance no restart meets, between device synchronisations, / ITERS
    ms_per_fit         the model's loop: calls of ICA_ITER_MAX iterations until no restart is running, then the moment pass alone
A warm-up first, then ROUNDS repetitions: the median.  A last child reruns the whole-run cases of tests/test_gpu_ica_step.py and
records the ratio (device - float64) / (float32 emulation - float64) of the final W.  Prints one JSON line; `--out FILE` also
writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(10000, 32, 1), (10000, 32, 50), (350000, 20, 1)]            # n, q, R
ROUNDS = 5
ITERS = 32
MAX_ITER = 200
TOL = 1e-4
CHILD_LIMIT_S = 240


def panel(n, q):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    cols = []
    for j in range(q):
        kind = j % 4
        if kind == 0:
            s = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) - 0.5
        elif kind == 1:
            u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) - 0.5
            s = -torch.sign(u) * torch.log1p(-2.0 * u.abs())
        elif kind == 2:
            s = torch.sign(torch.rand(n, generator=g, device="cuda", dtype=torch.float64) - 0.5) + 0.3 * torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
        else:
            s = torch.randn(n, generator=g, device="cuda", dtype=torch.float64) ** 3
        cols.append(s)
    S = torch.stack(cols, dim=1)
    X = S @ torch.randn((q, q), generator=g, device="cuda", dtype=torch.float64)
    X = X - X.mean(dim=0)
    d, E = torch.linalg.eigh(X.T @ X / n)
    return ((X @ E) / d.sqrt()).float().contiguous()


def child(n, q, R):
    import numpy as np
    import torch

    from xeofs_amd import engine
    from xeofs_amd.single.ica import ica_starts

    ctx = engine.default_context(0)
    Z = panel(n, q)
    W0 = torch.from_numpy(ica_starts(q, R, 0)).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def state():
        return W0.clone(), torch.zeros(R, dtype=torch.int32, device="cuda"), torch.zeros(R, dtype=torch.int32, device="cuda")

    def fixed():
        W, st, it = state()
        engine.fastica(ctx, Z, W, st, it, tol=1e-300, max_iter=ITERS, want=())
        return W

    def fit():
        W, st, it = state()
        done = calls = 0
        while done < MAX_ITER:
            T = min(engine.ICA_ITER_MAX, MAX_ITER - done)
            engine.fastica(ctx, Z, W, st, it, tol=TOL, max_iter=T, want=())
            done, calls = done + T, calls + 1
            if bool((st != 0).all()):
                break
        res = engine.fastica(ctx, Z, W, st, it, tol=TOL, max_iter=0, want=("gmean",))
        return W, st, it, res["gmean"], calls

    fixed(), fit()
    ms_fixed = [timed(fixed)[0] for _ in range(ROUNDS)]
    fits = [timed(fit) for _ in range(ROUNDS)]
    ms_fit = [f[0] for f in fits]
    W, st, it, gmean, calls = fits[0][1]
    iters = it.cpu().numpy()
    T = int(iters.max())

    def torch_loop(T):
        Wt = W0.float()
        for _ in range(T):
            S = Z @ Wt.transpose(1, 2)                                        # R x n x q
            g = torch.tanh(S)
            W1 = (g.transpose(1, 2) @ Z) / n - (1.0 - g * g).mean(dim=1)[:, :, None] * Wt
            W1 = W1.double()
            d, E = torch.linalg.eigh(W1 @ W1.transpose(1, 2))
            Wt = ((E / d.sqrt()[:, None, :]) @ E.transpose(1, 2) @ W1).float()
        return Wt

    torch_loop(2)
    t_fixed = [timed(lambda: torch_loop(ITERS))[0] for _ in range(ROUNDS)]
    t_fit = [timed(lambda: torch_loop(T)) for _ in range(ROUNDS)]
    Wt = t_fit[0][1].double()
    # the same fixed point up to sign: |W_solver W_torch^T| is a permutation matrix for a restart both converged on
    agree = float((W[0] @ Wt[0].T).abs().max(dim=1).values.min())

    sk_ms = sk_iters = None
    try:
        import warnings

        from sklearn.decomposition import FastICA

        Zh = Z.double().cpu().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            ica = FastICA(n_components=q, whiten=False, fun="logcosh", tol=TOL, max_iter=MAX_ITER, w_init=W0[0].cpu().numpy()).fit(Zh)
            sk_ms = (time.perf_counter() - t0) * 1e3
        sk_iters = int(ica.n_iter_)
    except ImportError:
        pass
    again = fit()
    return dict(n=n, q=q, R=R, rounds=ROUNDS, iters_fixed=ITERS, solver_ms_per_iteration=float(np.median(ms_fixed)) / ITERS,
                solver_ms_per_fit=float(np.median(ms_fit)), solver_ms_fit_all=ms_fit, calls_per_fit=calls, iterations=iters.tolist()[:8],
                iterations_max=T, status_counts=np.bincount(st.cpu().numpy(), minlength=3).tolist(),
                torch_ms_per_iteration=float(np.median(t_fixed)) / ITERS, torch_ms_per_fit=float(np.median([t[0] for t in t_fit])),
                speedup_per_iteration=float(np.median(t_fixed) / np.median(ms_fixed)),
                speedup_per_fit=float(np.median([t[0] for t in t_fit]) / np.median(ms_fit)), torch_agrees=agree,
                sklearn_ms_one_restart=sk_ms, sklearn_iterations=sk_iters, sklearn_ms_all_restarts=None if sk_ms is None else sk_ms * R,
                rerun_bit_equal=bool(torch.equal(W, again[0]) and torch.equal(gmean, again[3])))


def ratios():
    """the whole-run cases of tests/test_gpu_ica_step.py: (device - float64) / (float32 emulation - float64) of the final W"""
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ica_reference as kr

    from xeofs_amd import engine

    ctx = engine.default_context(0)
    out = []
    for fun, alpha, seed, n, q, tol in kr.RUN_CASES:
        Z, W0 = kr.mixed_panel(seed, n, q)
        ref, emu = kr.run(Z, W0, fun, alpha, tol, 200), kr.run(Z, W0, fun, alpha, tol, 200, f32=True)
        W = torch.from_numpy(W0[None].copy()).cuda()
        st, it = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        engine.fastica(ctx, Z, W, st, it, fun=fun, alpha=alpha, tol=tol, max_iter=64, want=())
        dev = float(np.abs(W[0].cpu().numpy() - ref["W"]).max())
        own = float(np.abs(emu["W"] - ref["W"]).max())
        out.append(dict(fun=fun, alpha=alpha, n=n, q=q, iterations=int(it[0]), reference_iterations=ref["iters"], device_minus_float64=dev,
                        emulation_minus_float64=own, ratio=dev / own))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(*(int(a) for a in args[1:4]))), flush=True)
        sys.exit(0)
    if args[:1] == ["--ratios"]:
        print(json.dumps(ratios()), flush=True)
        sys.exit(0)
    results = []
    for extra in [["--child"] + [str(v) for v in case] for case in CASES] + [["--ratios"]]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{extra} ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = dict(probe="ica", cases=results[:-1], whole_run_ratios=results[-1])
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
