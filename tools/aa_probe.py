"""Archetypal analysis (xeofs_amd.single.ArchetypalAnalysis; engine.simplex_rows, engine.simplex_pg, csrc/eofx_simplex.hpp) timed
at the bench's grid (n = 2000 samples, p = 129600 grid points, k = 8) and at the largest n the model takes (n = 16384, the
limit of the simplex kernel and of a 1 GB Gram matrix; p = 16384), with a small shape first (trouble shows early).
Every shape runs in a fresh child process under its own time limit, and a child that fails ends the probe.  The field: noisy
Dirichlet mixtures of k Gaussian patterns, made on the device.  A warm-up fit first (code objects, the arena), then ROUNDS fits
of MAX_ITER outer iterations at most, each between device synchronisations: the median fit, and its split into the Gram
matrix, the products with K, simplex_pg, simplex_rows and the host (stats of the model; every device step is followed by a
synchronisation there, so the shares add up).  Beside it: a torch restatement of the same iteration on the same K -- the recorded
steps of the last fit replayed with float32 torch operations on the device (matmul, a sort-based projection), the small
algebra on the device as well -- timed per outer iteration, and each of the two operators alone against its torch form on the
operands of the last iteration.  Prints one JSON line; `--out FILE` also writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(300, 5000, 4), (2000, 129600, 8), (16384, 16384, 8)]            # n, p, k
ROUNDS = 3
MAX_ITER = 40
CHILD_LIMIT_S = 280


def child(n, p, k):
    import numpy as np
    import torch

    import xeofs_amd as xe
    from xeofs_amd import engine

    ctx = engine.default_context(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    Z = torch.randn((k, p), generator=g, device="cuda")
    W = torch.distributions.Dirichlet(torch.full((k,), 0.5, device="cuda")).sample((n,))
    X = torch.empty((n, p), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 27) // p)
    for a in range(0, n, step):                                     # (in blocks: the temporaries stay small)
        X[a:a + step] = W[a:a + step] @ Z
        X[a:a + step] += 0.3 * torch.randn((X[a:a + step].shape[0], p), generator=g, device="cuda")
    del Z, W

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    arr = xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})

    def fit():
        m = xe.single.ArchetypalAnalysis(n_modes=k, random_state=0, max_iter=MAX_ITER)
        m.ctx = ctx
        return m.fit(arr, dim="time")

    fit()                                                           # warm-up
    runs = [timed(fit) for _ in range(ROUNDS)]
    ms = [r[0] for r in runs]
    m = runs[int(np.argsort(ms)[len(ms) // 2])][1]
    st = {key: v for key, v in m.stats.items() if key.startswith("ms_") or key in ("iterations", "products", "stalled")}
    res = dict(n=n, p=p, k=k, rounds=ROUNDS, max_iter=MAX_ITER, fit_ms_median=float(np.median(ms)), fit_ms_all=ms, fit_stats=st,
               explained_variance_fraction=m.explained_variance_fraction(),
               rejections=int(sum(s["rejections"] for s in m.stats["steps"])))
    its = max(1, m.stats["iterations"])
    res["per_iteration_ms"] = {key[3:]: st[key] / its for key in st if key.startswith("ms_") and key not in ("ms_gram", "ms_total")}

    # ---- the torch restatement of the same iteration on the same K
    mat = m.data["input_data"]
    K = mat.gram(0)[:n, :n].contiguous()
    trK = float(K.diagonal().double().sum())

    def project(U):
        s, _ = torch.sort(U, dim=1, descending=True)
        css = torch.cumsum(s, dim=1) - 1.0
        ks = torch.arange(1, U.shape[1] + 1, device=U.device, dtype=U.dtype)
        rho = (s - css / ks > 0).sum(dim=1, keepdim=True) - 1               # (the condition holds on a prefix)
        tau = css.gather(1, rho) / (rho + 1).to(U.dtype)
        return (U - tau).clamp_min_(0.0)

    idx = torch.as_tensor(m.stats["init_index"], device="cuda")
    steps = m.stats["steps"]

    def replay():
        B = torch.zeros((k, n), device="cuda")
        B[torch.arange(k, device="cuda"), idx] = 1.0
        A = torch.full((n, k), 1.0 / k, device="cuda")
        Q = K @ B.t()
        f = None
        for s in steps:
            M = B @ Q
            inv_L = 1.0 / float(torch.linalg.eigvalsh(M.double())[-1])
            for _ in range(s["inner"]):
                A = project(A - inv_L * (A @ M - Q))
            if s["accepted"]:
                S = A.t() @ A
                G = (S @ B - A.t()) @ K
                B = project(B - s["mu"] * G)
                Q = K @ B.t()
            f = trK - 2.0 * float((A.double() * Q.double()).sum()) + float(((A.t() @ A).double() * (B @ Q).double()).sum())
        return A, B, f

    replay()
    t_ms, (At, Bt, ft) = timed(replay)
    res.update(torch_replay_ms=t_ms, torch_replay_ms_per_iteration=t_ms / len(steps), torch_f_over_trK=ft / trK,
               model_f_over_trK=m.data["objective"] / m.data["trK"],
               model_ms_per_iteration=(st["ms_total"] - st["ms_gram"]) / its)

    # ---- the two operators alone, on operands of the size of the last iteration
    Bd = torch.from_numpy(m.data["weights"]).cuda()
    G = (torch.randn((k, n), generator=g, device="cuda") * 1e-3)
    fn = lambda: engine.simplex_rows(ctx, Bd, G, 1.0)
    fn()
    rows_ms = [timed(fn)[0] for _ in range(ROUNDS)]
    tfn = lambda: project(Bd - 1.0 * G)
    tfn()
    rows_t = [timed(tfn)[0] for _ in range(ROUNDS)]
    Ad = torch.from_numpy(m.data["scores"]).cuda()
    Qd = (K @ Bd.t()).contiguous()
    M = (Bd @ Qd).double().cpu().numpy()
    inv_L = 0.99 / float(np.linalg.eigvalsh(0.5 * (M + M.T))[-1])
    fn = lambda: engine.simplex_pg(ctx, Ad, Qd, M, inv_L, 10)
    fn()
    pg_ms = [timed(fn)[0] for _ in range(ROUNDS)]
    Mt = torch.from_numpy(M).float().cuda()

    def tpg():
        a = Ad
        for _ in range(10):
            a = project(a - inv_L * (a @ Mt - Qd))
        return a

    tpg()
    pg_t = [timed(tpg)[0] for _ in range(ROUNDS)]
    res.update(simplex_rows_ms_median=float(np.median(rows_ms)), torch_rows_ms_median=float(np.median(rows_t)),
               simplex_pg10_ms_median=float(np.median(pg_ms)), torch_pg10_ms_median=float(np.median(pg_t)))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(int(args[1]), int(args[2]), int(args[3]))), flush=True)
        sys.exit(0)
    shapes = []
    for n, p, k in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(p), str(k)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"shape ({n}, {p}, {k}) ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = dict(probe="aa", shapes=shapes)
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
