"""The Lloyd solver of weather-regime clustering (engine.kmeans_lloyd, csrc/eofx_kmeans.hpp; xeofs_amd.single.KMeans) timed on a
score panel of n = 10000 rows with R = 50 restarts at (q, k) = (14, 4) -- the shape of Michelangeli et al. (1995) -- and at the
limits (q, k) = (32, 32), against a torch-composed Lloyd loop from the same k-means++ seeds on the same device.
Every shape runs in a fresh child process under its own time limit, and a child that fails ends the probe.  The panel: k
Gaussian blobs three standard deviations apart in q dimensions, made on the device.  A warm-up call first, then ROUNDS calls of
at most MAX_ITER iterations between device synchronisations: the median.  The torch loop handles all restarts at once
(torch.cdist, argmin, a float64 index_add_ for the sums, bincount for the counts; an empty cluster keeps its centroid) and runs
the number of iterations the slowest restart of the solver took, with no test for convergence -- that test would cost it a
synchronisation per iteration.  A second torch loop forms the sums as a batched float64 product with the one-hot membership
instead of the scatter (index_add_ serialises on few destinations: at k = 4 it is most of that loop's time).  Beside the two timings: the iterations per restart, the share of labels on which the two
agree for the best restart, and the seeding time on the host.  Prints one JSON line; `--out FILE` also writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10000, 14, 4, 50), (10000, 32, 32, 50)]            # n, q, k, R
ROUNDS = 5
MAX_ITER = 300
CHILD_LIMIT_S = 200


def child(n, q, k, R):
    import numpy as np
    import torch

    from xeofs_amd import engine
    from xeofs_amd.single.kmeans import kmeanspp_seeds

    ctx = engine.default_context(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 3.0 * torch.randn((k, q), generator=g, device="cuda") / (2.0 ** 0.5)
    S = (centres[torch.randint(k, (n,), generator=g, device="cuda")] + torch.randn((n, q), generator=g, device="cuda")).contiguous()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    t0 = time.perf_counter()
    idx = kmeanspp_seeds(S.cpu().numpy(), k, R, 0)
    seed_ms = (time.perf_counter() - t0) * 1e3
    C0 = S[torch.as_tensor(idx, device="cuda")].contiguous()          # R x k x q

    solve = lambda: engine.kmeans_lloyd(ctx, S, C0, MAX_ITER)
    solve()                                                           # warm-up
    runs = [timed(solve) for _ in range(ROUNDS)]
    ms = [r[0] for r in runs]
    res = runs[0][1]
    iters = res["iters"].cpu().numpy()
    T = int(iters.max())
    rows = torch.arange(R, device="cuda")[:, None] * k                # (restart r owns the clusters r k .. r k + k - 1)

    S64R = S.double().repeat(R, 1)                                    # (made once: the loop does not pay for it)

    def torch_lloyd():
        C = C0.clone()
        for _ in range(T):
            lab = torch.cdist(S[None].expand(R, n, q), C).argmin(dim=2)                 # R x n
            flat = (lab + rows).reshape(-1)
            sums = torch.zeros((R * k, q), dtype=torch.float64, device="cuda").index_add_(0, flat, S64R)
            cnt = torch.bincount(flat, minlength=R * k)
            mean = (sums / cnt.clamp_min(1)[:, None]).float().reshape(R, k, q)
            C = torch.where((cnt > 0).reshape(R, k, 1), mean, C)
        d = torch.cdist(S[None].expand(R, n, q), C)
        md, lab = d.min(dim=2)
        return lab, (md.double() ** 2).sum(dim=1)

    best_of = lambda r: int(r["inertia"].argmin())
    torch_lloyd()
    truns = [timed(torch_lloyd) for _ in range(ROUNDS)]
    tms = [r[0] for r in truns]
    tlab, tin = truns[0][1]

    S64 = S.double()

    def torch_onehot():
        # the same loop with the sums as a batched float64 product with the one-hot membership (no scatter)
        C = C0.clone()
        for _ in range(T):
            lab = torch.cdist(S[None].expand(R, n, q), C).argmin(dim=2)
            oh = torch.nn.functional.one_hot(lab, k).to(torch.float64)                  # R x n x k
            sums = oh.transpose(1, 2) @ S64                                             # R x k x q
            cnt = oh.sum(dim=1)                                                         # R x k
            C = torch.where((cnt > 0)[:, :, None], (sums / cnt.clamp_min(1.0)[:, :, None]).float(), C)
        return torch.cdist(S[None].expand(R, n, q), C).argmin(dim=2)

    torch_onehot()
    oruns = [timed(torch_onehot) for _ in range(ROUNDS)]
    oms = [r[0] for r in oruns]
    best = int(res["inertia"].argmin())
    out = dict(n=n, q=q, k=k, R=R, rounds=ROUNDS, max_iter=MAX_ITER, solver_ms_median=float(np.median(ms)), solver_ms_all=ms,
               torch_ms_median=float(np.median(tms)), torch_ms_all=tms, torch_iterations=T,
               speedup=float(np.median(tms) / np.median(ms)), torch_onehot_ms_median=float(np.median(oms)), torch_onehot_ms_all=oms,
               speedup_onehot=float(np.median(oms) / np.median(ms)),
               onehot_labels_agree=float((oruns[0][1][best_of(res)] == res["labels"][best_of(res)]).float().mean()), iterations_min=int(iters.min()), iterations_max=T,
               iterations_sum=int(iters.sum()), converged=int(res["converged"].sum()), seed_ms=seed_ms,
               solver_us_per_restart_iteration=float(1e3 * np.median(ms) / max(1, int(iters.sum()))),
               best_restart=best, best_inertia=float(res["inertia"][best]), torch_inertia_of_it=float(tin[best]),
               labels_agree=float((tlab[best] == res["labels"][best]).float().mean()))
    again = solve()
    out["rerun_bit_equal"] = bool(all(torch.equal(res[key], again[key]) for key in res))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(*(int(a) for a in args[1:5]))), flush=True)
        sys.exit(0)
    shapes = []
    for shape in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in shape],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"shape {shape} ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = dict(probe="kmeans", shapes=shapes)
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
