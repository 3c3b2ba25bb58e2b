"""SparsePCA at the bench's config-4 shape (10000 x 1 036 800 float32, n_modes=10), phase by phase on the MI355X:
preprocess, QB passes, solver setup, the variable-projection loop (microseconds per iteration, iterations to converge),
the scores pass, device-memory growth, and the float64 numpy restatement on a subsampled width, extrapolated.

    python tools/spca_probe.py [--n 10000] [--nlat 720] [--nlon 1440] [--k 10] [--restate-width 20000]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def restate_loop_seconds(C, k, iters, alpha=1e-3, beta=1e-3):
    """wall time of `iters` iterations of the float64 numpy restatement (non-robust, l1) on C"""
    _, D, Vt = np.linalg.svd(C, full_matrices=False)
    V = Vt.T
    B = V[:, :k].copy()
    d0 = D[0] ** 2
    a2, b2 = alpha * d0, beta * d0
    nu = 1.0 / (d0 + b2)
    VD2 = V * D ** 2
    t0 = time.perf_counter()
    for _ in range(iters):
        U, s, Wt = np.linalg.svd(VD2 @ (Vt @ B), full_matrices=False)
        A = U @ Wt
        G = VD2 @ (Vt @ (A - B)) - b2 * B
        B = np.sign(B + nu * G) * np.maximum(np.abs(B + nu * G) - nu * a2, 0)
        R = (V * D).T - (V * D).T @ B @ A.T
        _ = 0.5 * np.sum(R ** 2) + a2 * np.abs(B).sum() + 0.5 * b2 * np.sum(B ** 2)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--nlat", type=int, default=720)
    ap.add_argument("--nlon", type=int, default=1440)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--restate-width", type=int, default=20000)
    args = ap.parse_args()

    import torch

    import bench
    from xeofs_amd import engine, spca
    from xeofs_amd.preprocessing import Preprocessor

    dev = "cuda:0"
    ctx = engine.default_context()
    P = args.nlat * args.nlon
    X = bench.make_field(args.n, args.nlat, args.nlon, 0, P, dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    out = dict(shape=[args.n, P], n_modes=args.k)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    t_all = time.perf_counter()
    pre = Preprocessor(True, False, False, True, ctx=ctx, in_place=True)
    from xeofs_amd import labelled

    da = labelled.DataArray(X, ("time", "x"))
    mat, out["ms_preprocess"] = timed(lambda: pre.fit_transform(da, "time"))
    Ct, out["ms_qb"] = timed(lambda: spca.spca_compress(ctx, mat, args.k, 10, 1, 1, 0))
    res, out["ms_solve"] = timed(lambda: spca.spca_solve(ctx, Ct, args.k))
    B = res["B"].to(torch.float32).cpu().numpy()
    _, out["ms_scores"] = timed(lambda: engine.project(ctx, mat, B))
    out["ms_fit_wall"] = 1e3 * (time.perf_counter() - t_all)
    out["ms_setup"] = res["ms"]["setup"]
    out["ms_loop"] = res["ms"]["loop"]
    out["n_iter"] = res["n_iter"]
    out["route"] = res["route"]
    l = Ct.shape[1]
    out["us_per_iteration"] = 1e3 * res["ms"]["loop"] / res["n_iter"]
    byts = P * (8 * l + 16 * args.k)
    out["bytes_per_iteration"] = byts
    out["achieved_GBps_per_iteration"] = byts / (out["us_per_iteration"] * 1e-6) / 1e9
    out["device_memory_growth_MB"] = (free0 - torch.cuda.mem_get_info()[0]) / 1e6
    out["zeros_in_B"] = float((B == 0).mean())
    # the float64 numpy restatement on a subsampled width, extrapolated linearly in p (LABELLED AS AN EXTRAPOLATION)
    w = min(args.restate_width, P)
    C = Ct[:w].T.contiguous().cpu().numpy()
    it = 20
    sec = restate_loop_seconds(C, args.k, it)
    out["numpy_restatement"] = dict(width=w, iterations_timed=it, seconds=sec,
                                    extrapolated_loop_seconds_at_full_width=sec / it * res["n_iter"] * P / w,
                                    note="extrapolated, not measured at full width")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
