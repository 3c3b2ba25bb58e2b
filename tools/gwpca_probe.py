"""Geographically weighted PCA at stated sizes (engine.gwpca, csrc/eofx_gw.hpp): per-stage times, tile pairs visited out of
all, achieved float64 FLOP/s of the covariance stage against the fp64 matrix-core peak (78.6 TF),
device-memory growth, and the numpy restatement's time on a subset of locations, EXTRAPOLATED to all of them.
Prints one JSON line per size.  Sizes (argument, default all): a = 1-degree global grid, p = 32, k = 4, bisquare 1000 km;
b = 2-degree grid, p = 32, gaussian 1000 km (no tile pair can be pruned); c = 2-degree grid, p = 128 (library eigh route)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from xeofs_amd import engine  # noqa: E402

PEAK = 78.6e12
SIZES = {"a": (1.0, 32, 4, "bisquare", 1000.0), "b": (2.0, 32, 4, "gaussian", 1000.0), "c": (2.0, 128, 4, "bisquare", 1000.0)}


def grid(step):
    lat = np.arange(-90 + step / 2, 90, step)
    lon = np.arange(-180 + step / 2, 180, step)
    g0, g1 = np.meshgrid(lat, lon, indexing="ij")
    return np.stack([g1.reshape(-1), g0.reshape(-1)], 1)


def restatement_seconds(X, xy, kernel, bw, k, m):
    lon, lat = np.radians(xy[:, 0]), np.radians(xy[:, 1])
    t0 = time.perf_counter()
    for i in range(m):
        a = np.clip(np.sin((lat - lat[i]) / 2) ** 2 + np.cos(lat[i]) * np.cos(lat) * np.sin((lon - lon[i]) / 2) ** 2, 0, 1)
        u = 6371.0 * 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a)) / bw
        w = np.where(u <= 1, (1 - u ** 2) ** 2, 0.0) if kernel == "bisquare" else np.exp(-0.5 * u ** 2)
        keep = w > 0
        w, x = w[keep], X[keep]
        y = x - (w[:, None] * x).sum(0) / w.sum()
        np.linalg.eigh((w[:, None] * y).T @ y / w.sum())
    return (time.perf_counter() - t0) / m


def run(name):
    step, p, k, kernel, bw = SIZES[name]
    xy = grid(step)
    n = xy.shape[0]
    rng = np.random.default_rng(0)
    X = (rng.normal(size=(n, p)) * np.linspace(3, 0.5, p)).astype(np.float32)
    ctx = engine.default_context(0)
    mat, _ = engine.preprocess(ctx, X, True, False, None, True)
    torch.cuda.synchronize()
    engine.gwpca(ctx, mat, xy, k, bw, "haversine", kernel)          # warm-up (code objects, arena)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    V, ev, tv, st = engine.gwpca(ctx, mat, xy, k, bw, "haversine", kernel)
    wall = time.perf_counter() - t0
    free1, _ = torch.cuda.mem_get_info()
    # covariance work: every visited tile pair is GW_T x GW_T location pairs, each 2 flops per packed augmented entry
    P2a = (p + 1) * (p + 2) // 2
    flops = st["tile_pairs_visited"] * 16 * 16 * P2a * 2.0
    Xp = mat.download().astype(np.float64)
    mat.free()
    m = 40
    per = restatement_seconds(Xp, xy, kernel, bw, k, m)
    out = dict(size=name, n=n, p=p, k=k, kernel=kernel, bandwidth_km=bw, wall_ms=wall * 1e3, **st,
               pruned_fraction=1 - st["tile_pairs_visited"] / st["tile_pairs_total"],
               cov_gflops=flops / max(st["ms_covariance"], 1e-9) / 1e6, cov_fraction_of_fp64_peak=flops / max(st["ms_covariance"], 1e-9) / 1e-3 / PEAK,
               device_mem_growth_mb=(free0 - free1) / 2 ** 20, numpy_restatement_locations=m,
               numpy_restatement_s_extrapolated_to_all=per * n, route="jacobi" if p <= engine.GW_EIG_PMAX else "torch.linalg.eigh")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    for s in (sys.argv[1:] or list(SIZES)):
        run(s)
