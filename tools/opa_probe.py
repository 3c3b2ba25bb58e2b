"""Lag-summed covariance of optimal persistence analysis (engine.lagcov, csrc/eofx_lagcov.hpp) against the plain device
formulation -- tau_max + 1 float64 torch.matmul products of shifted windows -- at (n, q, T) = (10000, 100, 50) and
(20000, 256, 200): interleaved rounds in one process, median and minimum of each, and the largest difference of the two
results relative to the largest entry.  With `--fit`, also one default OPA(n_modes=10, tau_max=50, n_pca_modes=100) fit of a
10000 x 100000 field made on the device and the share of it spent outside the inner PCA.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import xeofs_amd as xe  # noqa: E402
from xeofs_amd import engine  # noqa: E402
from xeofs_amd.single.opa import opa_lag_weights  # noqa: E402

SHAPES = [(10000, 100, 50), (20000, 256, 200)]
ROUNDS = 7


def matmul_form(S64, w):
    n = S64.shape[0]
    M = torch.zeros((S64.shape[1],) * 2, dtype=torch.float64, device=S64.device)
    for tau in range(len(w)):
        M += float(w[tau]) * (S64[:n - tau].T @ S64[tau:])
    return M


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def probe(ctx, n, q, T):
    g = torch.Generator(device="cuda").manual_seed(0)
    S = torch.randn((n, q), generator=g, device="cuda", dtype=torch.float32)
    S64 = S.to(torch.float64)
    w = opa_lag_weights(n, T)
    a = engine.lagcov(ctx, S, w)                    # warm-up of both (code objects, arena, library handles)
    b = matmul_form(S64, w)
    diff = float((a - b).abs().max() / b.abs().max())
    ours, theirs = [], []
    for _ in range(ROUNDS):
        ours.append(timed(lambda: engine.lagcov(ctx, S, w))[0])
        theirs.append(timed(lambda: matmul_form(S64, w))[0])
    return dict(n=n, q=q, tau_max=T, route="fused" if T + 1 <= engine.LAGCOV_FUSE_NTAU else "written",
                lagcov_ms_median=float(np.median(ours)), lagcov_ms_min=min(ours),
                matmul_ms_median=float(np.median(theirs)), matmul_ms_min=min(theirs),
                speedup_median=float(np.median(theirs) / np.median(ours)), max_rel_diff=diff)


def fit_share(n=10000, P=100000):
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn((n, 24), generator=g, device="cuda")
    phi = torch.linspace(0.98, 0.1, 24, device="cuda")
    for t in range(1, n):                           # AR(1) latents of mixed persistence
        z[t] += phi * z[t - 1]
    X = z @ torch.randn((24, P), generator=g, device="cuda") + torch.randn((n, P), generator=g, device="cuda")
    del z
    model = xe.single.OPA(n_modes=10, tau_max=50, n_pca_modes=100, random_state=0)
    ms, _ = timed(lambda: model.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(P)}), dim="time"))
    st = dict(model.stats)
    outside = st["ms_lagcov"] + st["ms_eigen"] + st["ms_project"]
    return dict(n=n, P=P, fit_ms=ms, **st, outside_pca_ms=outside, outside_pca_share_of_algorithm=outside / (outside + st["ms_pca"]),
                decorrelation_time=[float(v) for v in model.data["decorrelation_time"]])


if __name__ == "__main__":
    ctx = engine.default_context(0)
    out = dict(probe="opa", rounds=ROUNDS, shapes=[probe(ctx, *s) for s in SHAPES])
    if "--fit" in sys.argv[1:]:
        out["fit"] = fit_share()
    print(json.dumps(out), flush=True)
