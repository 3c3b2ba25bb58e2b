"""Low-pass covariance of low-frequency component analysis (engine.lowpass_cov, csrc/eofx_lowpass.hpp) against the plain
device formulation -- the same detrend, mirrored pad and 2 h + 1 shifted float64 slices, then one torch.matmul -- at
(n, q, h) = (10000, 100, 16), (10000, 100, 60) and (20000, 256, 180): interleaved rounds in one process, median and minimum
of each, and the largest difference of the two results relative to the largest entry.  With `--fit`, also a default
LFCA(n_modes=10, cutoff=40, n_pca_modes=100) fit of a 10000 x 100000 field made on the device, run twice (the first loads
code objects), and the share of the second spent outside the inner PCA.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import xeofs_amd as xe  # noqa: E402
from xeofs_amd import engine  # noqa: E402
from xeofs_amd.single.lfca import lanczos_weights, linear_trend  # noqa: E402

SHAPES = [(10000, 100, 16), (10000, 100, 60), (20000, 256, 180)]
ROUNDS = 7


def torch_form(S64, w, trend):
    """float64 torch doing the same filter plus matmul"""
    n = S64.shape[0]
    h = len(w) - 1
    t = torch.arange(n, dtype=torch.float64, device=S64.device)[:, None]
    T = trend[0][None, :] + trend[1][None, :] * t
    D = S64 - T
    Dp = torch.cat([D[1:h + 1].flip(0), D, D[n - 1 - h:n - 1].flip(0)])
    Y = torch.zeros_like(S64)
    for k in range(-h, h + 1):
        Y += float(w[abs(k)]) * Dp[h + k:h + k + n]
    Y += T
    return Y.T @ Y


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def probe(ctx, n, q, h):
    g = torch.Generator(device="cuda").manual_seed(0)
    S = torch.randn((n, q), generator=g, device="cuda", dtype=torch.float32).cumsum(0) * 0.05
    S64 = S.to(torch.float64)
    w = lanczos_weights(max(2.5, h / 1.5), h)
    trend = linear_trend(S.cpu().numpy())
    trend_d = torch.from_numpy(trend).cuda()
    a = engine.lowpass_cov(ctx, S, w, trend)        # warm-up of both (code objects, arena, library handles)
    b = torch_form(S64, w, trend_d)
    diff = float((a - b).abs().max() / b.abs().max())
    ours, theirs = [], []
    for _ in range(ROUNDS):
        ours.append(timed(lambda: engine.lowpass_cov(ctx, S, w, trend))[0])
        theirs.append(timed(lambda: torch_form(S64, w, trend_d))[0])
    return dict(n=n, q=q, h=h, lowpass_cov_ms_median=float(np.median(ours)), lowpass_cov_ms_min=min(ours),
                torch_ms_median=float(np.median(theirs)), torch_ms_min=min(theirs),
                speedup_median=float(np.median(theirs) / np.median(ours)), max_rel_diff=diff)


def fit_share(n=10000, P=100000):
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn((n, 24), generator=g, device="cuda")
    phi = torch.linspace(0.98, 0.1, 24, device="cuda")
    for t in range(1, n):                           # AR(1) latents of mixed persistence
        z[t] += phi * z[t - 1]
    X = z @ torch.randn((24, P), generator=g, device="cuda") + torch.randn((n, P), generator=g, device="cuda")
    del z
    field = xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(P)})
    first, _ = timed(lambda: xe.single.LFCA(n_modes=10, cutoff=40, n_pca_modes=100, random_state=0).fit(field, dim="time"))
    model = xe.single.LFCA(n_modes=10, cutoff=40, n_pca_modes=100, random_state=0)
    ms, _ = timed(lambda: model.fit(field, dim="time"))
    st = dict(model.stats)
    outside = st["ms_lowpass"] + st["ms_eigen"] + st["ms_project"]
    return dict(n=n, P=P, first_fit_ms=first, fit_ms=ms, **st, outside_pca_ms=outside, outside_pca_share_of_algorithm=outside / (outside + st["ms_pca"]),
                low_frequency_ratio=[float(v) for v in model.data["low_frequency_ratio"]])


if __name__ == "__main__":
    ctx = engine.default_context(0)
    out = dict(probe="lfca", rounds=ROUNDS, shapes=[probe(ctx, *s) for s in SHAPES])
    if "--fit" in sys.argv[1:]:
        out["fit"] = fit_share()
    print(json.dumps(out), flush=True)
