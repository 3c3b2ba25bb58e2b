"""Extended EOF at scale (xeofs_amd.single.ExtendedEOF, csrc/eofx_lag.hpp): one fit of a field made on the GPU, and the
per-product time of the lag operator next to the plain panel product of the same width on the same matrix.
Prints one JSON line.  Environment: N, NLAT, NLON (default: the config-4 field, 10000 x 360 x 2880 = 1 036 800 features),
E (embedding, 10), TAU (1), K (n_modes, 10), REPS (5)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import xeofs_amd as xe  # noqa: E402
from xeofs_amd import engine  # noqa: E402
from xeofs_amd.single.eeof import LagOps  # noqa: E402

n, nlat, nlon = int(os.environ.get("N", 10000)), int(os.environ.get("NLAT", 360)), int(os.environ.get("NLON", 2880))
E, tau, k, reps = int(os.environ.get("E", 10)), int(os.environ.get("TAU", 1)), int(os.environ.get("K", 10)), int(os.environ.get("REPS", 5))
dev = torch.device("cuda:0")
sync = torch.cuda.synchronize

X = bench.make_field(n, nlat, nlon, 0, nlat * nlon, dev).reshape(n, nlat * nlon)
sync()
field_gb = X.numel() * 4 / 1e9
ctx = engine.default_context(0)
free0, _ = torch.cuda.mem_get_info()
t0 = time.perf_counter()
m = xe.single.ExtendedEOF(n_modes=k, tau=tau, embedding=E, random_state=0).fit(xe.DataArray(X, dims=("time", "x")), "time")
sync()
fit_s = time.perf_counter() - t0
free1, _ = torch.cuda.mem_get_info()

# per-product times on the model's resident matrix: lag operator (panel width L = k + 10 rounded to 32) against the plain
# panel product of width E L
mat = m.data["input_data"]
mean, _ = engine.lag_stats(ctx, mat, tau, E)
ops = LagOps(ctx, mat, tau, E, mean)
L = engine.panel_width(k + 10)
prec = ctx.precision[0]
Zn = torch.randn((ops.n_pad, L), device=dev)
Ye = torch.randn((ops.p_pad, L), device=dev)
W = torch.randn((mat.n_pad, E * L), device=dev)
Yw = torch.randn((mat.p_pad, E * L), device=dev)


def timed(fn):
    fn()
    sync()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return 1e3 * (time.perf_counter() - t) / reps


res = dict(probe="eeof", n=n, p=nlat * nlon, embedding=E, tau=tau, n_modes=k, field_gb=round(field_gb, 2),
           fit_s=round(fit_s, 3), mem_growth_gb=round((free0 - free1) / 1e9, 2),
           mem_growth_over_field=round((free0 - free1) / 1e9 / field_gb, 2),
           embedded_copy_gb=round(field_gb * E, 1), L=L,
           lag_tmul_ms=round(timed(lambda: engine.lag_tmul(ctx, mat, tau, E, mean, Zn, prec=prec)), 3),
           panel_tmul_wide_ms=round(timed(lambda: engine.panel_tmul(ctx, mat, W, prec=prec)), 3),
           lag_mul_ms=round(timed(lambda: engine.lag_mul(ctx, mat, tau, E, mean, Ye, prec=prec)), 3),
           panel_mul_wide_ms=round(timed(lambda: engine.panel_mul(ctx, mat, Yw, prec=prec)), 3),
           singular_values=[round(float(v), 4) for v in m.data["norms"][:3]])
res["tmul_ratio"] = round(res["lag_tmul_ms"] / res["panel_tmul_wide_ms"], 3)
res["mul_ratio"] = round(res["lag_mul_ms"] / res["panel_mul_wide_ms"], 3)
print(json.dumps(res), flush=True)
