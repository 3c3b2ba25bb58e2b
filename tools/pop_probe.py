"""PC-space product of principal oscillation pattern analysis (engine.pcmul, csrc/eofx_pcmul.hpp) against the float64 route
it stands beside -- spca.spca_rowmul with its float64 up-conversion of the float32 panel and the down-conversion of the
result, which is what that route costs -- on the same operands at (rows, a, b) = (10000, 256, 512), (10000, 1024, 2048) and
(1036800, 100, 200): interleaved rounds in one process, median and minimum of each, and the largest difference of the two
results relative to the largest entry.  With `--fit`, also one default POP(n_pca_modes=100) fit of a 10000 x 100000 field made
on the device, split as model.stats splits it.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import xeofs_amd as xe  # noqa: E402
from xeofs_amd import engine, spca  # noqa: E402

SHAPES = [(10000, 256, 512), (10000, 1024, 2048), (1036800, 100, 200)]
ROUNDS = 7


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def probe(ctx, rows, a, b):
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((rows, a), generator=g, device="cuda", dtype=torch.float32)
    M = torch.randn((a, b), generator=g, device="cuda", dtype=torch.float64)

    def ours():
        return engine.pcmul(ctx, X, M, torch.float32)

    def theirs():
        return spca.spca_rowmul(ctx, X.to(torch.float64), M).to(torch.float32)

    y, z = ours(), theirs()                         # warm-up of both (code objects, allocator)
    diff = float((y - z).abs().max() / z.abs().max())
    del y, z
    t_ours, t_theirs = [], []
    for _ in range(ROUNDS):
        t_ours.append(timed(ours)[0])
        t_theirs.append(timed(theirs)[0])
    return dict(rows=rows, a=a, b=b, pcmul_ms_median=float(np.median(t_ours)), pcmul_ms_min=min(t_ours),
                rowmul_ms_median=float(np.median(t_theirs)), rowmul_ms_min=min(t_theirs),
                speedup_median=float(np.median(t_theirs) / np.median(t_ours)), max_rel_diff=diff,
                tflops_pcmul_median=2.0 * rows * a * b / np.median(t_ours) / 1e9)


def fit_split(n=10000, P=100000):
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn((n, 24), generator=g, device="cuda")
    phi = torch.linspace(0.98, 0.1, 24, device="cuda")
    for t in range(1, n):                           # AR(1) latents of mixed persistence
        z[t] += phi * z[t - 1]
    X = z @ torch.randn((24, P), generator=g, device="cuda") + torch.randn((n, P), generator=g, device="cuda")
    del z
    model = xe.single.POP(n_pca_modes=100, random_state=0)
    ms, _ = timed(lambda: model.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(P)}), dim="time"))
    st = dict(model.stats)
    outside = st["ms_lagcov"] + st["ms_eigen"] + st["ms_project"]
    return dict(n=n, P=P, fit_ms=ms, **st, outside_pca_ms=outside,
                outside_pca_share_of_algorithm=outside / (outside + st["ms_pca"]),
                n_complex_modes=int((model.data["eigenvalues"].imag != 0).sum()))


def eig_at_limit(q=1024):
    """the host's nonsymmetric eigenproblem at the widest PC space the model takes"""
    rng = np.random.default_rng(0)
    A = rng.standard_normal((q, q)) / np.sqrt(q)
    t0 = time.perf_counter()
    np.linalg.eig(A)
    return dict(q=q, host_eig_ms=(time.perf_counter() - t0) * 1e3)


if __name__ == "__main__":
    ctx = engine.default_context(0)
    out = dict(probe="pop", rounds=ROUNDS, shapes=[probe(ctx, *s) for s in SHAPES], eig=eig_at_limit())
    if "--fit" in sys.argv[1:]:
        out["fit"] = fit_split()
    print(json.dumps(out), flush=True)
