"""Block cross-covariance of multi-view CCA (engine.viewcov, csrc/eofx_viewcov.hpp) against the float64 library product
`Z.double().T @ Z.double()` through torch on the same GPU and the same panel, at n = 5000 with p = 4096 (three views) and
p = 600 (three views): interleaved rounds in one process after a warm-up of both, median and minimum of each, and the largest
difference of the two results on the entries of two different views relative to the largest entry.  The library product
computes the whole Gram matrix and neither centres nor scales; the kernel centres, scales and computes the tiles on or above
the diagonal that hold an entry of two views.

Every shape is one step: a fresh child process (`--shape I`) under its own time limit of STEP_SECONDS.  A step that fails or
runs out of time ends the probe -- nothing is tried again and no later step starts.  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

SHAPES = [(5000, [0, 1301, 1400, 4096]), (5000, [0, 150, 380, 600])]
ROUNDS = 9
STEP_SECONDS = 120


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def probe(n, off):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    from xeofs_amd import engine

    ctx = engine.default_context(0)
    p = off[-1]
    g = torch.Generator(device="cuda").manual_seed(0)
    Z = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float32)
    Z -= Z.mean(dim=0)                                # so that the two results can be held against each other

    def ours():
        return engine.viewcov(ctx, Z, off)

    def theirs():
        Zd = Z.double()
        return Zd.T @ Zd

    a, b = ours(), theirs()                           # warm-up of both (code objects, library algorithm choice, allocator)
    view = torch.from_numpy(np.repeat(np.arange(len(off) - 1), np.diff(off))).cuda()
    cross = view[:, None] != view[None, :]
    diff = float(((a - b / (n - 1)).abs() * cross).max() / (b / (n - 1)).abs().max())
    del a, b
    t_ours, t_theirs = [], []
    for _ in range(ROUNDS):
        t_ours.append(timed(torch, ours)[0])
        t_theirs.append(timed(torch, theirs)[0])
    wanted = float(cross.sum()) / 2                   # entries of two views above the diagonal
    return dict(n=n, p=p, offsets=off, viewcov_ms_median=float(np.median(t_ours)), viewcov_ms_min=min(t_ours),
                library_ms_median=float(np.median(t_theirs)), library_ms_min=min(t_theirs),
                library_over_viewcov_median=float(np.median(t_theirs) / np.median(t_ours)), max_rel_diff=diff,
                wanted_tflops_viewcov_median=2.0 * n * wanted / np.median(t_ours) / 1e9,
                full_tflops_library_median=2.0 * n * p * p / np.median(t_theirs) / 1e9)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        print(json.dumps(probe(*SHAPES[int(sys.argv[2])])), flush=True)
        sys.exit(0)
    shapes = []
    for i in range(len(SHAPES)):
        step = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(i)], capture_output=True, text=True,
                              timeout=STEP_SECONDS)       # (TimeoutExpired kills the child and ends the probe)
        if step.returncode != 0:
            sys.stderr.write(step.stdout + step.stderr)
            sys.exit(f"step {i} ended with status {step.returncode}: the probe stops here")
        shapes.append(json.loads(step.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(probe="viewcov", rounds=ROUNDS, step_seconds=STEP_SECONDS, shapes=shapes)), flush=True)
