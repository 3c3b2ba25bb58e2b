"""The gap fill of DINEOF (engine.lrfill, csrc/eofx_lrfill.hpp) at 10000 x 129600 with k = 20 and 50 modes and random gaps at
the fractions 0.05 / 0.3 / 0.7: the median of nine call times against the byte-and-flop model of DESIGN.md section 18,

    bytes = n p / 8 (the mask) + 8 n p (1 - (1 - f)^32) (F, read and written in 128 B row segments that hold a gap)
            + 4 k (n nbj + p nbi) (the A and B slabs of every tile, from L2 for the most part: not counted as HBM traffic)
    flops = 2 n p k (every 32 x 32 block holds a gap at these fractions)
    model = max(bytes / 6.3 TB/s, flops / 155 TFLOP/s)      (MI355X: achievable HBM rate, exact-float32 matrix-core rate)

and `engine.gap_mask` of the same field against n p 4 bytes at 6.3 TB/s.

Every case is one step: a fresh child process (`--case I`) under its own time limit of STEP_SECONDS.  A step that fails or
runs out of time ends the probe -- nothing is tried again and no later step starts.  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

N, P = 10000, 129600
CASES = [(k, f) for k in (20, 50) for f in (0.05, 0.3, 0.7)]
ROUNDS = 9
STEP_SECONDS = 150
HBM, F32_MATRIX = 6.3e12, 155e12


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def probe(k, f):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    from xeofs_amd import engine

    ctx = engine.default_context(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    F = torch.randn((N, P), generator=g, device="cuda", dtype=torch.float32)
    for r0 in range(0, N, 1000):                      # gaps as NaNs, by row blocks (no full-size temporary)
        blk = F[r0:r0 + 1000]
        blk[torch.rand(blk.shape, generator=g, device="cuda") < f] = float("nan")
    t_mask = []
    for _ in range(ROUNDS + 1):                       # (the first call is the warm-up)
        ms, (bits, gaps) = timed(torch, lambda: engine.gap_mask(ctx, F))
        t_mask.append(ms)
    torch.nan_to_num_(F, nan=0.0)
    A = torch.randn((N, k), generator=g, device="cuda", dtype=torch.float32)
    B = torch.randn((P, k), generator=g, device="cuda", dtype=torch.float32)
    t_fill, sums = [], None
    for _ in range(ROUNDS + 1):
        ms, sums = timed(torch, lambda: engine.lrfill(ctx, F, bits, A, B))
        t_fill.append(ms)
    assert sums[0] == gaps
    seg = 1.0 - (1.0 - f) ** 32
    nbytes = N * P / 8 + 8.0 * N * P * seg
    flops = 2.0 * N * P * k
    model_ms = max(nbytes / HBM, flops / F32_MATRIX) * 1e3
    med = float(np.median(t_fill[1:]))
    mask_model_ms = 4.0 * N * P / HBM * 1e3
    mask_med = float(np.median(t_mask[1:]))
    return dict(n=N, p=P, k=k, gap_fraction=f, gaps=gaps, lrfill_ms_median=med, lrfill_ms_min=min(t_fill[1:]),
                model_ms=model_ms, model_bytes_ms=nbytes / HBM * 1e3, model_flops_ms=flops / F32_MATRIX * 1e3,
                fraction_of_model=model_ms / med, gap_mask_ms_median=mask_med, gap_mask_model_ms=mask_model_ms,
                gap_mask_fraction_of_model=mask_model_ms / mask_med)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        print(json.dumps(probe(*CASES[int(sys.argv[2])])), flush=True)
        sys.exit(0)
    cases = []
    for i in range(len(CASES)):
        step = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True,
                              timeout=STEP_SECONDS)       # (TimeoutExpired kills the child and ends the probe)
        if step.returncode != 0:
            sys.stderr.write(step.stdout + step.stderr)
            sys.exit(f"case {i} ended with status {step.returncode}: the probe stops here")
        cases.append(json.loads(step.stdout.strip().splitlines()[-1]))
        print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
    print(json.dumps(dict(probe="lrfill", rounds=ROUNDS, step_seconds=STEP_SECONDS, cases=cases)), flush=True)
