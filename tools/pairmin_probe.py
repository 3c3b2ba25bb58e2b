"""The pairwise-minimum operator of the teleconnectivity map (engine.pairmin, csrc/eofx_pairmin.hpp), timed at a small size
first (n = 500 samples, p = 16384 grid points: trouble shows early) and at the bench's grid (n = 2000, p = 129600: 6.7e13 flops),
beside a chunked torch.matmul + min on the SAME tensor -- the only way to the same map without the kernel: every CHUNK x p block
of the correlation matrix is written, scaled, masked on its diagonal and read again for the row minimum.
Every shape runs in a fresh child process under its own time limit, and a child that fails ends the probe.  The operator: a
series-major centred panel T [p x n] on the device, w = 1 / |T_j|; a warm-up call first (code objects, the arena), then ROUNDS
calls, each between device synchronisations; median and minimum, achieved TFLOP/s = 2 n p^2 / t beside the 98.8 TF that
profiles/eot_probe.json records for the identical tile of the quadratic-form kernel, the 122 TF of an untuned LDS-tiled
float32-MFMA GEMM and the 155 TF peak of the instruction.  The baseline is timed once after a warm-up on one chunk, and the two
results are compared: the share of equal partners and the largest difference of the minima (the baseline's sums run in
another order).  Prints one JSON line; `--out FILE` also writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(500, 16384), (2000, 129600)]            # n, p
ROUNDS = 3
CHUNK = 4096                                       # rows of the correlation matrix the baseline holds at a time
CHILD_LIMIT_S = 240
COLQUAD_TF, GEMM_UNTUNED_TF, MFMA_F32_PEAK_TF = 98.8, 122.0, 155.0


def child(n, p):
    import numpy as np
    import torch

    from xeofs_amd import engine

    ctx = engine.default_context(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    T = torch.empty((p, n), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 28) // n)
    L = torch.randn((6, n), generator=g, device="cuda")
    for a in range(0, p, step):                                     # (filled in blocks: the generator's temporaries stay small)
        T[a:a + step].normal_(generator=g)
        # six planted series on top of the noise, so that the seesaws are real ones
        T[a:a + step] += (torch.randn((T[a:a + step].shape[0], 6), generator=g, device="cuda")
                          * torch.linspace(1.5, 0.3, 6, device="cuda")) @ L
        T[a:a + step] -= T[a:a + step].mean(dim=1, keepdim=True)
    w = (1.0 / T.double().pow(2).sum(dim=1).sqrt()).float()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    flops = 2.0 * n * p * p
    res = dict(n=n, p=p, rounds=ROUNDS, flops=flops)
    out = (torch.empty(p, dtype=torch.float32, device="cuda"), torch.empty(p, dtype=torch.int32, device="cuda"))
    fn = lambda: engine.pairmin(ctx, T, w, out=out)
    fn()
    first = (out[0].clone(), out[1].clone())
    ms = [timed(fn)[0] for _ in range(ROUNDS)]
    res["two_runs_equal"] = bool(torch.equal(first[0].view(torch.int32), out[0].view(torch.int32)) and torch.equal(first[1], out[1]))
    med = float(np.median(ms))
    tf = flops / (med * 1e-3) / 1e12
    res.update(pairmin_ms_median=med, pairmin_ms_min=min(ms), pairmin_ms_all=ms, achieved_TFLOPs=tf,
               over_colquad=tf / COLQUAD_TF, over_untuned_gemm=tf / GEMM_UNTUNED_TF, over_mfma_peak=tf / MFMA_F32_PEAK_TF)

    def baseline(rows):
        rmin = torch.empty(p, dtype=torch.float32, device="cuda")
        partner = torch.empty(p, dtype=torch.int64, device="cuda")
        for lo in range(0, rows, CHUNK):
            hi = min(p, lo + CHUNK)
            R = torch.matmul(T[lo:hi], T.t())
            R.mul_(w[lo:hi, None]).mul_(w[None, :])
            R[torch.arange(hi - lo, device="cuda"), torch.arange(lo, hi, device="cuda")] = float("inf")
            rmin[lo:hi], partner[lo:hi] = torch.min(R, dim=1)
            del R
        return rmin, partner

    baseline(CHUNK)                                                 # warm-up: one chunk
    base_ms, (bmin, bpart) = timed(lambda: baseline(p))
    res.update(torch_chunked_ms=base_ms, torch_chunk_rows=CHUNK, torch_TFLOPs=flops / (base_ms * 1e-3) / 1e12,
               speedup_over_torch=base_ms / med, partners_equal_share=float((bpart == out[1].long()).double().mean()),
               largest_rmin_difference=float((bmin - out[0]).abs().max()))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(int(args[1]), int(args[2]))), flush=True)
        sys.exit(0)
    shapes = []
    for n, p in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(p)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"shape ({n}, {p}) ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = dict(probe="pairmin", colquad_TF=COLQUAD_TF, untuned_gemm_TF=GEMM_UNTUNED_TF, mfma_f32_peak_TF=MFMA_F32_PEAK_TF,
               shapes=shapes)
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
