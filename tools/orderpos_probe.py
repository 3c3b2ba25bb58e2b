"""The rank-order operator of trend EOF analysis (engine.order_positions, csrc/eofx_orderpos.hpp) timed on series-major
panels T [p x n] of n = 10000 samples: p = 129600 and, where HBM holds the panel and its output twice over, p = 1036800.
Every shape runs in a fresh child process under its own time limit, and a child that fails ends the probe: warm-up calls first (code objects, the arena), then ROUNDS calls, each between
device synchronisations; median and minimum.  Beside it, at the width where its int64 indices fit, torch.sort(stable=True,
dim=1) on the same tensor in alternating rounds, and a check that both give the same positions.  Reported with the traffic
floor: a series read once and written once is 2 * 4 * n * p bytes, over the 8.0 TB/s the HBM is specified for and the
6.29 TB/s a float4 copy reaches.  Prints one JSON line; `--out FILE` also writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10000, 129600, True), (10000, 1036800, False)]          # n, p, beside torch.sort
ROUNDS = 5
CHILD_LIMIT_S = 180
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29


def child(n, p, with_torch):
    import numpy as np
    import torch

    from xeofs_amd import engine

    ctx = engine.default_context(0)
    free, _ = torch.cuda.mem_get_info()
    need = 2 * 4 * n * p
    if free < need + (8 << 30):
        return dict(n=n, p=p, skipped=f"needs {need / 1e9:.1f} GB for the panel and its output, {free / 1e9:.1f} GB free")
    g = torch.Generator(device="cuda").manual_seed(0)
    T = torch.empty((p, n), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 28) // n)
    for a in range(0, p, step):                                     # (filled in blocks: the generator's temporaries stay small)
        T[a:a + step].normal_(generator=g)
    scale = torch.rand(p, generator=g, device="cuda", dtype=torch.float64) + 0.5
    z = torch.empty((p, n), dtype=torch.float32, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ours_fn = lambda: engine.order_positions(ctx, T, scale, want="z", out=z)
    for _ in range(2):
        ours_fn()
    res = dict(n=n, p=p, rounds=ROUNDS, bytes_floor=need)
    use_torch = with_torch and torch.cuda.mem_get_info()[0] > (4 + 8 + 16) * n * p + (8 << 30)
    ours, theirs = [], []
    if use_torch:
        torch.sort(T[:step], stable=True, dim=1)
        _, (_, idx) = timed(lambda: torch.sort(T, stable=True, dim=1))
        q = engine.order_positions(ctx, T, want="q")
        res["same_positions_as_torch"] = bool(torch.equal(q, idx.to(torch.int32)))
        del q, idx
    for _ in range(ROUNDS):
        ours.append(timed(ours_fn)[0])
        if use_torch:
            theirs.append(timed(lambda: torch.sort(T, stable=True, dim=1))[0])
    med = float(np.median(ours))
    res.update(orderpos_ms_median=med, orderpos_ms_min=min(ours), achieved_TBs=need / (med * 1e-3) / 1e12,
               floor_ms_at_spec=need / (HBM_SPEC_TBS * 1e12) * 1e3, floor_ms_at_copy_rate=need / (HBM_COPY_TBS * 1e12) * 1e3,
               times_the_copy_rate_floor=med / (need / (HBM_COPY_TBS * 1e12) * 1e3))
    if use_torch:
        tm = float(np.median(theirs))
        res.update(torch_sort_ms_median=tm, torch_sort_ms_min=min(theirs), torch_over_orderpos=tm / med)
    elif with_torch:
        res["torch_sort"] = "not measured: its int64 indices and temporaries do not fit beside the panel"
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(int(args[1]), int(args[2]), args[3] == "1")), flush=True)
        sys.exit(0)
    shapes = []
    for n, p, with_torch in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(p), "1" if with_torch else "0"],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"shape ({n}, {p}) ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = dict(probe="orderpos", hbm_spec_TBs=HBM_SPEC_TBS, hbm_copy_TBs=HBM_COPY_TBS, shapes=shapes)
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
