"""The three operators of spectral EOF analysis (engine.blockxform, engine.rowgram, engine.slabmul; csrc/eofx_spectral.hpp) and a
whole SpectralEOF.fit, timed at n = 2000 samples, p = 129600 grid points, n_fft = 256 with the default overlap (14 blocks, 129
frequencies) and at a quarter of the bench's grid with the bench's length (n = 10000, p = 259200: 77 blocks), each beside the
library route on the SAME tensors:

    blockxform   T.unfold(1, n_fft, hop) @ B^T, then the transposing copy into [ncoef][nblk][p] -- the overlapped blocks and
                 the untransposed result are both materialised
    rowgram      torch.bmm(R, R^T) in float32 (the library has no float64 accumulation over float32 operands)
    slabmul      torch.bmm(W, R)

Every shape runs in a fresh child process under its own time limit, and a child that fails ends the probe.  Per operator: a
warm-up call (code objects, the arena, the library's choice of algorithm), then ROUNDS calls, each between device
synchronisations; median and minimum.  Achieved TFLOP/s of blockxform = 2 ncoef n_fft nblk p / t beside the 103.0 TF that
profiles/pairmin_probe.json records for the same tile in the pairwise-minimum kernel; rowgram and slabmul are bound by
reading Q once, so theirs is the achieved TB/s = 4 nb r p / t.  The fit is timed once after a warm-up fit at a small size, from
a host array (the upload and the preprocessing are part of it); its own split is in `fit_stats`.  The outputs of the two
routes are compared.  Prints one JSON line; `--out FILE` also writes it there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2000, 129600, 256, True), (10000, 259200, 256, False)]            # n, p, n_fft, whether a whole fit is timed too
ROUNDS = 5
N_MODES = 3
CHILD_LIMIT_S = 280
PAIRMIN_TF, MFMA_F32_PEAK_TF = 103.0, 155.0


def child(n, p, n_fft, with_fit):
    import numpy as np
    import torch

    import xeofs_amd as xe
    from xeofs_amd import engine
    from xeofs_amd.single.spectral_eof import block_count, coefficient_matrix

    ctx = engine.default_context(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    hop = n_fft - n_fft // 2
    nblk = block_count(n, n_fft, n_fft // 2)
    nfreq = n_fft // 2 + 1
    T = torch.empty((p, n), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 28) // n)
    for a in range(0, p, step):                                     # (filled in blocks: the generator's temporaries stay small)
        T[a:a + step].normal_(generator=g)
    B = torch.from_numpy(coefficient_matrix(n_fft, "hamming")).cuda()
    ncoef = B.shape[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def rounds(fn):
        fn()                                                        # warm-up
        ms = [timed(fn)[0] for _ in range(ROUNDS)]
        return float(np.median(ms)), min(ms), ms

    res = dict(n=n, p=p, n_fft=n_fft, hop=hop, nblk=nblk, nfreq=nfreq, ncoef=ncoef, rounds=ROUNDS)
    # ---- blockxform
    Q = torch.empty((ncoef, nblk, p), dtype=torch.float32, device="cuda")
    med, mn, ms = rounds(lambda: engine.blockxform(ctx, T, B, hop, nblk, out=Q))
    flops = 2.0 * ncoef * n_fft * nblk * p
    tf = flops / (med * 1e-3) / 1e12
    res.update(blockxform_ms_median=med, blockxform_ms_min=mn, blockxform_ms_all=ms, blockxform_flops=flops, blockxform_TFLOPs=tf,
               blockxform_over_pairmin=tf / PAIRMIN_TF, blockxform_over_mfma_peak=tf / MFMA_F32_PEAK_TF,
               blockxform_bytes_min=4.0 * (p * n + ncoef * nblk * p))
    lib = lambda: (T.unfold(1, n_fft, hop)[:, :nblk] @ B.t()).permute(2, 1, 0).contiguous()
    medl, mnl, msl = rounds(lib)
    Ql = lib()
    res.update(torch_unfold_matmul_ms_median=medl, torch_unfold_matmul_ms_min=mnl, torch_unfold_matmul_ms_all=msl,
               blockxform_speedup_over_torch=medl / med,
               blockxform_largest_difference_over_largest_value=float((Ql - Q).abs().max() / Q.abs().max()))
    del Ql
    # ---- rowgram
    R = Q.view(nfreq, 2 * nblk, p)
    G = torch.empty((nfreq, 2 * nblk, 2 * nblk), dtype=torch.float64, device="cuda")
    med, mn, ms = rounds(lambda: engine.rowgram(ctx, R, out=G))
    rbytes = 4.0 * nfreq * 2 * nblk * p
    res.update(rowgram_ms_median=med, rowgram_ms_min=mn, rowgram_ms_all=ms, rowgram_TBps=rbytes / (med * 1e-3) / 1e12,
               rowgram_flops=2.0 * nfreq * (2 * nblk) ** 2 * p)
    libg = lambda: torch.bmm(R, R.transpose(1, 2))
    medl, mnl, msl = rounds(libg)
    res.update(torch_bmm_gram_ms_median=medl, torch_bmm_gram_ms_min=mnl, torch_bmm_gram_ms_all=msl, rowgram_speedup_over_torch=medl / med,
               rowgram_largest_difference_over_largest_value=float((libg().double() - G).abs().max() / G.abs().max()))
    # ---- slabmul
    W = torch.randn((nfreq, 2 * N_MODES, 2 * nblk), generator=g, device="cuda")
    O = torch.empty((nfreq, 2 * N_MODES, p), dtype=torch.float32, device="cuda")
    med, mn, ms = rounds(lambda: engine.slabmul(ctx, W, R, out=O))
    res.update(slabmul_ms_median=med, slabmul_ms_min=mn, slabmul_ms_all=ms, slabmul_TBps=rbytes / (med * 1e-3) / 1e12)
    libs = lambda: torch.bmm(W, R)
    medl, mnl, msl = rounds(libs)
    res.update(torch_bmm_modes_ms_median=medl, torch_bmm_modes_ms_min=mnl, torch_bmm_modes_ms_all=msl, slabmul_speedup_over_torch=medl / med,
               slabmul_largest_difference_over_largest_value=float((libs() - O).abs().max() / O.abs().max()))
    del Q, R, G, W, O
    # ---- the whole fit
    if with_fit:
        rng = np.random.default_rng(0)
        small = rng.standard_normal((600, 4096)).astype(np.float32)
        fit = lambda X: xe.single.SpectralEOF(n_modes=N_MODES, n_fft=n_fft).fit(
            xe.DataArray(X, ("time", "x"), {"time": np.arange(X.shape[0]), "x": np.arange(X.shape[1])}), dim="time")
        fit(small)                                                   # warm-up: every code path of the fit
        X = np.ascontiguousarray(T.t().cpu().numpy())
        del T
        torch.cuda.empty_cache()
        ms_fit, m = timed(lambda: fit(X))
        res.update(fit_ms=ms_fit, fit_stats={k: (float(v) if isinstance(v, float) else int(v)) for k, v in m.stats.items()})
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(child(int(args[1]), int(args[2]), int(args[3]), args[4] == "1")), flush=True)
        sys.exit(0)
    shapes = []
    for n, p, n_fft, with_fit in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(p), str(n_fft), "1" if with_fit else "0"],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"shape ({n}, {p}, {n_fft}) ran past its limit of {CHILD_LIMIT_S} s", file=sys.stderr, flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr, flush=True)
            sys.exit(r.returncode)      # nothing more is started on the device after a failed child
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr, flush=True)
    out = dict(probe="spectral", pairmin_TF=PAIRMIN_TF, mfma_f32_peak_TF=MFMA_F32_PEAK_TF, shapes=shapes)
    line = json.dumps(out)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
