// eofx_lowpass.hpp -- the low-pass covariance of low-frequency component analysis (Wills et al. 2018; single/lfca.py):
//
//     d(u, j) = S[u, j] - (a_j + b_j u)                                              (the trend is optional: a = b = 0)
//     Y[t, j] = sum_{k = -h .. h} w[|k|] d(refl(t + k), j) + (a_j + b_j t),          R = Y^T Y
//
// (S [n x p] float32; w [h + 1], the trend [2 x p], Y and R float64), refl the mirror of an index about the first and the
// last sample: refl(u) = -u below 0, 2 (n - 1) - u above n - 1.  h <= n - 1, so one reflection lands inside.
//   lowpass_fir_kernel    Y [n x p] float64, written once.  A thread slides the window of 16 outputs of the lag covariance
//                         along the samples (fir16, eofx_lagcov.hpp): one read of S feeds 16 fused multiply-adds, the weights
//                         are read from the symmetric copy wsym[15 + h + k] = w[|k|] padded with 15 zeros on either side
//                         (no bounds test; the products with the padding are exact zeros), and every Y[t, j] is summed
//                         over k ascending from -h.
//   lowpass_gram_kernel   R = Y^T Y of the written panel: one workgroup per row group and PAIR (bi, bj), bi <= bj, of
//                         64-column blocks of Y.  Per row tile of 64 samples the two tiles of Y are staged in LDS
//                         (fir_stage_tile; one when bi == bj); wave w owns rows 16 w .. 16 w + 15 of the 64 x 64 block: four accumulators on the fp64
//                         matrix cores (eofx_mfma64.hpp); on a diagonal pair the 16 x 16 blocks below the diagonal are
//                         skipped.  A workgroup walks its row tiles in ascending order and writes one partial, every
//                         value with gi <= gj together with its mirror image from the same register; f64_reduce_kernel
//                         (eofx_kernels.hpp) sums the partials in a fixed order, so R == R^T bit for bit.
// A route that filtered the tiles in LDS (Y never written) was built and measured slower at every shape: both operands of
// Y^T Y are filtered tiles, so every pair of column blocks repeats the filter of its two blocks, and the 2 h + 1 multiply-adds
// per entry cost more than the one write and read of Y they save (docs/EXPERIMENTS.md).
// LDS of the Gram kernel: 2 x 64 x MFMA64_TILE_LD doubles = 80 KiB: two workgroups of four waves fit the 160 KiB of a CU.
// Float64 throughout, no atomics, the grid a function of the shape alone: two runs are equal bit for bit.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"
#include "eofx_lagcov.hpp"

namespace eofx {

constexpr size_t LOWPASS_LDS_Y = (size_t)2 * FIR_R * MFMA64_TILE_LD * sizeof(double);

// the mirrored sample of u, or -1 where one reflection does not land in 0 .. n - 1 (rows no stored output reads)
__device__ __forceinline__ int64_t lowpass_refl(int64_t u, int64_t n) {
  if (u < 0) u = -u;
  else if (u > n - 1) u = 2 * (n - 1) - u;
  return (u >= 0 && u < n) ? u : -1;
}

// The thread map of a written panel (fir_thread), the window over the 2 h + 1 taps of wsym: load(u) = d(t0 - h + u), so that
// output a sees d(t0 + a + k) with weight w[|k|].  trend [2 x p] (a then b) or NULL.
__global__ __launch_bounds__(256) void lowpass_fir_kernel(const float* __restrict__ S, int64_t n, int p, int64_t ld,
                                                           const double* __restrict__ wsym, int h,
                                                           const double* __restrict__ trend, double* __restrict__ Y) {
  const FirThread th = fir_thread(p);
  if (th.t0 >= n) return;
  const double ta = trend ? trend[th.j] : 0.0, tb = trend ? trend[p + th.j] : 0.0;
  double acc[FIR_WIN];
  fir16(
      [&](int u) {
        const int64_t r = lowpass_refl(th.t0 - h + u, n);
        if (r < 0) return 0.0;
        const double s = (double)S[r * ld + th.j];
        return trend ? s - fma(tb, (double)r, ta) : s;
      },
      wsym, 2 * h + 1, acc);
  fir_store(Y, n, p, th, [&](int a, int64_t t) { return trend ? acc[a] + fma(tb, (double)t, ta) : acc[a]; });
}

// grid (G, nb (nb + 1) / 2), nb = ceil(p / 64), block 256, dynamic LDS LOWPASS_LDS_Y.  blockIdx.y counts the pairs (bi, bj),
// bi <= bj, row by row.  Y [n x p], tight.  part [G x p x p]: partial b = the row tiles b, b + G, ... in ascending order,
// both images of every value.
__global__ __launch_bounds__(256, 2) void lowpass_gram_kernel(const double* __restrict__ Y, int64_t n, int p,
                                                               double* __restrict__ part) {
  extern __shared__ double lowpass_lds[];
  double* Ya = lowpass_lds;                                                     // [64][MFMA64_TILE_LD]
  double* Yb = lowpass_lds + FIR_R * MFMA64_TILE_LD;                           // [64][MFMA64_TILE_LD]
  const int nb = (p + 63) / 64;
  int bi = 0, bj = blockIdx.y;
  while (bj >= nb - bi) {
    bj -= nb - bi;
    ++bi;
  }
  bj += bi;
  const bool diag = bi == bj;
  const int wave = threadIdx.x >> 6;
  const Mfma64Lane ln = mfma64_lane();
  const int lc = ln.c, lk = ln.k;
  const bool active = 64 * bi + 16 * wave < p;                                  // (wave-uniform)
  const auto keep = [&](int y) { return 64 * bj + 16 * y < p && !(diag && y < wave); };
  const int64_t ntiles = (n + FIR_R - 1) / FIR_R;
  f64x4 acc[4];
  mfma64_zero(acc);
  const double* B = diag ? Ya : Yb;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * FIR_R;
    fir_stage_tile(Y, n, p, bi, r0, Ya);
    if (!diag) fir_stage_tile(Y, n, p, bj, r0, Yb);
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int s = 0; s < FIR_R / 4; ++s) {
        const double a = Ya[(4 * s + lk) * MFMA64_TILE_LD + 16 * wave + lc];
#pragma unroll
        for (int y = 0; y < 4; ++y)
          if (keep(y)) mfma64_step(acc[y], a, B[(4 * s + lk) * MFMA64_TILE_LD + 16 * y + lc]);
      }
    }
    __syncthreads();      // the next tile overwrites the LDS
  }
  if (!active) return;
  double* G = part + (int64_t)blockIdx.x * p * p;
#pragma unroll
  for (int y = 0; y < 4; ++y)
    if (keep(y))
      mfma64_each(acc[y], [&](int r, int c, double v) {
        const int gi = 64 * bi + 16 * wave + r, gj = 64 * bj + 16 * y + c;
        if (gi < p && gj < p && gi <= gj) {
          G[(int64_t)gi * p + gj] = v;
          if (gi != gj) G[(int64_t)gj * p + gi] = v;
        }
      });
}

}  // namespace eofx
