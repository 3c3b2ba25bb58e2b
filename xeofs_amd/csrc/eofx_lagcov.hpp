// eofx_lagcov.hpp -- the lag-summed covariance of optimal persistence analysis (xeofs/single/opa.py:104-171):
//
//     M[i, j] = sum_{tau < ntau} w[tau] sum_{t < n - tau} S[t, i] S[t + tau, j]          (S [n x p] float32, w, M float64)
//
// The reference forms one n x p x p product per lag.  Exchanging the sums gives ONE finite impulse response filter along
// the samples and ONE cross-product:
//
//     Y[t, j] = sum_{tau < ntau} w[tau] S[t + tau, j]      (rows t + tau >= n count as zero),          M = S^T Y,
//
// O(n p (ntau + p)) instead of O(n p^2 ntau).
//   lagcov_fir_kernel     Y [n x p] float64 written once (the route of ntau > LAGCOV_FUSE_NTAU);
//   lagcov_cross_kernel   per row tile of 64 samples and column block of 64: the tile of Y in LDS -- filtered there from the
//                         staged rows of S plus their ntau - 1 halo rows (FUSED: Y never reaches HBM) or read from the
//                         written Y --, then S^T Y on the fp64 matrix cores (eofx_mfma64.hpp; a blocked 4 x 4 block
//                         of accumulators), wave w owning the 64 x 64 output block of column block 4 g + w of S.  A workgroup walks its row tiles in ascending
//                         order and writes one partial; f64_reduce_kernel (eofx_kernels.hpp) sums the partials in a fixed order.
// Both filters slide a window of 16 outputs per thread along the samples: one read of S feeds 16 fused multiply-adds, and
// every Y[t, j] is summed over tau ascending.  The weights are read from a copy padded with 15 zeros on either side
// (wpad[15 + tau] = w[tau]), so the window needs no bounds test; the products with the padding are exact zeros.
// Float64 throughout, no atomics, the grid a function of the shape alone: two runs are equal bit for bit.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"

namespace eofx {

constexpr int LAGCOV_SROWS = LAGCOV_R + LAGCOV_FUSE_NTAU - 1;      // 128 staged rows of 64 float32
constexpr int LAGCOV_YLD = 80;           // row stride of the Y tile in doubles: rows 4 s + lk, lk = 0, 1 on disjoint banks
constexpr size_t LAGCOV_LDS_Y = (size_t)LAGCOV_R * LAGCOV_YLD * sizeof(double);
constexpr size_t LAGCOV_LDS_S = (size_t)LAGCOV_SROWS * 64 * sizeof(float);

// acc[a] = sum_tau w[tau] s(a + tau) for the 16 outputs a of a window, load(u) = s(u), u < ntau + 15.
// Output a sees s(u) with weight wpad[15 + u - a]: w[u - a] inside 0 <= u - a < ntau, an exact zero outside.
template <class Load>
__device__ __forceinline__ void lagcov_fir16(Load load, const double* __restrict__ wpad, int ntau, double (&acc)[LAGCOV_WIN]) {
#pragma unroll
  for (int a = 0; a < LAGCOV_WIN; ++a) acc[a] = 0.0;
#pragma unroll 4
  for (int u = 0; u < ntau + LAGCOV_PADW; ++u) {
    const double s = load(u);
    const double* wu = wpad + LAGCOV_PADW + u;          // (wave-uniform: scalar loads)
#pragma unroll
    for (int a = 0; a < LAGCOV_WIN; ++a) acc[a] = fma(wu[-a], s, acc[a]);
  }
}

// grid ceil(ceil(n / 16) p / 256), block 256: thread (window g, column j) writes Y[16 g .. 16 g + 15][j] (Y [n x p], tight)
__global__ __launch_bounds__(256) void lagcov_fir_kernel(const float* __restrict__ S, int64_t n, int p, int64_t ld,
                                                          const double* __restrict__ wpad, int ntau, double* __restrict__ Y) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t g = id / p;
  const int j = (int)(id - g * p);
  const int64_t t0 = g * LAGCOV_WIN;
  if (t0 >= n) return;
  double acc[LAGCOV_WIN];
  lagcov_fir16([&](int u) { const int64_t t = t0 + u; return t < n ? (double)S[t * ld + j] : 0.0; }, wpad, ntau, acc);
#pragma unroll
  for (int a = 0; a < LAGCOV_WIN; ++a)
    if (t0 + a < n) Y[(t0 + a) * p + j] = acc[a];
}

// grid (G, nb * ceil(nb / 4)), nb = ceil(p / 64), block 256, dynamic LDS LAGCOV_LDS_Y (+ LAGCOV_LDS_S when FUSED).
// blockIdx.y = bj + nb * g: column block bj of Y against column blocks 4 g .. 4 g + 3 of S (one per wave).
// part [G x p x p]: partial b = the row tiles b, b + G, ... in ascending order.
template <bool FUSED>
__global__ __launch_bounds__(256, 2) void lagcov_cross_kernel(const float* __restrict__ S, int64_t n, int p, int64_t ld,
                                                              const double* __restrict__ wpad, int ntau,
                                                              const double* __restrict__ Y, double* __restrict__ part) {
  extern __shared__ double lagcov_lds[];
  double* Ys = lagcov_lds;                                                    // [64][LAGCOV_YLD]
  float* Sh = reinterpret_cast<float*>(lagcov_lds + LAGCOV_R * LAGCOV_YLD);   // [LAGCOV_SROWS][64] (FUSED)
  const int nb = (p + 63) / 64;
  const int bj = blockIdx.y % nb, bi = 4 * (blockIdx.y / nb) + (threadIdx.x >> 6);
  const Mfma64Lane ln = mfma64_lane();
  const int lc = ln.c, lk = ln.k;
  const int64_t ntiles = (n + LAGCOV_R - 1) / LAGCOV_R;
  f64x4 acc[4][4];
  mfma64_zero(acc);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * LAGCOV_R;
    // this wave's rows of S, eight k-steps at a time: the first half is in flight while the tile of Y is made, the second
    // while the products of the first issue (all sixteen at once spill next to the accumulators)
    constexpr int H = LAGCOV_R / 8;
    float av[2][H][4];
    auto fetch = [&](int h) {
#pragma unroll
      for (int s = 0; s < H; ++s)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int64_t t = r0 + 4 * (H * h + s) + lk;
          const int gi = 64 * bi + 16 * x + lc;
          av[h][s][x] = (t < n && gi < p) ? S[t * ld + gi] : 0.f;
        }
    };
    fetch(0);
    if constexpr (FUSED) {
      const int srows = LAGCOV_R + ntau - 1;       // the tile and its halo (<= LAGCOV_SROWS): all the windows read; past n: zeros
      for (int e = threadIdx.x; e < srows * 64; e += 256) {
        const int64_t t = r0 + (e >> 6);
        const int gj = 64 * bj + (e & 63);
        Sh[e] = (t < n && gj < p) ? S[t * ld + gj] : 0.f;
      }
      __syncthreads();
      const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
      double y[LAGCOV_WIN];
      lagcov_fir16([&](int u) { return (double)Sh[(LAGCOV_WIN * g + u) * 64 + j]; }, wpad, ntau, y);
#pragma unroll
      for (int a = 0; a < LAGCOV_WIN; ++a) Ys[(LAGCOV_WIN * g + a) * LAGCOV_YLD + j] = y[a];
    } else {
      for (int e = threadIdx.x; e < LAGCOV_R * 64; e += 256) {
        const int64_t t = r0 + (e >> 6);
        const int gj = 64 * bj + (e & 63);
        Ys[(e >> 6) * LAGCOV_YLD + (e & 63)] = (t < n && gj < p) ? Y[t * p + gj] : 0.0;
      }
    }
    __syncthreads();
    if (bi < nb) {
      fetch(1);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < H; ++s) {
          double a[4], b[4];
#pragma unroll
          for (int x = 0; x < 4; ++x) a[x] = (double)av[h][s][x];
#pragma unroll
          for (int y = 0; y < 4; ++y) b[y] = Ys[(4 * (H * h + s) + lk) * LAGCOV_YLD + 16 * y + lc];
          mfma64_step(acc, a, b, Mfma64All{});
        }
    }
    __syncthreads();      // the next tile overwrites the LDS
  }
  if (bi >= nb) return;
  double* G = part + (int64_t)blockIdx.x * p * p;
  mfma64_each_blocked(acc, Mfma64All{}, [&](int, int, int i, int j, double v) {
    const int gi = 64 * bi + i, gj = 64 * bj + j;
    if (gi < p && gj < p) G[(int64_t)gi * p + gj] = v;
  });
}

}  // namespace eofx
