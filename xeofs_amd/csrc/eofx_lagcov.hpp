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
// The low-pass covariance (eofx_lowpass.hpp) is built from the same fir16, fir_thread, fir_store and fir_stage_tile.
// Float64 throughout, no atomics, the grid a function of the shape alone: two runs are equal bit for bit.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"

namespace eofx {

constexpr int LAGCOV_SROWS = FIR_R + LAGCOV_FUSE_NTAU - 1;         // 128 staged rows of 64 float32
constexpr size_t LAGCOV_LDS_Y = (size_t)FIR_R * MFMA64_TILE_LD * sizeof(double);
constexpr size_t LAGCOV_LDS_S = (size_t)LAGCOV_SROWS * 64 * sizeof(float);

// acc[a] = sum_{i < taps} wpad[15 + i] s(a + i) for the 16 outputs a of a window, load(u) = s(u), u < taps + 15, summed over
// u ascending.  Output a sees s(u) with weight wpad[15 + u - a]: a weight inside 0 <= u - a < taps, an exact zero outside.
template <class Load>
__device__ __forceinline__ void fir16(Load load, const double* __restrict__ wpad, int taps, double (&acc)[FIR_WIN]) {
#pragma unroll
  for (int a = 0; a < FIR_WIN; ++a) acc[a] = 0.0;
#pragma unroll 4
  for (int u = 0; u < taps + FIR_PADW; ++u) {
    const double s = load(u);
    const double* wu = wpad + FIR_PADW + u;             // (wave-uniform: scalar loads)
#pragma unroll
    for (int a = 0; a < FIR_WIN; ++a) acc[a] = fma(wu[-a], s, acc[a]);
  }
}

// A written-panel filter runs on a grid ceil(ceil(n / 16) p / 256), block 256: thread (window g, column j) owns the outputs
// Y[t0 .. t0 + 15][j], t0 = 16 g, of the tight panel Y [n x p] (none where t0 >= n) and stores Y[t0 + a][j] = value(a, t0 + a).
struct FirThread {
  int64_t t0;
  int j;
};
__device__ __forceinline__ FirThread fir_thread(int p) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t g = id / p;
  return {g * FIR_WIN, (int)(id - g * p)};
}
template <class Value>
__device__ __forceinline__ void fir_store(double* __restrict__ Y, int64_t n, int p, FirThread th, Value value) {
#pragma unroll
  for (int a = 0; a < FIR_WIN; ++a) {
    const int64_t t = th.t0 + a;
    if (t < n) Y[t * p + th.j] = value(a, t);
  }
}

// the 64 x 64 tile at rows r0 .. r0 + 63 of column block b of the tight panel Y [n x p] into dst [64][MFMA64_TILE_LD] (LDS),
// by the 256 threads of a workgroup; rows past n and columns past p are exact zeros
__device__ __forceinline__ void fir_stage_tile(const double* __restrict__ Y, int64_t n, int p, int b, int64_t r0, double* dst) {
  for (int e = threadIdx.x; e < FIR_R * 64; e += 256) {
    const int64_t t = r0 + (e >> 6);
    const int gj = 64 * b + (e & 63);
    dst[(e >> 6) * MFMA64_TILE_LD + (e & 63)] = (t < n && gj < p) ? Y[t * p + gj] : 0.0;
  }
}

__global__ __launch_bounds__(256) void lagcov_fir_kernel(const float* __restrict__ S, int64_t n, int p, int64_t ld,
                                                          const double* __restrict__ wpad, int ntau, double* __restrict__ Y) {
  const FirThread th = fir_thread(p);
  if (th.t0 >= n) return;
  double acc[FIR_WIN];
  fir16([&](int u) { const int64_t t = th.t0 + u; return t < n ? (double)S[t * ld + th.j] : 0.0; }, wpad, ntau, acc);
  fir_store(Y, n, p, th, [&](int a, int64_t) { return acc[a]; });
}

// grid (G, nb * ceil(nb / 4)), nb = ceil(p / 64), block 256, dynamic LDS LAGCOV_LDS_Y (+ LAGCOV_LDS_S when FUSED).
// blockIdx.y = bj + nb * g: column block bj of Y against column blocks 4 g .. 4 g + 3 of S (one per wave).
// part [G x p x p]: partial b = the row tiles b, b + G, ... in ascending order.
template <bool FUSED>
__global__ __launch_bounds__(256, 2) void lagcov_cross_kernel(const float* __restrict__ S, int64_t n, int p, int64_t ld,
                                                              const double* __restrict__ wpad, int ntau,
                                                              const double* __restrict__ Y, double* __restrict__ part) {
  extern __shared__ double lagcov_lds[];
  double* Ys = lagcov_lds;                                                    // [64][MFMA64_TILE_LD]
  float* Sh = reinterpret_cast<float*>(lagcov_lds + FIR_R * MFMA64_TILE_LD);   // [LAGCOV_SROWS][64] (FUSED)
  const int nb = (p + 63) / 64;
  const int bj = blockIdx.y % nb, bi = 4 * (blockIdx.y / nb) + (threadIdx.x >> 6);
  const Mfma64Lane ln = mfma64_lane();
  const int lc = ln.c, lk = ln.k;
  const int64_t ntiles = (n + FIR_R - 1) / FIR_R;
  f64x4 acc[4][4];
  mfma64_zero(acc);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * FIR_R;
    // this wave's rows of S, eight k-steps at a time: the first half is in flight while the tile of Y is made, the second
    // while the products of the first issue (all sixteen at once spill next to the accumulators)
    constexpr int H = FIR_R / 8;
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
      const int srows = FIR_R + ntau - 1;       // the tile and its halo (<= LAGCOV_SROWS): all the windows read; past n: zeros
      for (int e = threadIdx.x; e < srows * 64; e += 256) {
        const int64_t t = r0 + (e >> 6);
        const int gj = 64 * bj + (e & 63);
        Sh[e] = (t < n && gj < p) ? S[t * ld + gj] : 0.f;
      }
      __syncthreads();
      const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
      double y[FIR_WIN];
      fir16([&](int u) { return (double)Sh[(FIR_WIN * g + u) * 64 + j]; }, wpad, ntau, y);
#pragma unroll
      for (int a = 0; a < FIR_WIN; ++a) Ys[(FIR_WIN * g + a) * MFMA64_TILE_LD + j] = y[a];
    } else {
      fir_stage_tile(Y, n, p, bj, r0, Ys);
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
          for (int y = 0; y < 4; ++y) b[y] = Ys[(4 * (H * h + s) + lk) * MFMA64_TILE_LD + 16 * y + lc];
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
