// eofx_pcmul.hpp -- the PC-space product of principal oscillation pattern analysis (xeofs/single/pop.py:185-198, 239):
//
//     Y [rows x b] = X [rows x a] M [a x b]        (X float32 | float64, M float64, Y float64 | float32; a <= 1024, b <= 2048)
//
// a tall panel -- the n samples' PCA scores or the P features' PCA patterns -- times a small dense matrix whose inner length
// is the number of PCA modes.  Accumulated in float64 on the fp64 matrix cores (eofx_mfma64.hpp) and rounded once.
//   pcmul_kernel   a workgroup of four waves owns a tile of 64 rows and 256 columns of Y, wave w the 64 x 64 block of columns
//                  64 w .. 64 w + 63 (a blocked 4 x 4 block of accumulators).  The inner
//                  length is walked in slabs of 16: the slab of X (64 x 16, converted to float64 in registers) and of M
//                  (16 x 256) are fetched into registers while the products of the previous slab issue, then stored to LDS.
//                  Row strides: 18 doubles for X (lanes (i, k) and (i, k + 1), i < 16, on 32 distinct bank pairs: 36 i mod 64
//                  runs over the multiples of 4) and 272 for M (rows k and k + 1 on disjoint halves of the banks, as
//                  MFMA64_TILE_LD).  Blocks of 16 rows or 16 columns that lie wholly outside Y are skipped (wave-uniform).
// Every output is summed over k ascending by one lane chain, no atomics, the grid a function of the shape alone: two runs
// are equal bit for bit.  Rows, columns and k out of range are staged as zeros and never stored.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"

namespace eofx {

constexpr int PCMUL_AMAX = 1024;         // inner length (the PCA modes)
constexpr int PCMUL_BMAX = 2048;         // columns of M
constexpr int PCMUL_R = 64;              // rows per tile
constexpr int PCMUL_C = 256;             // columns per workgroup (64 per wave)
constexpr int PCMUL_K = 16;              // inner length per slab
constexpr int PCMUL_XLD = PCMUL_K + 2;   // row stride of the X slab in doubles
constexpr int PCMUL_MLD = PCMUL_C + 16;  // row stride of the M slab in doubles
constexpr int PCMUL_XE = PCMUL_R * PCMUL_K / 256;      // elements of the X slab per thread (4)
constexpr int PCMUL_ME = PCMUL_K;                      // elements of the M slab per thread (one column, 16 rows)

// grid (ceil(rows / 64), ceil(b / 256)), block 256
template <class TX, class TY>
__global__ __launch_bounds__(256, 2) void pcmul_kernel(const TX* __restrict__ X, int64_t rows, int a, int64_t ldx,
                                                       const double* __restrict__ M, int b, TY* __restrict__ Y, int64_t ldy) {
  __shared__ double Xs[PCMUL_R * PCMUL_XLD];
  __shared__ double Ms[PCMUL_K * PCMUL_MLD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const Mfma64Lane ln = mfma64_lane();
  const int lc = ln.c, lk = ln.k;
  const int64_t r0 = (int64_t)blockIdx.x * PCMUL_R;
  const int cg = blockIdx.y * PCMUL_C;             // first column of the workgroup
  const int c0 = cg + 64 * wave;                   // first column of the wave
  const int nxb = (int)((rows - r0 < PCMUL_R ? rows - r0 : (int64_t)PCMUL_R) + 15) / 16;       // 16-row blocks with a row of Y
  const int nyb = c0 >= b ? 0 : ((b - c0 < 64 ? b - c0 : 64) + 15) / 16;                       // 16-column blocks of this wave
  f64x4 acc[4][4];
  mfma64_zero(acc);
  double xr[PCMUL_XE], mr[PCMUL_ME];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < PCMUL_XE; ++i) {           // element e = tid + 256 i of the slab: row e / 16, k e % 16
      const int e = tid + 256 * i;
      const int64_t r = r0 + (e >> 4);
      const int k = k0 + (e & 15);
      xr[i] = (r < rows && k < a) ? (double)X[r * ldx + k] : 0.0;
    }
    const int c = cg + tid;
#pragma unroll
    for (int i = 0; i < PCMUL_ME; ++i) mr[i] = (k0 + i < a && c < b) ? M[(int64_t)(k0 + i) * b + c] : 0.0;
  };
  fetch(0);
  for (int k0 = 0; k0 < a; k0 += PCMUL_K) {
    if (k0) __syncthreads();                       // the products of the previous slab have read the LDS
#pragma unroll
    for (int i = 0; i < PCMUL_XE; ++i) {
      const int e = tid + 256 * i;
      Xs[(e >> 4) * PCMUL_XLD + (e & 15)] = xr[i];
    }
#pragma unroll
    for (int i = 0; i < PCMUL_ME; ++i) Ms[i * PCMUL_MLD + tid] = mr[i];
    __syncthreads();
    if (k0 + PCMUL_K < a) fetch(k0 + PCMUL_K);     // in flight under the products
    if (nyb == 0) continue;                        // (wave-uniform; the barriers above are passed by every wave)
#pragma unroll
    for (int s = 0; s < PCMUL_K / 4; ++s) {
      double av[4], bv[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) av[x] = Xs[(16 * x + lc) * PCMUL_XLD + 4 * s + lk];
#pragma unroll
      for (int y = 0; y < 4; ++y) bv[y] = Ms[(4 * s + lk) * PCMUL_MLD + 64 * wave + 16 * y + lc];
      mfma64_step(acc, av, bv, [&](int x, int y) { return x < nxb && y < nyb; });
    }
  }
  mfma64_each_blocked(acc, Mfma64All{}, [&](int, int, int i, int j, double v) {
    const int64_t r = r0 + i;
    const int c = c0 + j;
    if (r < rows && c < b) Y[r * ldy + c] = (TY)v;
  });
}

}  // namespace eofx
