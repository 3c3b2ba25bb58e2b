// eofx_viewcov.hpp -- the block cross-covariance of multi-view canonical correlation analysis (xeofs/multi/cca.py:480-494):
//
//     C[i, j] = 1 / (n - 1) sum_t (Z[t, i] - mean[i]) (Z[t, j] - mean[j])      for i, j in different views,
//     C[i, j] = +0.0 inside a view (or the same sum with keep_diag)           (Z [n x p] float32, mean, C float64)
//
// with Z = [S_1 | ... | S_m] the views side by side and view[i] the view of column i.  The reference forms the whole
// covariance and subtracts its diagonal blocks; here those blocks and the lower triangle are never computed.
//   viewcov_zero_kernel     C = +0.0 over its p x p window (row stride ldc).
//   viewcov_kernel          one workgroup of four waves per LISTED tile of 128 x 128 outputs, wave (wi, wj) owning the 64 x 64
//                           block (a blocked 4 x 4 block of accumulators on the fp64 matrix cores, eofx_mfma64.hpp).
//                           The host lists the tiles (bi, bj), bj >= bi, that hold a wanted output: on or above the diagonal
//                           and, without keep_diag, not wholly inside one view.  The samples are walked in slabs of 16: the
//                           two slabs of Z (16 x 128 columns of the rows and of the columns of the tile) are fetched as
//                           float32 into registers while the products of the previous slab issue, then converted, centred
//                           in float64 and stored to LDS [k][column], row stride 144 doubles (rows k and k + 1 on disjoint
//                           halves of the banks, as MFMA64_TILE_LD).  Inside a tile a wave is idle (wave-uniform) when its block
//                           lies below the diagonal, outside C, or -- without keep_diag -- inside one view; blocks of 16 rows
//                           or columns outside C, and the 16 x 16 blocks below the diagonal of a wave on the diagonal, are
//                           skipped.  Every wanted C[i, j], i <= j, is written together with its mirror image C[j, i] from
//                           the same register: C == C^T bit for bit; a tile that straddles a view boundary masks per
//                           element (the zeros are those of viewcov_zero_kernel).
//   SPLIT                   when the listed tiles are too few to fill the machine, the slabs are split over G workgroups per
//                           tile, each a contiguous run of slabs in ascending order; partial (tile, g) is a 128 x 128 block,
//                           and viewcov_finish_kernel sums g ascending, scales, masks and writes both images.  G x tiles <=
//                           VIEWCOV_WGS, so the partials stay within VIEWCOV_WGS x 128 KiB = 64 MiB whatever n and p.
// Float64 throughout, no atomics; the tile list, G and the summation order are functions of (n, p, off, keep_diag) alone: two
// runs are equal bit for bit.  Rows and columns out of range are staged as zeros and never stored.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"

namespace eofx {

constexpr int VIEWCOV_PMAX = 4096;       // columns of Z
constexpr int VIEWCOV_MMAX = 64;         // views
constexpr int VIEWCOV_LD = VIEWCOV_T + 16;             // row stride of a slab in doubles
constexpr int VIEWCOV_E = VIEWCOV_K * VIEWCOV_T / 256; // elements of one slab per thread (8: one column, every other row)
constexpr int64_t VIEWCOV_TT = (int64_t)VIEWCOV_T * VIEWCOV_T;

// grid (ceil(p / 256), p), block 256: row blockIdx.y
__global__ __launch_bounds__(256) void viewcov_zero_kernel(double* __restrict__ C, int p, int64_t ldc) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < p) C[(int64_t)blockIdx.y * ldc + j] = 0.0;
}

// one wanted output and its mirror image
__device__ __forceinline__ void viewcov_store(double* __restrict__ C, int64_t ldc, int gi, int gj, double v) {
  C[(int64_t)gi * ldc + gj] = v;
  if (gi != gj) C[(int64_t)gj * ldc + gi] = v;
}

// grid (ntiles, G), block 256.  tiles [ntiles x 2] = (bi, bj); view [p]; chunk = slabs per split (all of them when !SPLIT).
// SPLIT: part [(tile G + g) x 128 x 128] raw sums; else C is written.
template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void viewcov_kernel(const float* __restrict__ Z, int64_t n, int p, int64_t ld,
                                                         const double* __restrict__ mean, const int* __restrict__ view,
                                                         const int* __restrict__ tiles, int keep_diag, int64_t chunk,
                                                         double* __restrict__ C, int64_t ldc, double* __restrict__ part) {
  __shared__ double As[VIEWCOV_K * VIEWCOV_LD];
  __shared__ double Bs[VIEWCOV_K * VIEWCOV_LD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const Mfma64Lane ln = mfma64_lane();
  const int lc = ln.c, lk = ln.k;
  const int wi = wave >> 1, wj = wave & 1;
  const int bi = tiles[2 * blockIdx.x], bj = tiles[2 * blockIdx.x + 1];
  const int i0 = bi * VIEWCOV_T, j0 = bj * VIEWCOV_T;       // first row and column of the tile
  const int ri = i0 + 64 * wi, cj = j0 + 64 * wj;           // ... and of this wave's block
  const int nxb = ri >= p ? 0 : ((p - ri < 64 ? p - ri : 64) + 15) / 16;       // 16-row blocks of this wave with a row of C
  const int nyb = cj >= p ? 0 : ((p - cj < 64 ? p - cj : 64) + 15) / 16;       // 16-column blocks
  bool active = nxb > 0 && nyb > 0 && !(bi == bj && wi > wj);
  const bool diag = bi == bj && wi == wj;                  // the block on the diagonal: its 16 x 16 blocks x > y lie below it
  if (active && !keep_diag) {
    const int il = ri + 63 < p ? ri + 63 : p - 1, jl = cj + 63 < p ? cj + 63 : p - 1;
    const int v = view[ri];                                 // (view is ascending: the block is inside one view when its corners are)
    active = !(view[il] == v && view[cj] == v && view[jl] == v);
  }
  // this thread's column of either slab and its mean
  const int col = tid & (VIEWCOV_T - 1), row0 = tid >> 7;   // rows row0, row0 + 2, ...
  const int ga = i0 + col, gb = j0 + col;
  const double ma = (mean && ga < p) ? mean[ga] : 0.0, mb = (mean && gb < p) ? mean[gb] : 0.0;
  const int64_t nslabs = (n + VIEWCOV_K - 1) / VIEWCOV_K;
  const int64_t s0 = (int64_t)blockIdx.y * chunk;
  const int64_t s1 = s0 + chunk < nslabs ? s0 + chunk : nslabs;
  f64x4 acc[4][4];
  mfma64_zero(acc);
  // the 16 x 16 blocks of this wave that are computed and written
  const auto keep = [&](int x, int y) { return x < nxb && y < nyb && !(diag && x > y); };
  float ar[VIEWCOV_E], br[VIEWCOV_E];
  auto fetch = [&](int64_t slab) {
#pragma unroll
    for (int e = 0; e < VIEWCOV_E; ++e) {
      const int64_t t = slab * VIEWCOV_K + row0 + 2 * e;
      ar[e] = (t < n && ga < p) ? Z[t * ld + ga] : 0.f;
      br[e] = (t < n && gb < p) ? Z[t * ld + gb] : 0.f;
    }
  };
  if (s0 < s1) fetch(s0);
  for (int64_t slab = s0; slab < s1; ++slab) {
    if (slab > s0) __syncthreads();                // the products of the previous slab have read the LDS
#pragma unroll
    for (int e = 0; e < VIEWCOV_E; ++e) {          // centred in float64; rows and columns out of range stay exact zeros
      const int64_t t = slab * VIEWCOV_K + row0 + 2 * e;
      const bool in = t < n;
      As[(row0 + 2 * e) * VIEWCOV_LD + col] = (in && ga < p) ? (double)ar[e] - ma : 0.0;
      Bs[(row0 + 2 * e) * VIEWCOV_LD + col] = (in && gb < p) ? (double)br[e] - mb : 0.0;
    }
    __syncthreads();
    if (slab + 1 < s1) fetch(slab + 1);            // in flight under the products
    if (!active) continue;                         // (wave-uniform; the barriers above are passed by every wave)
#pragma unroll
    for (int s = 0; s < VIEWCOV_K / 4; ++s) {
      double av[4], bv[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) av[x] = As[(4 * s + lk) * VIEWCOV_LD + 64 * wi + 16 * x + lc];
#pragma unroll
      for (int y = 0; y < 4; ++y) bv[y] = Bs[(4 * s + lk) * VIEWCOV_LD + 64 * wj + 16 * y + lc];
      mfma64_step(acc, av, bv, keep);
    }
  }
  if (!active) return;
  const double denom = (double)(n - 1);
  mfma64_each_blocked(acc, keep, [&](int, int, int i, int j, double v) {
    const int li = 64 * wi + i, lj = 64 * wj + j;
    if constexpr (SPLIT) {
      part[((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * VIEWCOV_TT + li * VIEWCOV_T + lj] = v;
    } else {
      const int gi = i0 + li, gj = j0 + lj;
      if (gi < p && gj < p && gi <= gj && (keep_diag || view[gi] != view[gj])) viewcov_store(C, ldc, gi, gj, v / denom);
    }
  });
}

// grid (128 * 128 / 256, ntiles), block 256: element e = 256 blockIdx.x + tid of tile blockIdx.y, summed over g ascending.
// Reads only what viewcov_kernel<true> wrote: a wanted output lies in an active wave's block.
__global__ __launch_bounds__(256) void viewcov_finish_kernel(const double* __restrict__ part, int G, int64_t n, int p,
                                                             const int* __restrict__ view, const int* __restrict__ tiles,
                                                             int keep_diag, double* __restrict__ C, int64_t ldc) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int gi = tiles[2 * blockIdx.y] * VIEWCOV_T + e / VIEWCOV_T, gj = tiles[2 * blockIdx.y + 1] * VIEWCOV_T + e % VIEWCOV_T;
  if (gi >= p || gj >= p || gi > gj || !(keep_diag || view[gi] != view[gj])) return;
  const double* src = part + (int64_t)blockIdx.y * G * VIEWCOV_TT + e;
  double sum = 0.0;
  for (int g = 0; g < G; ++g) sum += src[(int64_t)g * VIEWCOV_TT];
  viewcov_store(C, ldc, gi, gj, sum / (double)(n - 1));
}

}  // namespace eofx
