// eofx_colquad.hpp -- the quadratic-form operator of empirical orthogonal teleconnections (van den Dool, Saha & Johansson
// 2000; single/eot.py): for every series (row) of a series-major float32 panel T [p x n] and ANY square float32 matrix
// A [n x n] (row-major, no symmetry assumed),
//
//     q[j] = sum_s sum_t T[j, s] A[s, t] T[j, t]                                  (float64)
//
// With A = Xc Xc^T deflated by the series found so far, q[j] is the variance of all grid points explained by grid point j
// times |x_j|^2: one mode of EOT is one call.  The p x n product Y = T A is never written.
//   colquad_kernel      workgroup (i, c) of (row_tiles, splits) owns the COLQUAD_TJ = 128 series j0 = 128 i .. and the column
//                       blocks [c cb / splits, (c + 1) cb / splits) of the cb = ceil(n / 128) blocks of COLQUAD_TS = 128
//                       columns of A.  Per column block s0: Y[j, s] = sum_t T[j, t] A[t, s] on the matrix cores, t walked in
//                       chunks of COLQUAD_KC = 32; wave (wi, wj) of four owns the 64 x 64 block of Y, a 2 x 2 block of 32 x 32
//                       accumulators of v_mfma_f32_32x32x2_f32 -- float32 operands and accumulators, bitwise an fmaf chain over
//                       t ascending.  (The product is taken as T . A and contracted with T[j, s] over the COLUMN index s of A:
//                       sum_s T[j, s] (sum_t T[j, t] A[t, s]) is the same double sum with the names of s and t exchanged.)
//     staging           thread (t = tid & 31, g = tid >> 5) loads sample t0 + t of the 16 series g + 8 e: a half-wave reads 128
//                       contiguous bytes of one series, so a load instruction touches two cache lines (a first form, 16
//                       consecutive t of one series per thread, touched 64 lines per instruction and ran at 0.64 of the rate);
//                       they are stored transposed, Ts[t][series].  The 32 x 128 chunk of A goes to Bs[t][column] as it lies,
//                       entry 256 e + tid by thread tid (a wave reads 256 contiguous bytes of a row of A).  The loads of chunk
//                       t0 + 32 are issued into registers before the products of chunk t0, so they are on their way while the
//                       matrix cores work (register prefetch; LDS is single-buffered, two barriers per chunk).  Indices out of
//                       range are clamped, so the 32 loads are unconditional and in flight together; what is out of range
//                       (series >= p, t >= n, column >= n) is stored as zero: fma(0, 0, c) == c.
//     LDS image         Ts [32][129] and Bs [32][128] floats, 16.1 + 16 KiB: two workgroups per CU.  The odd row length of Ts
//                       puts the 32 stores of a half-wave (32 t, one series: 129 dwords apart) on 32 different banks.  Operand
//                       read: lane l takes Ts[2 u + (l >> 5)][row0 + (l & 31)] -- a group of 32 lanes reads 32 consecutive
//                       dwords: conflict-free.
//     epilogue          accumulator register r of lane l is series (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its
//                       block: the lane reads T[j, s] of its column from global memory (128 B coalesced per series), and adds
//                       (double) Y[j, s] * (double) T[j, s] over its two columns -- selected, not multiplied, away where j >= p
//                       or s >= n; then the 32 lanes of a series in a fixed butterfly, and lane 0 of the half-wave adds the
//                       sum to red[wj][series] in LDS (2 KiB; only this wave touches its entries; keeping the 32 sums of a
//                       lane in registers over the column blocks spilled).  Column blocks ascending; at the end the two waves
//                       that share a series, wj ascending.
//   colquad_sum_kernel  splits > 1: q[j] = sum_c part[c][j], c ascending.  (splits == 1: the first kernel writes q itself.)
// Series j of the result is computed from series j of T and from A alone: every product of the matrix core, every lane sum and
// every partial stays inside one series, so a NaN or an infinity in one series reaches no other.  No atomics; the grid and the
// order of every sum are functions of (n, p) alone (colquad_plan): two runs are equal bit for bit.  Nothing but q[0 .. p) and
// the arena scratch of splits x p doubles is written.  Traffic and flops: DESIGN.md section 22.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eofx.h"

namespace eofx {

constexpr int COLQUAD_NMAX = 16384;      // samples: A is 1 GB there
constexpr int COLQUAD_TJ = 128;          // series per workgroup (64 per wave)
constexpr int COLQUAD_TS = 128;          // columns of A per block (64 per wave)
constexpr int COLQUAD_KC = 32;           // samples t per chunk
constexpr int COLQUAD_TLD = COLQUAD_TJ + 1;      // floats between two t of the LDS image of T (see "LDS image")
constexpr int COLQUAD_SMAX = 16;         // workgroups that share the columns of A for one series tile, at most
constexpr int COLQUAD_WGS = 512;         // workgroups the split aims at: two per CU

typedef float colquad_f32x16 __attribute__((ext_vector_type(16)));

// launch shape of colquad_kernel (a function of n and p alone; p >= 1, n >= 1): grid (row_tiles, splits), and split c takes the
// column blocks colquad_first_block(pl, c) .. colquad_first_block(pl, c + 1) - 1 -- at least one each
struct ColquadPlan {
  int64_t row_tiles;   // ceil(p / COLQUAD_TJ)
  int col_blocks;      // ceil(n / COLQUAD_TS)
  int splits;          // min(col_blocks, COLQUAD_SMAX, ceil(COLQUAD_WGS / row_tiles))
};
inline ColquadPlan colquad_plan(int64_t n, int64_t p) {
  ColquadPlan pl;
  pl.row_tiles = (p + COLQUAD_TJ - 1) / COLQUAD_TJ;
  pl.col_blocks = (int)((n + COLQUAD_TS - 1) / COLQUAD_TS);
  int64_t s = (COLQUAD_WGS + pl.row_tiles - 1) / pl.row_tiles;
  if (s > COLQUAD_SMAX) s = COLQUAD_SMAX;
  if (s > pl.col_blocks) s = pl.col_blocks;
  pl.splits = (int)s;
  return pl;
}
__host__ __device__ __forceinline__ int colquad_first_block(int col_blocks, int splits, int c) {
  return (int)((int64_t)c * col_blocks / splits);
}

// grid (row_tiles, splits), block 256.  out [splits x p]: out[c p + j] = the part of q[j] of the column blocks of split c.
__global__ __launch_bounds__(256, 2) void colquad_kernel(const float* __restrict__ T, int64_t p, int n, int64_t ld,
                                                         const float* __restrict__ A, int64_t lda, double* __restrict__ out,
                                                         int col_blocks) {
  __shared__ float Ts[COLQUAD_KC * COLQUAD_TLD];
  __shared__ float Bs[COLQUAD_KC * COLQUAD_TS];
  __shared__ double red[2][COLQUAD_TJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int64_t j0 = (int64_t)blockIdx.x * COLQUAD_TJ;
  const int b_lo = colquad_first_block(col_blocks, (int)gridDim.y, (int)blockIdx.y);
  const int b_hi = colquad_first_block(col_blocks, (int)gridDim.y, (int)blockIdx.y + 1);
  const int st = tid & 31, sg = tid >> 5;                               // staging of T: this thread's t of a chunk, its series sg + 8 e
  red[tid >> 7][tid & 127] = 0.0;                                      // (ordered against its first use by the barriers of a chunk)
  for (int cb = b_lo; cb < b_hi; ++cb) {
    const int s0 = cb * COLQUAD_TS;
    colquad_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // the chunk t0 from global memory into registers (clamped, not predicated: the 32 loads are in flight together)
    float tr[COLQUAD_KC / 2], ar[COLQUAD_KC / 2];
    const int ac = s0 + (tid & 127) < n ? s0 + (tid & 127) : n - 1;       // this thread's column of A, the same in every chunk
    const auto fetch = [&](int t0) {
      const int tc = t0 + st < n ? t0 + st : n - 1;
#pragma unroll
      for (int e = 0; e < COLQUAD_KC / 2; ++e) {
        const int64_t gj = j0 + sg + 8 * e;
        tr[e] = T[(gj < p ? gj : p - 1) * ld + tc];
        const int gt = t0 + 2 * e + (tid >> 7);
        ar[e] = A[(int64_t)(gt < n ? gt : n - 1) * lda + ac];
      }
    };
    fetch(0);
    for (int t0 = 0; t0 < n; t0 += COLQUAD_KC) {
      __syncthreads();                                                  // the products of the previous chunk have read the LDS
#pragma unroll
      for (int e = 0; e < COLQUAD_KC / 2; ++e) {
        Ts[st * COLQUAD_TLD + sg + 8 * e] = (t0 + st < n && j0 + sg + 8 * e < p) ? tr[e] : 0.f;
        const int x = 256 * e + tid;
        Bs[x] = (t0 + (x >> 7) < n && s0 + (x & 127) < n) ? ar[e] : 0.f;
      }
      if (t0 + COLQUAD_KC < n) fetch(t0 + COLQUAD_KC);                  // the next chunk is on its way during the products
      __syncthreads();
      const int steps = ((n - t0 < COLQUAD_KC ? n - t0 : COLQUAD_KC) + 1) / 2;
      for (int u = 0; u < steps; ++u) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = Ts[(2 * u + lh) * COLQUAD_TLD + 64 * wi + 32 * a + lr];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = Bs[(2 * u + lh) * COLQUAD_TS + 64 * wj + 32 * b + lr];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
    // red[wj][j] += sum_s (double) Y[j, s] (double) T[j, s] over the 64 columns of this wave: b ascending per lane, then the 32
    // lanes of a series in a fixed butterfly (a half-wave holds one series per register).  Only this wave touches its entries.
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      double v[16];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int s = s0 + 64 * wj + 32 * b + lr;
        float tv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t j = j0 + 64 * wi + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lh;
          tv[r] = T[(j < p ? j : p - 1) * ld + (s < n ? s : n - 1)];    // (clamped: the 16 loads are in flight together)
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t j = j0 + 64 * wi + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const double x = (j < p && s < n) ? (double)acc[a][b][r] * (double)tv[r] : 0.0;      // selected, not multiplied, away
          v[r] = b ? v[r] + x : x;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v[r] += __shfl_xor(v[r], o);
        if (lr == 0) red[wj][64 * wi + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lh] += v[r];
      }
    }
  }
  __syncthreads();
  if (tid < COLQUAD_TJ && j0 + tid < p) out[(int64_t)blockIdx.y * p + j0 + tid] = red[0][tid] + red[1][tid];
}

// grid ceil(p / 256), block 256: q[j] = sum_c part[c p + j], c ascending
__global__ __launch_bounds__(256) void colquad_sum_kernel(const double* __restrict__ part, int splits, int64_t p,
                                                          double* __restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p) return;
  double s = part[j];
  for (int c = 1; c < splits; ++c) s += part[(int64_t)c * p + j];
  q[j] = s;
}

}  // namespace eofx
