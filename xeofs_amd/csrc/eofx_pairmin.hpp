// eofx_pairmin.hpp -- the pairwise-minimum operator of the teleconnectivity map (Wallace & Gutzler 1981;
// single/teleconnectivity.py): for a series-major float32 panel T [p x n] and a float32 scale vector w [p],
//
//     d[j, i]    = sum_t T[j, t] T[i, t]        (float32 operands and accumulators, t ascending)
//     r[j, i]    = (d[j, i] * w[j]) * w[i]      (float32, this order)
//     rmin[j]    = min r[j, i] over i != j with w[i] > 0 and r[j, i] not NaN
//     partner[j] = the LOWEST i that attains it (int32)
//
// and rmin[j] = NaN, partner[j] = -1 where w[j] <= 0, w[j] is NaN or no admissible i exists.  With T centred and
// w[j] = 1 / |T_j|, r is the correlation matrix of the series and -rmin the teleconnectivity; the kernel assumes neither.
// The p x p matrix r never exists: 2 n p^2 flops on the matrix cores with the reduction in the epilogue.
//   pairmin_kernel      workgroup (a, c) of (tiles, splits) owns the PAIRMIN_TJ = 128 series j0 = 128 a .. and the tiles
//                       [c tiles / splits, (c + 1) tiles / splits) of the tiles = ceil(p / 128) tiles of PAIRMIN_TI = 128
//                       series i, walked in ASCENDING order.  Per tile i0: d[j, i] on the matrix cores, t walked in chunks of
//                       PAIRMIN_KC = 32; wave (wi, wj) of four owns the 64 x 64 block of d, a 2 x 2 block of 32 x 32
//                       accumulators of v_mfma_f32_32x32x2_f32 -- bitwise an fmaf chain over t ascending (the tile map, the
//                       staging and the chunk loop are those of eofx_colquad.hpp; the second operand is the panel itself).
//     staging           thread (t = tid & 31, g = tid >> 5) loads sample t0 + t of the 16 series g + 8 e of BOTH tiles: a
//                       half-wave reads 128 contiguous bytes of one series; they are stored transposed, Js[t][series j] and
//                       Is[t][series i].  The loads of chunk t0 + 32 are issued into registers before the products of chunk
//                       t0 (register prefetch; LDS is single-buffered, two barriers per chunk).  Indices out of range are
//                       clamped, so the 32 loads are unconditional and in flight together; what is out of range (series >= p,
//                       t >= n) is stored as zero: fma(0, 0, c) == c.
//     LDS image         Js [32][129] and Is [32][129] floats, 2 x 16.1 KiB, and 2.5 KiB for the minima and w[j]: two workgroups
//                       per CU.  The odd row length puts the 32 stores of a half-wave (32 t, one series: 129 dwords apart) on
//                       32 different banks.  Operand read: lane l takes Js[2 u + (l >> 5)][row0 + (l & 31)] -- a group of 32
//                       lanes reads 32 consecutive dwords: conflict-free.
//     epilogue          accumulator register r of lane l is series j = (r & 3) + 8 (r >> 2) + 4 (l >> 5), series i = l & 31
//                       of its block.  Per tile the lane forms x = (d w[j]) w[i] (w[j] from LDS, w[i] from global memory,
//                       clamped) for its two columns, b ascending, and keeps the smaller on strict <; a pair is SELECTED
//                       away -- not scaled away -- where i >= p (a padding series never becomes a partner, whatever w
//                       holds), i == j, w[i] > 0 fails, or x is NaN.  Then the 32 lanes of a series in a butterfly, and lane
//                       0 of the half-wave holds the result against red[wj][series] in LDS, the minimum of the tiles before
//                       (only this wave touches its entries; keeping the 32 (value, index) pairs of a lane in registers
//                       over the tiles spilled 126 VGPRs).  After the last tile the two waves wj that share a series,
//                       wj ascending.  Every combination is by the one rule
//                           b replaces a  <=>  b has a partner and (a has none, or b.value < a.value,
//                                                                   or b.value == a.value and b.index < a.index),
//                       a total order on (value, index), so the lowest index wins every tie in any order of combination
//                       (-0.0 == +0.0: the value of the lower index is kept).  Then the rule on w[j]; a series without a
//                       partner is written as (NaN, -1).
//   pairmin_combine_kernel  splits > 1: (rmin, partner)[j] = the partials of split c = 0, 1, ... combined in ascending order
//                       by the same rule.  (splits == 1: the first kernel writes rmin and partner itself.)
// A NaN or an infinity in series i reaches r[j, i] of every j, and nothing else: a NaN pair is not admissible, an infinite
// one takes part in the comparisons of row j as the value it is.  The accumulators of a pair (j, i) are computed from the two
// series alone (zero padding meets only padding or t >= n, where BOTH operands are zero), so a bad series changes neither
// rmin nor partner of a series whose admissible minimum lies elsewhere.  No atomics; the grid and the order of every
// comparison are functions of (n, p) alone (pairmin_plan): two runs are equal bit for bit.  Nothing but rmin[0 .. p),
// partner[0 .. p) and the arena scratch of splits x p partials is written.  r[j, i] = r[i, j] is NOT used: every tile pair
// is visited (the open step, DESIGN.md section 23, with the traffic and flops).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eofx.h"

namespace eofx {

constexpr int64_t PAIRMIN_NMAX = (int64_t)1 << 30;      // samples: t and t0 + 32 stay inside an int
constexpr int PAIRMIN_TJ = 128;          // series j per workgroup (64 per wave)
constexpr int PAIRMIN_TI = 128;          // series i per tile (64 per wave)
constexpr int PAIRMIN_KC = 32;           // samples t per chunk
constexpr int PAIRMIN_LD = PAIRMIN_TJ + 1;       // floats between two t of the LDS images (see "LDS image")
constexpr int PAIRMIN_SMAX = 16;         // workgroups that share the tiles of i for one tile of j, at most
constexpr int PAIRMIN_WGS = 512;         // workgroups the split aims at: two per CU

typedef float pairmin_f32x16 __attribute__((ext_vector_type(16)));

// launch shape of pairmin_kernel (a function of p alone; p >= 1): grid (tiles, splits), and split c takes the tiles of i
// pairmin_first_tile(tiles, splits, c) .. pairmin_first_tile(tiles, splits, c + 1) - 1 -- at least one each
struct PairminPlan {
  int64_t tiles;       // ceil(p / PAIRMIN_TJ): the tiles of j and of i
  int splits;          // min(tiles, PAIRMIN_SMAX, ceil(PAIRMIN_WGS / tiles))
};
inline PairminPlan pairmin_plan(int64_t n, int64_t p) {
  (void)n;
  PairminPlan pl;
  pl.tiles = (p + PAIRMIN_TJ - 1) / PAIRMIN_TJ;
  int64_t s = (PAIRMIN_WGS + pl.tiles - 1) / pl.tiles;
  if (s > PAIRMIN_SMAX) s = PAIRMIN_SMAX;
  if (s > pl.tiles) s = pl.tiles;
  pl.splits = (int)s;
  return pl;
}
__host__ __device__ __forceinline__ int64_t pairmin_first_tile(int64_t tiles, int splits, int c) { return (int64_t)c * tiles / splits; }

// b replaces a: the one rule of every combination (index < 0: no partner)
__host__ __device__ __forceinline__ bool pairmin_better(float bv, int bi, float av, int ai) {
  return bi >= 0 && (ai < 0 || bv < av || (bv == av && bi < ai));
}

// grid (tiles, splits), block 256.  out_v, out_i [splits x p]: the minimum of series j over the tiles of split c.
__global__ __launch_bounds__(256, 2) void pairmin_kernel(const float* __restrict__ T, int64_t p, int n, int64_t ld,
                                                         const float* __restrict__ w, float* __restrict__ out_v,
                                                         int32_t* __restrict__ out_i, int64_t tiles) {
  __shared__ float Js[PAIRMIN_KC * PAIRMIN_LD];
  __shared__ float Is[PAIRMIN_KC * PAIRMIN_LD];
  __shared__ float red_v[2][PAIRMIN_TJ];
  __shared__ int red_i[2][PAIRMIN_TJ];
  __shared__ float wjs[PAIRMIN_TJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int64_t j0 = (int64_t)blockIdx.x * PAIRMIN_TJ;
  const int64_t b_lo = pairmin_first_tile(tiles, (int)gridDim.y, (int)blockIdx.y);
  const int64_t b_hi = pairmin_first_tile(tiles, (int)gridDim.y, (int)blockIdx.y + 1);
  const int st = tid & 31, sg = tid >> 5;                               // staging: this thread's t of a chunk, its series sg + 8 e
  if (tid < PAIRMIN_TJ) wjs[tid] = w[j0 + tid < p ? j0 + tid : p - 1];    // (clamped; ordered against their first use by the
  red_i[tid >> 7][tid & 127] = -1;                                      //  barriers of a chunk: n >= 1)
  red_v[tid >> 7][tid & 127] = 0.f;
  for (int64_t ib = b_lo; ib < b_hi; ++ib) {
    const int64_t i0 = ib * PAIRMIN_TI;
    pairmin_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // the chunk t0 from global memory into registers (clamped, not predicated: the 32 loads are in flight together)
    float jr[PAIRMIN_KC / 2], ir[PAIRMIN_KC / 2];
    const auto fetch = [&](int t0) {
      const int tc = t0 + st < n ? t0 + st : n - 1;
#pragma unroll
      for (int e = 0; e < PAIRMIN_KC / 2; ++e) {
        const int64_t gj = j0 + sg + 8 * e, gi = i0 + sg + 8 * e;
        jr[e] = T[(gj < p ? gj : p - 1) * ld + tc];
        ir[e] = T[(gi < p ? gi : p - 1) * ld + tc];
      }
    };
    fetch(0);
    for (int t0 = 0; t0 < n; t0 += PAIRMIN_KC) {
      __syncthreads();                                                  // the products of the previous chunk have read the LDS
#pragma unroll
      for (int e = 0; e < PAIRMIN_KC / 2; ++e) {
        Js[st * PAIRMIN_LD + sg + 8 * e] = (t0 + st < n && j0 + sg + 8 * e < p) ? jr[e] : 0.f;
        Is[st * PAIRMIN_LD + sg + 8 * e] = (t0 + st < n && i0 + sg + 8 * e < p) ? ir[e] : 0.f;
      }
      if (t0 + PAIRMIN_KC < n) fetch(t0 + PAIRMIN_KC);                  // the next chunk is on its way during the products
      __syncthreads();
      const int steps = ((n - t0 < PAIRMIN_KC ? n - t0 : PAIRMIN_KC) + 1) / 2;
      for (int u = 0; u < steps; ++u) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = Js[(2 * u + lh) * PAIRMIN_LD + 64 * wi + 32 * a + lr];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = Is[(2 * u + lh) * PAIRMIN_LD + 64 * wj + 32 * b + lr];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
    // x = (d w[j]) w[i]: the minimum of series j over the 64 columns of this wave -- b ascending per lane, then the 32 lanes of
    // a series in a butterfly (a half-wave holds one series per register) -- against red[wj][series], the minimum of the tiles
    // before.  Only this wave touches its entries.
    float wiv[2];
    bool col_ok[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t i = i0 + 64 * wj + 32 * b + lr;
      wiv[b] = w[i < p ? i : p - 1];
      col_ok[b] = i < p && wiv[b] > 0.f;                                // selected, not scaled, away
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int s = 64 * wi + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float wjv = wjs[s];
        float v = 0.f;
        int x = -1;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int64_t i = i0 + 64 * wj + 32 * b + lr;
          const float y = (acc[a][b][r] * wjv) * wiv[b];
          if (col_ok[b] && i != j0 + s && y == y && (x < 0 || y < v)) {
            v = y;
            x = (int)i;
          }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
          const float ov = __shfl_xor(v, o);
          const int ox = __shfl_xor(x, o);
          if (pairmin_better(ov, ox, v, x)) {
            v = ov;
            x = ox;
          }
        }
        if (lr == 0 && pairmin_better(v, x, red_v[wj][s], red_i[wj][s])) {
          red_v[wj][s] = v;
          red_i[wj][s] = x;
        }
      }
  }
  // the two waves that share a series, wj ascending
  __syncthreads();
  if (tid < PAIRMIN_TJ && j0 + tid < p) {
    float v = red_v[0][tid];
    int x = red_i[0][tid];
    if (pairmin_better(red_v[1][tid], red_i[1][tid], v, x)) {
      v = red_v[1][tid];
      x = red_i[1][tid];
    }
    if (!(wjs[tid] > 0.f)) x = -1;                                      // w[j] <= 0 or NaN
    const int64_t o = (int64_t)blockIdx.y * p + j0 + tid;
    out_v[o] = x < 0 ? __builtin_nanf("") : v;
    out_i[o] = x;
  }
}

// grid ceil(p / 256), block 256: (rmin, partner)[j] = the partials part[c p + j] combined, c ascending
__global__ __launch_bounds__(256) void pairmin_combine_kernel(const float* __restrict__ part_v, const int32_t* __restrict__ part_i,
                                                              int splits, int64_t p, float* __restrict__ rmin,
                                                              int32_t* __restrict__ partner) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p) return;
  float v = part_v[j];
  int x = part_i[j];
  for (int c = 1; c < splits; ++c) {
    const float ov = part_v[(int64_t)c * p + j];
    const int ox = part_i[(int64_t)c * p + j];
    if (pairmin_better(ov, ox, v, x)) {
      v = ov;
      x = ox;
    }
  }
  rmin[j] = x < 0 ? __builtin_nanf("") : v;
  partner[j] = x;
}

}  // namespace eofx
