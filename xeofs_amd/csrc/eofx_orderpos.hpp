// eofx_orderpos.hpp -- the rank-order operator of trend EOF analysis (Hannachi 2007; single/trend_eof.py): for every series
// (row) of a series-major float32 panel T [p x n],
//
//     Q[j, r] = the time index t of the r-th smallest value of series j, equal values in ascending time
//               (numpy.argsort(kind="stable"); -0.0 equals +0.0; every NaN sorts last, in time order),
//     Z[j, r] = (float)(((double)Q[j, r] - (n - 1) / 2) * scale[j])            (the float64 product, rounded once)
//
//   orderpos_kernel   one pass: a series is read once, sorted on chip, written once.  Keys are 64-bit: the order-preserving
//                     integer image of the float (orderpos_vkey) in the high word, the time index in the low word -- all keys
//                     of a series differ, so ANY sorting network returns the stable argsort and two runs are equal bit for
//                     bit.  The series is padded to m = max(8, next power of two of n) with keys above every real one
//                     (value word 0xffffffff, index i >= n at position i).
//   the network       bitonic on m positions in the form whose every compare-exchange leaves the smaller key at the LOWER
//                     position: merge phase k (blocks of k positions) starts with the mirror step i <-> i ^ (k - 1) and goes
//                     on with the strides k / 4 .. 1.  The padding key of position i >= n therefore never moves: it is never
//                     stored, a read of it is made up in registers, and a thread whose positions all lie past n does nothing
//                     -- the work and the LDS follow n, not m.
//   three steps a pass  A thread takes 8 keys per pass and runs THREE steps on them in registers (strides 4s, 2s, s; in the
//                     first pass of a phase the mirror step and the strides 2s, s on the 4 positions base + e s and their 4
//                     mirror images), so a phase of L steps costs ceil(L / 3) trips through LDS and barriers instead of L;
//                     the steps left over (L mod 3) go first, as one pass of 2 or 4 keys per thread.  The groups are aligned
//                     from stride 1 upwards, so s is a power of 8.  The first pass sorts 8 contiguous samples straight from
//                     global memory (the phases 2, 4, 8) and the last one writes the outputs straight from registers: 8
//                     consecutive positions per thread.  m = 16384: 105 steps in 36 passes.
//   LDS image         key i lives at i ^ ((i >> 5) & 7) ^ (((i >> 6) & 3) << 3) -- 8-byte slots, 32 to a 256-byte bank row; a
//                     half-wave's 32 reads of one pass land on 32 different slots for s = 1 and s = 8 and, untouched by the
//                     swizzle, for s >= 64 (MI355X: ds_read_b64 is serviced per 32-lane half).  A mirror image i ^ (k - 1)
//                     complements the low bits of i: as many different slots.
//   tiers             by the padded length m (orderpos_plan): m <= 2048 -- 256 threads, m / 8 of them per series and
//                     2048 / m series per workgroup; m = 4096 -- 512 threads; m = 8192 and 16384 -- 1024 threads.  Dynamic
//                     LDS: m keys per series up to m = 1024, above that the n keys of the series (rounded up to 32): 78 KiB
//                     at n = 10000 -- two workgroups of 16 waves per CU -- and 128 KiB at n = 16384.  A workgroup loops over
//                     its groups of series: the grid is bounded by the CU count, not by p.
// Reads and writes of a series are contiguous; nothing is written past column n of a row; no atomics.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "eofx.h"

namespace eofx {

constexpr int ORDERPOS_NMAX = 16384;        // samples of a series: 16384 keys of 8 bytes are 128 KiB of the 160 KiB of a CU
constexpr int ORDERPOS_MMIN = 8;            // the shortest padded length: one thread's 8 keys

// launch shape of orderpos_kernel for series of n samples (a function of n alone)
struct OrderposPlan {
  int m;          // padded length: a power of two, >= ORDERPOS_MMIN
  int threads;    // workgroup size
  int tps;        // threads per series
  int spb;        // series per workgroup
  int keys;       // LDS slots of one series
  size_t lds;     // dynamic LDS in bytes: spb * keys keys
  int per_cu;     // workgroups a CU holds (LDS and the 2048-thread limit)
};
inline OrderposPlan orderpos_plan(int64_t n) {
  OrderposPlan pl;
  int m = ORDERPOS_MMIN;
  while (m < n) m <<= 1;
  pl.m = m;
  if (m <= 2048) {
    pl.threads = 256;
    pl.tps = m / 8;
    pl.spb = 256 / pl.tps;
  } else {
    pl.threads = m == 4096 ? 512 : 1024;
    pl.tps = pl.threads;
    pl.spb = 1;
  }
  pl.keys = m <= 1024 ? m : (int)((n + 31) / 32 * 32);      // (the slot map permutes aligned blocks of 32)
  pl.lds = (size_t)pl.spb * pl.keys * sizeof(uint64_t);
  const int by_lds = (int)(163840 / pl.lds), by_threads = 2048 / pl.threads;
  pl.per_cu = by_lds < by_threads ? by_lds : by_threads;
  return pl;
}

// the order-preserving 32-bit image of a float: -0.0 -> +0.0 first, negative values complemented, the others with the sign
// bit set; every NaN (any sign, any payload) -> 0xffffffff, above +inf (0xff800000)
__host__ __device__ __forceinline__ uint32_t orderpos_vkey(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the padding key of position i >= n: above every real key, and ascending in i
__host__ __device__ __forceinline__ uint64_t orderpos_pad(int i) { return ((uint64_t)0xffffffffu << 32) | (uint32_t)i; }
// LDS slot of key i of a series (a bijection of every aligned block of 32 slots)
__host__ __device__ __forceinline__ int orderpos_slot(int i) { return i ^ ((i >> 5) & 7) ^ (((i >> 6) & 3) << 3); }

// the smaller key to a (the lower position), the larger to b
__host__ __device__ __forceinline__ void orderpos_cx(uint64_t& a, uint64_t& b) {
  const uint64_t x = a, y = b;
  const bool sw = x > y;
  a = sw ? y : x;
  b = sw ? x : y;
}

// the phases 2, 4 and 8 on 8 contiguous keys: v[e] = the key of position base + e
__host__ __device__ __forceinline__ void orderpos_sort8(uint64_t (&v)[8]) {
#pragma unroll
  for (int kk = 2; kk <= 8; kk <<= 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (!(e & (kk >> 1))) orderpos_cx(v[e], v[e ^ (kk - 1)]);             // the mirror step
#pragma unroll
    for (int h = kk >> 2; h >= 1; h >>= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (!(e & h)) orderpos_cx(v[e], v[e | h]);
  }
}

// R steps of merge phase k on the 2^R keys of every item u = tl, tl + tps, ... < m / 2^R of this thread, s = 2^b:
//   MIRROR (the first pass of a phase, 2^R s = k): the mirror step, then the strides 2^(R-2) s .. s, on the positions
//          base + e s (e < 2^(R-1)) and their mirror images (base + e s) ^ (k - 1);
//   else:  the strides 2^(R-1) s .. s on the positions base + e s (e < 2^R).
// base: u with R zero bits inserted at bit b -- the lowest position of the item, so an item with base >= n holds padding
// only.  Positions >= n are made up on the way in and dropped on the way out.  out(i, key): where the keys go.
template <int R, bool MIRROR, class Out>
__host__ __device__ __forceinline__ void orderpos_pass(const uint64_t* key, int n, int m, int k, int b, int tl, int tps, Out out) {
  constexpr int E = 1 << R, H = E >> 1;
  const int s = 1 << b;
  for (int u = tl; u < (m >> R); u += tps) {
    const int base = ((u >> b) << (b + R)) | (u & (s - 1));
    if (base >= n) break;                                     // (base ascends with u)
    int pos[E];
    uint64_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      pos[e] = MIRROR ? (e < H ? base + e * s : (base + (e - H) * s) ^ (k - 1)) : base + e * s;
      v[e] = pos[e] < n ? key[orderpos_slot(pos[e])] : orderpos_pad(pos[e]);
    }
    if (MIRROR) {
#pragma unroll
      for (int e = 0; e < H; ++e) orderpos_cx(v[e], v[H + e]);
#pragma unroll
      for (int h = H >> 1; h >= 1; h >>= 1)
#pragma unroll
        for (int e = 0; e < H; ++e)
          if (!(e & h)) {
            orderpos_cx(v[e], v[e | h]);
            orderpos_cx(v[H + (e | h)], v[H + e]);            // (the mirror images descend with e)
          }
    } else {
#pragma unroll
      for (int h = H; h >= 1; h >>= 1)
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (!(e & h)) orderpos_cx(v[e], v[e | h]);
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (pos[e] < n) out(pos[e], v[e]);
  }
}

// grid <= ceil(p / spb), block pl.threads, dynamic LDS pl.lds (pl = orderpos_plan(n); m, tps, spb, keys from it).
// T [p x n] with row stride ld; scale [p] float64 or NULL (ones); Qi [p x n] int32 (row stride ldq) and Zt [p x n] float32 (row
// stride ldz), either may be NULL.
__global__ __launch_bounds__(1024) void orderpos_kernel(const float* __restrict__ T, int64_t p, int n, int64_t ld,
                                                         const double* __restrict__ scale, int* __restrict__ Qi, int64_t ldq,
                                                         float* __restrict__ Zt, int64_t ldz, int m, int tps, int spb, int keys) {
  extern __shared__ uint64_t orderpos_lds[];
  const int sl = threadIdx.x / tps, tl = threadIdx.x - sl * tps;       // series of the group, thread of the series
  uint64_t* key = orderpos_lds + (size_t)sl * keys;
  const double centre = 0.5 * (double)(n - 1);
  const int64_t groups = (p + spb - 1) / spb;
  int logm = 3;
  while ((1 << logm) < m) ++logm;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t j = g * spb + sl;
    const int nj = j < p ? n : 0;                    // (a series past p: no position is real, every pass falls through)
    const float* src = T + (j < p ? j : 0) * ld;
    const double sc = (j < p && scale) ? scale[j] : 1.0;
    int* q_row = (j < p && Qi) ? Qi + j * ldq : nullptr;
    float* z_row = (j < p && Zt) ? Zt + j * ldz : nullptr;
    const auto emit = [&](int r, uint64_t kv) {      // position r < n of the sorted series
      const int q = (int)(uint32_t)kv;
      if (q_row) q_row[r] = q;
      if (z_row) z_row[r] = (float)(((double)q - centre) * sc);
    };
    const auto to_lds = [&](int i, uint64_t kv) { key[orderpos_slot(i)] = kv; };
    // 8 contiguous samples per thread from global memory, the phases 2, 4, 8 in registers
    for (int u = tl; (u << 3) < nj; u += tps) {
      const int base = u << 3;
      uint64_t v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = base + e;
        v[e] = t < nj ? ((uint64_t)orderpos_vkey(__float_as_uint(src[t])) << 32) | (uint32_t)t : orderpos_pad(t);
      }
      orderpos_sort8(v);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (base + e < nj) {
          if (m == 8) emit(base + e, v[e]);
          else to_lds(base + e, v[e]);
        }
    }
    // merge phases k = 16 .. m: L = log2 k steps; the mirror step with the L mod 3 (or 3) top steps, then groups of three
    for (int L = 4; L <= logm; ++L) {
      const int k = 1 << L, r = L % 3;
      __syncthreads();
      if (r == 1) orderpos_pass<1, true>(key, nj, m, k, L - 1, tl, tps, to_lds);
      if (r == 2) orderpos_pass<2, true>(key, nj, m, k, L - 2, tl, tps, to_lds);
      if (r == 0) orderpos_pass<3, true>(key, nj, m, k, L - 3, tl, tps, to_lds);
      __syncthreads();
      for (int b = L - (r ? r : 3) - 3; b > 0; b -= 3) {
        orderpos_pass<3, false>(key, nj, m, k, b, tl, tps, to_lds);
        __syncthreads();
      }
      if (L < logm) orderpos_pass<3, false>(key, nj, m, k, 0, tl, tps, to_lds);
      else orderpos_pass<3, false>(key, nj, m, k, 0, tl, tps, emit);
    }
    __syncthreads();      // the next group overwrites the LDS
  }
}

}  // namespace eofx
