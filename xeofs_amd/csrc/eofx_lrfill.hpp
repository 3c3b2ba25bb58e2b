// eofx_lrfill.hpp -- the gap operators of DINEOF (Beckers & Rixen 2003): EOF analysis of a field with isolated missing values
// as an EM iteration -- fit a rank-k truncated SVD, write the rank-k reconstruction into the gaps, repeat.
//
//     gapmask   bit (j & 31) of bits[i ldb + (j >> 5)] = isnan(X[i, j]),      count = the number of set bits
//     lrfill    F[i, j] <- sum_{m < k} A[i, m] B[j, m]   where the bit of (i, j) is set, in place, with
//               sums = (count, sum (new - old)^2, sum new^2) over the written entries
//
// (X, F [n x p] float32, row stride ld; bits [n x ceil(p / 32)] 32-bit words, row stride ldb; A [n x k] the scores U diag(s)
// and B [p x k] the components, float32 panels with row strides lda, ldbm >= k.)
//   gapmask_kernel          a wave reads 8 x 64 consecutive columns of one row per step (one coalesced 256 B row segment per
//                           load, eight loads in flight); each ballot yields two words, lanes 0 .. 15 store the sixteen words.
//                           Columns >= p count as valid, so the tail bits of the last word are zeros; words past
//                           ceil(p / 32) are not written.  NaN is tested on the bit pattern (any payload, either sign).
//                           A grid of G <= LRFILL_WGS workgroups strides over the (row, 512 columns) units; the wave's
//                           population count is an integer, the workgroup's goes to slot g.
//   lrfill_kernel           workgroup g of G <= LRFILL_WGS walks the tiles g, g + G, ... of 128 x 128 outputs (tile t = row block
//                           t % nbi, column block t / nbi: workgroups that run together share column blocks, so the B slabs
//                           are re-read from L2).  Wave (wi, wj) of four owns the 64 x 64 block, a 2 x 2 block of 32 x 32
//                           accumulators of v_mfma_f32_32x32x2_f32 -- float32 operands, bitwise an fmaf chain over m.
//                           Per tile: the 128 x 4 mask words go to LDS first, bits outside the matrix cleared (rows >= n,
//                           columns >= p: whatever the caller left in the last word is ignored); a tile without a bit is left
//                           at once (workgroup-uniform): no product, no byte of F.  Otherwise k is walked in chunks of 32:
//                           thread (row = tid >> 1, half = tid & 1) loads 16 consecutive m of its row of A and of B (a pair
//                           of lanes covers 128 contiguous bytes; indices out of range are clamped, so the 32 loads are
//                           unconditional and in flight together) and stores them transposed, As[m][row], Bs[m][column]
//                           (rows, columns and m out of range as zeros: fma(0, 0, c) == c).  A 32 x 32 block without a bit
//                           issues no product (wave-uniform).
//     LDS image             As, Bs [32][128] floats, 2 x 16 KiB, + 2 KiB of mask words.  Operand read: lane l takes
//                           As[2 s + (l >> 5)][row0 + (l & 31)] -- ds_read_b32 is served in the lane groups {0-31}, {32-63} over
//                           32 banks, and a group reads 32 consecutive dwords: conflict-free without padding.  Staging store:
//                           a group of 32 lanes holds 16 rows x 2 halves, the halves 16 x 128 dwords apart = the same bank,
//                           a 2-way conflict, which a ds_write_b32 hides behind its own register transfer.
//     old values, epilogue  accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31: the
//                           32 lanes of a row segment share one mask word (an LDS broadcast) and test their own bit.  Only a
//                           set bit reads the old value and stores the new one (128 B coalesced per row segment), through
//                           one buffer resource per register: it covers rows x and x + 4 of the block (the two half-waves),
//                           4 ld + 32 entries.  A clear bit is the offset just past the resource, where a load returns 0 and
//                           a store is dropped without touching memory: no load or store sits behind a branch, and the 16
//                           loads of a 32 x 32 block are in flight together.  Hence ld <= 2^26 (LRFILL_LDMAX).
//   lrfill_finish_kernel    the partials of slot g (count, sum d^2, sum new^2; float64, count an exact integer) are summed by one
//                           workgroup: thread t the slots t, t + 256, ... ascending, then thread 0 the 256 sums ascending.
// No atomics; G and the tile walk are functions of (n, p) alone, the order inside a workgroup is fixed: two runs are equal bit
// for bit in F and in the sums.  Scratch: LRFILL_WGS x 3 doubles whatever n and p.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"

namespace eofx {

constexpr int LRFILL_KMAX = 256;         // modes
constexpr int64_t LRFILL_LDMAX = (int64_t)1 << 26;      // row stride of F in entries (a buffer resource covers 4 ld + 32 of them)
constexpr int LRFILL_T = 128;            // rows and columns of F per tile (64 per wave)
constexpr int LRFILL_KC = 32;            // modes per chunk
constexpr int LRFILL_WGS = 2048;         // workgroups at most; also the bound of the partial slots
constexpr int GAPMASK_COLS = 512;        // columns of one row per wave step (eight loads in flight)

typedef float lrfill_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool lrfill_isnan_bits(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u; }
// (a raw buffer over `bytes` bytes from `base`, as row_rsrc of eofx_hfft.hpp: an offset beyond it reads 0 / stores nothing)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lrfill_rsrc(float* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000);
}

// grid G, block 256.  part [G] = set bits of the units of workgroup g.
__global__ __launch_bounds__(256) void gapmask_kernel(const float* __restrict__ X, int64_t n, int64_t p, int64_t ld,
                                                      unsigned* __restrict__ bits, int64_t ldb, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nwords = (p + 31) / 32, nchunks = (p + GAPMASK_COLS - 1) / GAPMASK_COLS;
  const int64_t units = n * nchunks, stride = (int64_t)gridDim.x * 4;
  constexpr int Q = GAPMASK_COLS / 64;
  const int64_t di = stride / nchunks, dc = stride % nchunks;      // the step of (row, chunk): no division inside the loop
  unsigned long long count = 0;
  int64_t u = (int64_t)blockIdx.x * 4 + wave;
  int64_t i = u / nchunks, c = u % nchunks;
  for (; u < units; u += stride) {
    const unsigned* row = reinterpret_cast<const unsigned*>(X) + i * ld;
    unsigned v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int64_t j = c * GAPMASK_COLS + 64 * q + lane;
      v[q] = row[j < p ? j : p - 1];               // (clamped, not predicated: the Q loads are issued together)
    }
    unsigned mine = 0;                             // the word of lane w < 2 Q: half (w & 1) of ballot w >> 1
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const unsigned long long b = __ballot(c * GAPMASK_COLS + 64 * q + lane < p && lrfill_isnan_bits(v[q]));
      count += (unsigned long long)__popcll(b);
      if ((lane >> 1) == q) mine = (unsigned)((lane & 1) ? (b >> 32) : (b & 0xffffffffull));
    }
    if (lane < 2 * Q) {
      const int64_t w = c * (GAPMASK_COLS / 32) + lane;
      if (w < nwords) bits[i * ldb + w] = mine;
    }
    i += di;
    c += dc;
    if (c >= nchunks) {
      c -= nchunks;
      ++i;
    }
  }
  if (lane == 0) red[wave] = count;                // (count is wave-uniform)
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup of 256: out[0] = sum of part[0 .. G) (integers: any order is exact)
__global__ __launch_bounds__(256) void gapmask_finish_kernel(const unsigned long long* __restrict__ part, int G, long long* __restrict__ out) {
  __shared__ unsigned long long red[256];
  unsigned long long s = 0;
  for (int g = threadIdx.x; g < G; g += 256) s += part[g];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int i = 0; i < 256; ++i) t += red[i];
    out[0] = (long long)t;
  }
}

// grid G, block 256.  part [G x 3] = (count, sum (new - old)^2, sum new^2) of the tiles of workgroup g.
__global__ __launch_bounds__(256, 2) void lrfill_kernel(float* __restrict__ F, int64_t n, int64_t p, int64_t ld,
                                                        const unsigned* __restrict__ bits, int64_t ldb, const float* __restrict__ A,
                                                        int64_t lda, const float* __restrict__ B, int64_t ldbm, int k,
                                                        double* __restrict__ part) {
  __shared__ float As[LRFILL_KC * LRFILL_T];
  __shared__ float Bs[LRFILL_KC * LRFILL_T];
  __shared__ unsigned Ms[LRFILL_T * 4];
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int64_t nbi = (n + LRFILL_T - 1) / LRFILL_T, nbj = (p + LRFILL_T - 1) / LRFILL_T, ntiles = nbi * nbj;
  const int64_t nwords = (p + 31) / 32;
  const int srow = tid >> 1, sm0 = (tid & 1) * (LRFILL_KC / 2);          // staging: this thread's row and first m of a chunk
  double cnt = 0.0, sd = 0.0, sn = 0.0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i0 = (t % nbi) * LRFILL_T, j0 = (t / nbi) * LRFILL_T;
    // the tile's mask words, bits outside the matrix cleared
    unsigned mine = 0, mw[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {                                       // (clamped, not predicated: both loads in flight)
      const int w = tid + 256 * e;
      const int64_t gi = i0 + (w >> 2), gw = (j0 >> 5) + (w & 3);
      mw[e] = bits[(gi < n ? gi : n - 1) * ldb + (gw < nwords ? gw : nwords - 1)];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int w = tid + 256 * e;
      const int64_t gi = i0 + (w >> 2), gw = (j0 >> 5) + (w & 3);
      const int64_t left = p - 32 * gw;                                 // columns of this word inside the matrix
      unsigned m = (gi < n && gw < nwords) ? mw[e] : 0u;
      if (left < 32) m &= left > 0 ? (1u << left) - 1u : 0u;
      Ms[w] = m;
      mine |= m;
    }
    if (!__syncthreads_or(mine != 0)) continue;                         // (workgroup-uniform; also orders Ms against its readers)
    bool any[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) any[a][b] = __any(Ms[(64 * wi + 32 * a + lr) * 4 + 2 * wj + b] != 0);
    lrfill_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int64_t ga = i0 + srow, gb = j0 + srow;
    const float* Arow = A + (ga < n ? ga : n - 1) * lda;                // clamped, not predicated: the 32 loads of a chunk are
    const float* Brow = B + (gb < p ? gb : p - 1) * ldbm;               // issued together, and what is out of range becomes 0
    for (int m0 = 0; m0 < k; m0 += LRFILL_KC) {
      if (m0) __syncthreads();                                          // the products of the previous chunk have read the LDS
      float ar[LRFILL_KC / 2], br[LRFILL_KC / 2];
#pragma unroll
      for (int e = 0; e < LRFILL_KC / 2; ++e) {
        const int m = m0 + sm0 + e, mc = m < k ? m : k - 1;
        ar[e] = Arow[mc];
        br[e] = Brow[mc];
      }
#pragma unroll
      for (int e = 0; e < LRFILL_KC / 2; ++e) {
        const bool in = m0 + sm0 + e < k;
        As[(sm0 + e) * LRFILL_T + srow] = (in && ga < n) ? ar[e] : 0.f;
        Bs[(sm0 + e) * LRFILL_T + srow] = (in && gb < p) ? br[e] : 0.f;
      }
      __syncthreads();
      const int steps = ((k - m0 < LRFILL_KC ? k - m0 : LRFILL_KC) + 1) / 2;
      for (int s = 0; s < steps; ++s) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = As[(2 * s + lh) * LRFILL_T + 64 * wi + 32 * a + lr];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = Bs[(2 * s + lh) * LRFILL_T + 64 * wj + 32 * b + lr];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            if (any[a][b]) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (!any[a][b]) continue;
        // Row (r & 3) + 8 (r >> 2) of the block, both half-waves, through one buffer resource: a lane whose bit is clear
        // is given the offset just past the resource, where a load returns 0 without touching memory and a store is
        // dropped -- no branch, so the 16 loads of the old values are in flight together, and only set bits move bytes.
        const unsigned span = (unsigned)(4 * ld + 32) * 4u;             // bytes of rows x and x + 4, columns 0 .. 31 (ld <= LRFILL_LDMAX)
        unsigned off[16];
        float oldv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ru = 64 * wi + 32 * a + (r & 3) + 8 * (r >> 2);
          const unsigned bit = (Ms[(ru + 4 * lh) * 4 + 2 * wj + b] >> lr) & 1u;   // (cleared outside the matrix: gi < n and gj < p)
          off[r] = bit ? (unsigned)(4 * lh * ld + lr) * 4u : span;
          oldv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
              lrfill_rsrc(F + (i0 + ru) * ld + (j0 + 64 * wj + 32 * b), span), off[r], 0, 0));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ru = 64 * wi + 32 * a + (r & 3) + 8 * (r >> 2);
          const bool set = off[r] != span;
          const float nv = acc[a][b][r];
          const double d = (double)nv - (double)oldv[r];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, nv),
                                                lrfill_rsrc(F + (i0 + ru) * ld + (j0 + 64 * wj + 32 * b), span), off[r], 0, 0);
          cnt += set ? 1.0 : 0.0;
          sd += set ? d * d : 0.0;
          sn += set ? (double)nv * (double)nv : 0.0;
        }
      }
    __syncthreads();                                                    // Ms, As, Bs are free for the next tile
  }
  // lanes in a fixed butterfly, waves ascending
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    sd += __shfl_xor(sd, o);
    sn += __shfl_xor(sn, o);
  }
  if (lane == 0) {
    red[wave][0] = cnt;
    red[wave][1] = sd;
    red[wave][2] = sn;
  }
  __syncthreads();
  if (tid < 3) part[(int64_t)blockIdx.x * 3 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one workgroup of 256: sums[c] = sum of part[g x 3 + c], thread t the slots t, t + 256, ... ascending, then t ascending
__global__ __launch_bounds__(256) void lrfill_finish_kernel(const double* __restrict__ part, int G, double* __restrict__ sums) {
  __shared__ double red[3][256];
  double s[3] = {0.0, 0.0, 0.0};
  for (int g = threadIdx.x; g < G; g += 256)
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += part[(int64_t)g * 3 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) red[c][threadIdx.x] = s[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[threadIdx.x][i];
    sums[threadIdx.x] = t;
  }
}

}  // namespace eofx
