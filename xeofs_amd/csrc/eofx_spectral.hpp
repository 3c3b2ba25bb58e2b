// eofx_spectral.hpp -- the three device operators of spectral EOF analysis (Towne, Schmidt & Colonius 2018; Schmidt et al.
// 2019; single/spectral_eof.py).  All three are generic linear algebra on float32 operands; none of them knows about Fourier:
// the host builds the coefficient matrix in float64 and rounds it once.
//
//   blockxform   Q[c][b][j] = sum_t B[c, t] T[j, b hop + t]          T [p x n] series-major (ld >= n), B [ncoef x n_fft]
//                (ldb >= n_fft), Q [ncoef][nblk][p] float32 with j contiguous: the transform along time of overlapping blocks of
//                every series.  2 ncoef n_fft nblk p flops on v_mfma_f32_32x32x2_f32; every Q a float32 fma chain, t ascending.
//     blockxform_kernel  workgroup (s, c, z) of (series tiles, coefficient tiles, groups) owns the BLOCKXFORM_TS = 128 series
//                j0 = 128 s .., the BLOCKXFORM_TC = 128 coefficients c0 = 128 c .., and WALKS the blocks
//                [z nblk / groups, (z + 1) nblk / groups) in ascending order.  It walks several blocks, it does not take one:
//                block b + 1 of a series tile re-reads n_overlap of the n_fft samples that block b read, and a workgroup that
//                reads them back to back finds them in the L2 of its own XCD (a tile of 128 series x n_fft samples is
//                128 KiB at n_fft = 256), whereas workgroups of neighbouring blocks are dealt round-robin to the eight XCDs
//                and would each miss.  It also keeps the grid inside (2^31, 65535, 65535) for any nblk.  groups is chosen so
//                that the grid holds about BLOCKXFORM_WGS workgroups (blockxform_plan: a function of the shapes alone; the
//                result does not depend on it, every Q is one chain).
//                The 128 x 128 tile, the staging, the padded LDS rows and the register prefetch are those of
//                eofx_pairmin.hpp / eofx_colquad.hpp: B is the ROW operand (Bs[t][coefficient]), the series are the COLUMN
//                operand (Ts[t][series]), t walked in chunks of 32.  Accumulator register r of lane l is coefficient
//                (r & 3) + 8 (r >> 2) + 4 (l >> 5), series l & 31 of its 32 x 32 block: the 32 lanes of a half-wave store
//                128 contiguous bytes of Q.  A wave whose 64 coefficients are all >= ncoef or whose 64 series are all
//                >= p skips its products (wave-uniform), so a short last tile costs about what it holds.
//     staging    thread (t = tid & 31, g = tid >> 5) loads sample b hop + t0 + t of the 16 series g + 8 e and element t0 + t
//                of the 16 coefficient rows g + 8 e with scalar dword loads: block starts b hop have ANY alignment, nothing
//                assumes 16 bytes.  Indices are clamped (series to p - 1, rows to ncoef - 1, t to n_fft - 1: never past the
//                block, so never past sample n - 1), the loads are unconditional; what is out of range is stored as ZERO in
//                both images (t >= n_fft in both, series >= p, rows >= ncoef): fma(0, 0, c) == c.
//                A NaN or an infinity in series j meets accumulators of column j only.  Nothing outside
//                Q[0 .. ncoef)[0 .. nblk)[0 .. p) is written.
//
//   rowgram      G[f] = R_f R_f^T (float64, r x r) of nb slabs R_f [r x p] (float32, contiguous, slab stride r p).
//     rowgram_kernel     workgroup (tile pair, split c, slab f): the product tile of pairmin_kernel with R_f as both
//                operands and the features as the chain.  The features are walked in spans of ROWGRAM_SPAN = 2048: inside a
//                span float32 fma chains on the matrix cores (feature ascending), at the end of a span the accumulators are
//                converted to float64 and ADDED to the workgroup's own partial in the arena (first span: stored), span
//                ascending; only the thread that owns an element touches it.  Split c of `splits` takes the spans
//                [c spans / splits, (c + 1) spans / splits).  Only tile pairs ta <= tb are computed, and a 32 x 32 block whose
//                rows or columns are all >= r is skipped (wave-uniform): with r <= 32 one product of sixteen is left.
//     rowgram_finish_kernel  G[f][a][b] = G[f][b][a] = the partials of (a, b), a <= b, added over c ascending: the result
//                equals its transpose bit for bit by construction.
//                rowgram_plan is a function of (r, p, nb) alone -- the split of (r, p) alone, so G[f] does not depend on
//                the batch a slab is computed in; no atomics; two runs are equal bit for bit.
//
//   slabmul      out[f] [q x p] = W[f] [q x r] R_f [r x p], float32 fma chains over the r rows ascending.  2 q r p nb flops
//                against 4 r p nb bytes read: q / 2 flops per byte, at most 8 for q <= SLABMUL_QMAX = 16, far below the
//                ~20 flops per byte at which the float32 VALU of an MI355X catches up with its HBM -- the operator is bound
//                by reading R once, the matrix cores would buy nothing, so it is a VALU kernel: W[f] transposed in LDS
//                (Ws[i][m], read as broadcast 16-byte words), every thread owns two features (j and j + 256 of a block of
//                512: coalesced dword loads of a row of R_f) and QT accumulators each, QT = 8 or 16 >= q.
// gfx950 only.
// The constants and the plans are plain C++: a host compiler that does not define __HIPCC__ sees them and not the kernels
// (tests/spectral_shim.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "eofx.h"
#define EOFX_SPECTRAL_HD __host__ __device__ __forceinline__
#else
#define EOFX_SPECTRAL_HD inline
#endif

namespace eofx {

constexpr int BLOCKXFORM_NFFT_MAX = 16384;     // samples per block
constexpr int BLOCKXFORM_NCOEF_MAX = 8192;     // rows of B: 64 coefficient tiles
constexpr int BLOCKXFORM_TC = 128;             // coefficients per workgroup (64 per wave)
constexpr int BLOCKXFORM_TS = 128;             // series per workgroup (64 per wave)
constexpr int BLOCKXFORM_KC = 32;              // samples t per chunk
constexpr int BLOCKXFORM_LD = BLOCKXFORM_TS + 1;       // floats between two t of the LDS images (odd: see eofx_pairmin.hpp)
constexpr int BLOCKXFORM_WGS = 1024;           // workgroups the block groups aim at: four per CU
constexpr int BLOCKXFORM_GMAX = 65535;         // groups of blocks, at most (grid z)

constexpr int ROWGRAM_RMAX = 512;              // rows of a slab
constexpr int ROWGRAM_SPAN = 2048;             // features per float32 chain
constexpr int ROWGRAM_SMAX = 16;               // splits of the spans, at most
constexpr int ROWGRAM_NBMAX = 65535;           // slabs per call (grid z)
constexpr int ROWGRAM_T = 128;                 // rows per tile
constexpr int ROWGRAM_KC = 32;
constexpr int ROWGRAM_LD = ROWGRAM_T + 1;

constexpr int SLABMUL_QMAX = 16;               // rows of W[f]
constexpr int SLABMUL_RMAX = ROWGRAM_RMAX;     // rows of a slab
constexpr int SLABMUL_NBMAX = 65535;           // slabs per call (grid y)
constexpr int SLABMUL_TP = 512;                // features per workgroup: two per thread

// ---- plans: functions of the shapes alone ---------------------------------------------------------------------------------
struct BlockxformPlan {
  int64_t stiles;      // ceil(p / 128)
  int ctiles;          // ceil(ncoef / 128)
  int groups;          // clamp(ceil(BLOCKXFORM_WGS / (stiles ctiles)), 1, min(nblk, BLOCKXFORM_GMAX))
};
inline BlockxformPlan blockxform_plan(int64_t p, int64_t ncoef, int64_t nblk) {
  BlockxformPlan pl;
  pl.stiles = (p + BLOCKXFORM_TS - 1) / BLOCKXFORM_TS;
  pl.ctiles = (int)((ncoef + BLOCKXFORM_TC - 1) / BLOCKXFORM_TC);
  const int64_t wgs = (pl.stiles > 0 ? pl.stiles : 1) * (pl.ctiles > 0 ? pl.ctiles : 1);
  int64_t g = (BLOCKXFORM_WGS + wgs - 1) / wgs;
  if (g > nblk) g = nblk;
  if (g > BLOCKXFORM_GMAX) g = BLOCKXFORM_GMAX;
  if (g < 1) g = 1;
  pl.groups = (int)g;
  return pl;
}
// group z of `groups` walks the blocks spectral_first(nblk, groups, z) .. spectral_first(nblk, groups, z + 1) - 1
EOFX_SPECTRAL_HD int64_t spectral_first(int64_t count, int parts, int z) { return (int64_t)z * count / parts; }

struct RowgramPlan {
  int rt;              // ceil(r / 128): tiles of rows; the grid holds rt * rt tile pairs, those with ta > tb leave at once
  int64_t spans;       // ceil(p / ROWGRAM_SPAN)
  int splits;          // min(spans, max(1, ROWGRAM_SMAX / (rt (rt + 1) / 2))): NOT a function of nb, so G[f] of a slab is the
};                     // same bit for bit in whatever batch it is computed; the partials take at most nb x 2 MiB
inline RowgramPlan rowgram_plan(int64_t r, int64_t p, int64_t nb) {
  (void)nb;            // (the grid is (rt rt, splits, nb))
  RowgramPlan pl;
  pl.rt = (int)((r + ROWGRAM_T - 1) / ROWGRAM_T);
  pl.spans = (p + ROWGRAM_SPAN - 1) / ROWGRAM_SPAN;
  const int pairs = pl.rt > 0 ? pl.rt * (pl.rt + 1) / 2 : 1;
  int64_t s = ROWGRAM_SMAX / pairs;
  if (s > pl.spans) s = pl.spans;
  if (s < 1) s = 1;
  pl.splits = (int)s;
  return pl;
}
inline int slabmul_qt(int64_t q) { return q <= 8 ? 8 : 16; }          // accumulators per feature of the kernel that runs

#if defined(__HIPCC__)
typedef float spectral_f32x16 __attribute__((ext_vector_type(16)));

// ---- blockxform -------------------------------------------------------------------------------------------------------------
// grid (stiles, ctiles, groups), block 256
__global__ __launch_bounds__(256, 2) void blockxform_kernel(const float* __restrict__ T, int64_t p, int64_t ld,
                                                            const float* __restrict__ B, int ncoef, int nfft, int64_t ldb,
                                                            int64_t hop, int64_t nblk, float* __restrict__ Q) {
  __shared__ float Bs[BLOCKXFORM_KC * BLOCKXFORM_LD];
  __shared__ float Ts[BLOCKXFORM_KC * BLOCKXFORM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int64_t j0 = (int64_t)blockIdx.x * BLOCKXFORM_TS;
  const int c0 = (int)blockIdx.y * BLOCKXFORM_TC;
  const int64_t b_lo = spectral_first(nblk, (int)gridDim.z, (int)blockIdx.z);
  const int64_t b_hi = spectral_first(nblk, (int)gridDim.z, (int)blockIdx.z + 1);
  const int st = tid & 31, sg = tid >> 5;                               // staging: this thread's t of a chunk, its rows sg + 8 e
  const bool wave_on = c0 + 64 * wi < ncoef && j0 + 64 * wj < p;        // (wave-uniform) this wave's 64 x 64 block holds anything
  for (int64_t blk = b_lo; blk < b_hi; ++blk) {
    const float* __restrict__ Tb = T + blk * hop;
    spectral_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    float br[BLOCKXFORM_KC / 2], tr[BLOCKXFORM_KC / 2];
    const auto fetch = [&](int t0) {
      const int tc = t0 + st < nfft ? t0 + st : nfft - 1;
#pragma unroll
      for (int e = 0; e < BLOCKXFORM_KC / 2; ++e) {
        const int gc = c0 + sg + 8 * e;
        const int64_t gj = j0 + sg + 8 * e;
        br[e] = B[(int64_t)(gc < ncoef ? gc : ncoef - 1) * ldb + tc];
        tr[e] = Tb[(gj < p ? gj : p - 1) * ld + tc];
      }
    };
    fetch(0);
    for (int t0 = 0; t0 < nfft; t0 += BLOCKXFORM_KC) {
      __syncthreads();                                                  // the products of the previous chunk have read the LDS
#pragma unroll
      for (int e = 0; e < BLOCKXFORM_KC / 2; ++e) {
        Bs[st * BLOCKXFORM_LD + sg + 8 * e] = (t0 + st < nfft && c0 + sg + 8 * e < ncoef) ? br[e] : 0.f;
        Ts[st * BLOCKXFORM_LD + sg + 8 * e] = (t0 + st < nfft && j0 + sg + 8 * e < p) ? tr[e] : 0.f;
      }
      if (t0 + BLOCKXFORM_KC < nfft) fetch(t0 + BLOCKXFORM_KC);         // the next chunk is on its way during the products
      __syncthreads();
      const int steps = ((nfft - t0 < BLOCKXFORM_KC ? nfft - t0 : BLOCKXFORM_KC) + 1) / 2;
      for (int u = 0; wave_on && u < steps; ++u) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = Bs[(2 * u + lh) * BLOCKXFORM_LD + 64 * wi + 32 * a + lr];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = Ts[(2 * u + lh) * BLOCKXFORM_LD + 64 * wj + 32 * b + lr];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
    // the store: register r of lane l is coefficient (r & 3) + 8 (r >> 2) + 4 (l >> 5), series l & 31 of its block
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int64_t j = j0 + 64 * wj + 32 * b + lr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = c0 + 64 * wi + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (c < ncoef && j < p) Q[((int64_t)c * nblk + blk) * p + j] = acc[a][b][r];
        }
      }
  }
}

// ---- rowgram ----------------------------------------------------------------------------------------------------------------
// grid (rt * rt, splits, nb), block 256.  part [nb][splits][r][r] float64: the partial of split c (elements of the tile pairs
// ta <= tb)
__global__ __launch_bounds__(256, 2) void rowgram_kernel(const float* __restrict__ R, int r, int64_t p, int rt, int64_t spans,
                                                         double* __restrict__ part) {
  const int ta = (int)blockIdx.x / rt, tb = (int)blockIdx.x % rt;
  if (ta > tb) return;                                                  // (uniform: before any barrier)
  __shared__ float As[ROWGRAM_KC * ROWGRAM_LD];
  __shared__ float Bs[ROWGRAM_KC * ROWGRAM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int a0 = ta * ROWGRAM_T, b0 = tb * ROWGRAM_T;
  const int splits = (int)gridDim.y, c = (int)blockIdx.y;
  const int64_t f = blockIdx.z;
  const float* __restrict__ Rf = R + f * (int64_t)r * p;
  double* __restrict__ out = part + (f * splits + c) * (int64_t)r * r;
  const int64_t s_lo = spectral_first(spans, splits, c), s_hi = spectral_first(spans, splits, c + 1);
  const int st = tid & 31, sg = tid >> 5;
  bool row_on[2], col_on[2];                                            // (wave-uniform) the 32 x 32 blocks that hold anything: with
#pragma unroll                                                          //  r <= 32 one product of the sixteen of a workgroup is left
  for (int a = 0; a < 2; ++a) row_on[a] = a0 + 64 * wi + 32 * a < r;
#pragma unroll
  for (int b = 0; b < 2; ++b) col_on[b] = b0 + 64 * wj + 32 * b < r;
  const bool wave_on = row_on[0] && col_on[0];
  for (int64_t s = s_lo; s < s_hi; ++s) {
    const int64_t k_lo = s * ROWGRAM_SPAN;
    const int klen = (int)(p - k_lo < ROWGRAM_SPAN ? p - k_lo : ROWGRAM_SPAN);
    spectral_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;
    float ar[ROWGRAM_KC / 2], br[ROWGRAM_KC / 2];
    const auto fetch = [&](int t0) {
      const int64_t tc = k_lo + (t0 + st < klen ? t0 + st : klen - 1);
#pragma unroll
      for (int e = 0; e < ROWGRAM_KC / 2; ++e) {
        const int ga = a0 + sg + 8 * e, gb = b0 + sg + 8 * e;
        ar[e] = Rf[(int64_t)(ga < r ? ga : r - 1) * p + tc];
        br[e] = Rf[(int64_t)(gb < r ? gb : r - 1) * p + tc];
      }
    };
    fetch(0);
    for (int t0 = 0; t0 < klen; t0 += ROWGRAM_KC) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < ROWGRAM_KC / 2; ++e) {
        As[st * ROWGRAM_LD + sg + 8 * e] = (t0 + st < klen && a0 + sg + 8 * e < r) ? ar[e] : 0.f;
        Bs[st * ROWGRAM_LD + sg + 8 * e] = (t0 + st < klen && b0 + sg + 8 * e < r) ? br[e] : 0.f;
      }
      if (t0 + ROWGRAM_KC < klen) fetch(t0 + ROWGRAM_KC);
      __syncthreads();
      const int steps = ((klen - t0 < ROWGRAM_KC ? klen - t0 : ROWGRAM_KC) + 1) / 2;
      for (int u = 0; wave_on && u < steps; ++u) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = As[(2 * u + lh) * ROWGRAM_LD + 64 * wi + 32 * a + lr];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = Bs[(2 * u + lh) * ROWGRAM_LD + 64 * wj + 32 * b + lr];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            if (row_on[a] && col_on[b]) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
    // this span's chains, in float64, onto the partial of the spans before (only this thread touches its elements)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = b0 + 64 * wj + 32 * b + lr;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = a0 + 64 * wi + 32 * a + (q & 3) + 8 * (q >> 2) + 4 * lh;
          if (row < r && col < r) {
            const int64_t o = (int64_t)row * r + col;
            double v = (double)acc[a][b][q];
            if (s > s_lo) v = out[o] + v;
            out[o] = v;
          }
        }
      }
  }
}

// grid (ceil(r r / 256), nb), block 256: G[f][a][b] = G[f][b][a] = the partials of (a, b), a <= b, c ascending
__global__ __launch_bounds__(256) void rowgram_finish_kernel(const double* __restrict__ part, int splits, int r,
                                                             double* __restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)r * r) return;
  const int a = (int)(e / r), b = (int)(e % r);
  if (a > b) return;
  const int64_t f = blockIdx.y, rr = (int64_t)r * r;
  double v = part[f * splits * rr + e];
  for (int c = 1; c < splits; ++c) v += part[(f * splits + c) * rr + e];
  G[f * rr + e] = v;
  G[f * rr + (int64_t)b * r + a] = v;
}

// ---- slabmul ----------------------------------------------------------------------------------------------------------------
// grid (ceil(p / 512), nb), block 256
template <int QT>
__global__ __launch_bounds__(256) void slabmul_kernel(const float* __restrict__ W, const float* __restrict__ R, int q, int r,
                                                      int64_t p, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float Ws[SLABMUL_RMAX * QT];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.y;
  const float* __restrict__ Wf = W + f * (int64_t)q * r;
  const float* __restrict__ Rf = R + f * (int64_t)r * p;
  for (int e = tid; e < r * QT; e += 256) {
    const int i = e / QT, m = e % QT;
    Ws[e] = m < q ? Wf[(int64_t)m * r + i] : 0.f;
  }
  __syncthreads();
  const int64_t j0 = (int64_t)blockIdx.x * SLABMUL_TP + tid, j1 = j0 + 256;
  const int64_t c0 = j0 < p ? j0 : p - 1, c1 = j1 < p ? j1 : p - 1;     // clamped: the loads are unconditional
  float acc0[QT], acc1[QT];
#pragma unroll
  for (int m = 0; m < QT; ++m) acc0[m] = acc1[m] = 0.f;
  for (int i = 0; i < r; ++i) {
    const float x0 = Rf[(int64_t)i * p + c0], x1 = Rf[(int64_t)i * p + c1];
#pragma unroll
    for (int m = 0; m < QT; ++m) {
      const float w = Ws[i * QT + m];
      acc0[m] = __builtin_fmaf(w, x0, acc0[m]);
      acc1[m] = __builtin_fmaf(w, x1, acc1[m]);
    }
  }
  float* __restrict__ of = out + f * (int64_t)q * p;
#pragma unroll
  for (int m = 0; m < QT; ++m)
    if (m < q) {
      if (j0 < p) of[(int64_t)m * p + j0] = acc0[m];
      if (j1 < p) of[(int64_t)m * p + j1] = acc1[m];
    }
}

#endif  // __HIPCC__

}  // namespace eofx
