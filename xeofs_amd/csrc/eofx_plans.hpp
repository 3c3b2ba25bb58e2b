// eofx_plans.hpp -- every launch plan of the engine, stated once: split factors, tile lists, grid sizes, route predicates and the
// small host tables that go with a launch.  A plan here is a function of the SHAPE alone (plus the documented getenv tuning
// hooks): plain C++17, no HIP, no context, so the host compiler builds it alone and tests/test_plans_cpu.py runs it without a GPU
// (tests/plans_shim.cpp) -- next to the Python restatements the GPU route tests choose their shapes with.  eofx_abi.hip keeps the
// launches, copies, caches and error reporting.  Constants that both a kernel and a plan need are defined here; the kernel
// headers include this one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "eofx.h"

namespace eofx {

// ---- tile sizes shared with the kernels ----------------------------------------------------------------------------------
constexpr int ATB_KG = 32;    // atb kernels: K granularity (slabs are consumed in pairs)
constexpr int ATB_BM = 512;   // atb kernels: A columns per workgroup
constexpr int AXB_KG = 64;    // axb kernels: K granularity (slabs are consumed in pairs)
constexpr int AXB_BM = 256;   // axb kernels: rows per workgroup
constexpr int GR_BM = 256;    // NT kernel (eofx_gram.hpp): tile rows = tile columns
constexpr int GR_BK = 32;     // NT kernel: features per stage, one 128-byte line {hi[32], lo[32]} per row
constexpr int64_t EOFX_GRAM_MAX_SIDE = 32768;
constexpr int SPCA_GMAX = 2048;     // workgroups of the streaming passes of eofx_spca.hpp (a function of the shape only)
constexpr int VIEWCOV_T = 128;           // rows and columns of C per tile (64 per wave)
constexpr int VIEWCOV_K = 16;            // samples per slab
constexpr int VIEWCOV_WGS = 512;         // workgroups aimed at; also the bound of the partial blocks
constexpr int VIEWCOV_SPLIT_SLABS = 16;  // a split takes at least this many slabs (256 samples)
constexpr int FIR_R = 64;                // filter covariances (eofx_lagcov.hpp, eofx_lowpass.hpp): samples per row tile
constexpr int FIR_WIN = 16;              // outputs per thread of the sliding window
constexpr int FIR_PADW = FIR_WIN - 1;    // zeros on either side of the weights
constexpr int LAGCOV_PADW = FIR_PADW, LOWPASS_PADW = FIR_PADW;      // (the names tests/plans_shim.cpp reports either plan's padding under)
constexpr int LAGCOV_PMAX = 1024;        // columns of S (the partials stay within 8 workgroups x 8 MiB at the limit)
constexpr int LAGCOV_FUSE_NTAU = 65;     // a row tile and its ntau - 1 halo rows fit the 128 staged rows up to here
constexpr int LAGCOV_WGS = 512;          // workgroups aimed at (two per CU fit the LDS of the fused kernel)
constexpr int LOWPASS_WGS = 512;          // workgroups aimed at (two per CU)
constexpr int64_t LOWPASS_PART_MAX = (int64_t)1 << 23;      // doubles of partials (64 MiB)
// Lags are processed in groups whose side-by-side sample panel is at most this many columns wide: the wide product then
// stays on the wide-panel kernels (the MFMA NT kernel of eofx_gram.hpp from 512 columns, the 128-column streaming tiles
// below) while E = 100 lags of a 64-column panel do not ask for a 6400-column intermediate.  The field is read once
// per group.
constexpr int EOFX_LAG_GROUP_COLS = 1024;

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

#if defined(__HIPCC__)
#define EOFX_HOST_DEVICE __host__ __device__
#else
#define EOFX_HOST_DEVICE
#endif
// ---- the fp16 planes of an X Y pass's panel (eofx_axb_dma.hpp) -----------------------------------------------------------
// A tall panel [K_all x L] (K_all a multiple of AXB_KG) as two fp16 planes (hi, lo) in the order axb_f16_dma_kernel's LDS buffer
// holds them: [column block of 64][feature pair of 64 features][plane][k-group of 8 features][column slot][8 halves], the slot
// of column c being c ^ ((c >> 3) & 7).  One pair is AXB_PAIR_BYTES; a (k-group, column) of one plane is one 16-byte unit.
constexpr int AXB_PLANE_BYTES = 8 * 64 * 16;              // one plane of a feature pair: 8 k-groups x 64 slots x 16 bytes
constexpr int AXB_PAIR_BYTES = 2 * AXB_PLANE_BYTES;       // one feature pair (64 features) x 64 columns, two fp16 planes
// byte offset of the half that holds feature k of column c (0 .. 63) of column block cb in plane 0 (hi) or 1 (lo)
EOFX_HOST_DEVICE inline int64_t axb_plane_offset(int64_t cb, int64_t K_all, int64_t k, int c, int plane) {
  const int64_t pair = k >> 6;
  const int g = (int)(k >> 3) & 7, t = (int)k & 7;
  const int slot = c ^ ((c >> 3) & 7);
  return (cb * (K_all / AXB_KG) + pair) * AXB_PAIR_BYTES + (int64_t)plane * AXB_PLANE_BYTES + (g * 64 + slot) * 16 + t * 2;
}
inline size_t axb_planes_bytes(int64_t K_all, int L) { return (size_t)((L + 63) / 64) * (size_t)(K_all / AXB_KG) * AXB_PAIR_BYTES; }

// ---- the two streaming products ------------------------------------------------------------------------------------------
struct AtbPlan {
  int S;
  int64_t kps;
};
// split-K factor from a small cost model: 512 resident workgroups, ~10 GB/s of A per
// workgroup slot, partial-sum traffic at ~4 TB/s.
// 128-column tiles (atb_f16_kernel<4>, one workgroup per CU): the wide products (Gram matrices, PCA panels) and the
// two-matrix form of a 128-column complex panel (33-64 complex columns: Re and Im are then streamed ONCE per pass)
// (round 3: also the single-matrix passes of sketches of 65 columns and more -- EOF with 55+ modes: one 128-column launch at
// 4.3 TB/s beats two 64-column launches at 6.5 TB/s: 229.7 -> 205.6 ms per rSVD at k = 100, config-4 size)
inline bool atb_wide(int L) {
  if (const char* ev = std::getenv("EOFX_ATB_WIDE_MIN")) return L >= atoi(ev);   // tuning hook (tools/wide_sketch_probe.py)
  return L >= 96;       // (96 columns: one partial 128-column tile, see atb_tiles)
}
inline AtbPlan atb_plan(int64_t M, int64_t K, int L, bool wide = false) {
  const int bx = (int)(M / ATB_BM);
  const int bz = wide ? (L + 127) / 128 : (L + 63) / 64;
  const double resident = wide ? 256.0 : 512.0;
  AtbPlan best{1, K};
  // tuning / test hook: EOFX_ATB_SPLITS=1 keeps small products in ONE split, where the kernels' own epilogues finish the tile
  // (tests/test_gpu_plane_producers.py runs the plane epilogue of atb_f16_kernel at small shapes that way)
  if (const char* ev = std::getenv("EOFX_ATB_SPLITS"))
    if (atoi(ev) == 1) return best;
  double best_t = 1e30;
  for (int S = 1; S <= 128; ++S) {
    const int64_t kps = round_up((K + S - 1) / S, ATB_KG);
    const int s_eff = (int)((K + kps - 1) / kps);
    if (s_eff != S) continue;
    const double blocks = (double)bx * bz * s_eff;
    const double rounds = std::ceil(blocks / resident);
    double t = rounds * (double)kps * 2048.0 / 1.0e10;
    if (s_eff > 1) t += (2.0 * s_eff + 1.0) * (double)M * L * 4.0 / 4.0e12;
    if (t < best_t * 0.98) {
      best_t = t;
      best = {s_eff, kps};
    }
  }
  return best;
}
// axb_f16_kernel (the in-place sample-side product): rows_pad / 256 row tiles x S feature splits.  S = 1 when the row
// tiles alone fill the chip, otherwise a multiple of 8 (one split per XCD at a time) from the same kind of cost model.
inline AtbPlan axb_plan(int64_t rows_pad, int64_t K) {
  const int64_t rt = rows_pad / AXB_BM;
  const int64_t units = K / AXB_KG;
  if (rt >= 1024 || units < 16) return {1, K};
  if (const char* ev = std::getenv("EOFX_AXB_SPLITS")) {   // tuning hook (tools/atb_probe.py)
    const int want = std::max(8, atoi(ev) / 8 * 8);
    const int64_t kps = round_up((units + want - 1) / want, 1) * AXB_KG;
    return {(int)((K + kps - 1) / kps), kps};
  }
  AtbPlan best{1, K};
  double best_t = 1e30;
  for (int s8 = 1; s8 <= 32 && 8 * s8 <= units; ++s8) {
    const int S = 8 * s8;
    const int64_t kps = (units + S - 1) / S * AXB_KG;
    const int s_eff = (int)((K + kps - 1) / kps);
    if (s_eff > S || s_eff <= S - 8) continue;
    const double rounds = std::ceil((double)rt * s8 / 64.0);          // 64 resident workgroups per XCD
    double t = rounds * (double)kps * 1024.0 / 1.25e10;               // 256 rows x 4 B per feature, ~12.5 GB/s per slot
    t += (2.0 * s_eff + 1.0) * (double)rows_pad * 64.0 * 4.0 / 4.0e12;
    if (t < best_t * 0.98) {
      best_t = t;
      best = {s_eff, kps};
    }
  }
  return best;
}
inline size_t atb_scratch_bytes(int64_t M, int64_t K, int L) {
  const AtbPlan pl = atb_plan(M, K, L), plw = atb_plan(M, K, L, true);
  const int smax = std::max(pl.S, atb_wide(L) ? plw.S : 1);
  size_t b = smax > 1 ? (size_t)smax * M * L * (sizeof(float) + sizeof(double)) + 4096 : 4096;   // f32 or f64 partials
  const AtbPlan px = axb_plan(M, round_up(K, AXB_KG));      // in case M is the sample side of an in-place matrix
  if (px.S > 1) b = std::max(b, (size_t)px.S * M * round_up(L, 64) * sizeof(float) + 4096);
  return b;
}

// Column tiles of a panel of L columns (a multiple of 32), in launch order: `count` adjacent tiles of `width` columns from
// column `col_base` on are ONE launch (every launch reads the field once).
// wide (the split-fp16 atb kernel from atb_wide on): full 128-column tiles, then -- when 96 columns are left (panels of
// 96 / 224 columns) -- ONE partial wide tile (width 96) instead of a 64- and a 32-column launch, then the 64 / 32-column rests;
// otherwise (other precisions, the in-place X Y of launch_axb): 64-column tiles and one of 32.
struct ColTile {
  int width, col_base, count;
};
struct ColTiles {
  int n = 0;
  ColTile t[4];
  int columns() const {      // tiles in all: every one of them reads the field once
    int c = 0;
    for (int i = 0; i < n; ++i) c += t[i].count;
    return c;
  }
};
inline ColTiles atb_tiles(int L, bool wide) {
  ColTiles out;
  const int n4 = wide ? L / 128 : 0;
  const int part4 = (wide && L - 128 * n4 == 96) ? 96 : 0;
  const int cb4 = 128 * n4 + part4;
  const int nfull = (L - cb4) / 64, rem = (L - cb4) % 64;
  if (n4 > 0) out.t[out.n++] = {128, 0, n4};
  if (part4) out.t[out.n++] = {96, 128 * n4, 1};
  if (nfull > 0) out.t[out.n++] = {64, cb4, nfull};
  if (rem) out.t[out.n++] = {32, cb4 + nfull * 64, 1};
  return out;
}

// ---- further rules -------------------------------------------------------------------------------------------------------
// number of row-strided partial Gram matrices: >= 4 slabs of 32 rows per workgroup for the narrow
// (sketch-width) panels; wide panels already expose (L/64)^2 sub-blocks, so fewer partials (<= 64 MB)
inline int gram_parts(int64_t rows, int L) {
  // workgroups along the rows; every workgroup writes one partial (L x L float64):
  // >= 8 k-steps (32 rows) per wave, <= 128 MB of partials (a 130 000 x 1536 panel, 300 sub-blocks: 3 row parts 8.9 ms,
  // 6 .. 24 parts 7.1 ms -- tools/wide_small_probe.py)
  // (one workgroup per CU: the products run at the fp64 MFMA rate either way -- ~45 TFLOP/s here -- and every further
  // partial is 8 L^2 bytes written and read again: 194 / 210 / 243 us for 256 / 512 / 1024 partials of a 1M x 64 panel)
  const int64_t by_rows = std::min<int64_t>((rows + 127) / 128, 256);
  const int64_t by_mem = ((int64_t)128 << 20) / ((int64_t)L * L * 8);
  if (const char* ev = std::getenv("EOFX_GRAM_PARTS")) return std::max(1, atoi(ev));   // tuning hook (tools/small_kernel_probe.py)
  return (int)std::max<int64_t>(1, std::min(by_rows, std::max<int64_t>(by_mem, 1)));
}

inline int rsvd_auto_iters(int k, int64_t n, int64_t p) {
  // sklearn extmath._randomized_svd: n_iter = 7 if n_components < 0.1 * min(M.shape) else 4
  return ((double)k < 0.1 * (double)std::min(n, p)) ? 7 : 4;
}

constexpr size_t EOFX_ORTH_TALL_BYTES = (size_t)16 << 20;
// Is the tall panel re-normalised between the two products of a power iteration?  scikit-learn normalises after EVERY
// product; leaving that step out is exact in exact arithmetic, but one iteration then squares sigma_1 / sigma_l inside
// the float32 panel and the Cholesky-QR that follows squares it again: modes more than ~500x below the leading one
// drift from the float64 reference (6e-5 at 1370x, lost beyond 4000x; with the step 8e-6 at 41000x, tests
// test_peaked_spectrum_*).  The step costs 0.85 ms per iteration at config 4 (4 % of a fit), so:
//   * always: small tall panels (<= 16 MiB: microseconds), the float64 mode, and the FIRST iteration of every fit;
//   * afterwards only where it matters: after the first iteration the small-side Gram matrix W^T W is a Rayleigh
//     quotient of X X^T on an orthonormal basis; if the square root of the ratio of its extreme eigenvalues
//     (~ sigma_1 / sigma_l) exceeds hostla::PEAKED_RATIO the remaining iterations keep the step.
// ONE rule (eofx_orth_tall_rule / eofx_peaked_spectrum) for the C++ drivers and the panel-level (sharded) driver.
inline bool orth_tall_rule(int64_t tall_pad, int L, int prec_power) {
  if (std::getenv("EOFX_FORCE_ORTH_TALL")) return true;    // experiments (tools/cond_study.py)
  return prec_power == EOFX_PREC_F64 || (size_t)tall_pad * L * sizeof(float) <= EOFX_ORTH_TALL_BYTES;
}

// ---- the real decompositions (eofx_rsvd_f32, eofx_fit_f32, eofx_fit_sharded_f32, the cross-covariance entries) -----------------
// fix_null_columns on a factor of rows_pad x Lo: the panel's copy, the partial Gram matrices and four Lo x Lo matrices
inline size_t null_repair_bytes(int64_t rows_pad, int Lo) {
  return (size_t)rows_pad * Lo * 4 + (size_t)(gram_parts(rows_pad, Lo) + 4) * Lo * Lo * 8 + (64 << 10);
}
// the blocked device Cholesky inverse of a sketch wider than one wavefront: 2 Lb^2 + Lb^2 / 2 + 64^2 + Lb doubles
inline size_t rinv_blocked_bytes(int l) {
  const size_t Lb = (size_t)round_up(l, 64);
  return (2 * Lb * Lb + Lb * Lb / 2 + 64 * 64 + Lb) * sizeof(double) + 8192;
}
// everything rsvd_core carves for a tall_pad x small_pad operator, a sketch of l columns and k modes
inline size_t rsvd_scratch_bytes(int64_t tall_pad, int64_t small_pad, int l, int k) {
  const size_t L = (size_t)round_up(l, 32), Lo = (size_t)round_up(k, 32);
  size_t b = 0;
  b += 2 * small_pad * L * 4 + 2 * tall_pad * L * 4 + tall_pad * Lo * 4 + small_pad * Lo * 4;
  b += atb_scratch_bytes(small_pad, tall_pad, (int)L);        // split-K partials (small side)
  b += atb_scratch_bytes(tall_pad, small_pad, (int)L);        // split-K partials (tall side)
  b += atb_scratch_bytes(small_pad, tall_pad, (int)Lo);
  b += (size_t)(4 * gram_parts(std::max(tall_pad, small_pad), (int)L) + 8) * L * L * 8 + 2 * L * Lo * 8 + 4096;  // gram partials, Rinv, G0, R2, M1, M2
  b += (size_t)std::max(tall_pad, small_pad) * (Lo + L) * 4;  // export / import staging
  if (l > 64) b += rinv_blocked_bytes(l);                     // blocked device Cholesky of a wide sketch
  b += 4 << 20;
  return b;
}

enum { RSVD_PLAN_OK = 0, RSVD_PLAN_RANK, RSVD_PLAN_WIDTH };
// The sketch rules of a rows x cols matrix (the counts the rank and the orientation are decided on: valid features of a masked
// matrix, features over all ranks of a sharded one -- eofx_fit_sharded_f32 passes (n, P_total) with n < P_total, so r = n).
// n_iter < 0: scikit-learn's count.  status: the first check that failed, in the order the entries report them; every field is
// set either way (the fit entries do not look at the status: the two-step path reports it once the field is compacted).
struct RsvdPlan {
  int status;
  int64_t r;                  // rank bound min(rows, cols)
  int l_req, l;               // sketch width asked for (k + n_oversamples), used (<= r)
  int L, Lo;                  // columns of the sketch panels / of the output panels (multiples of 32)
  int n_iter;                 // resolved
  bool transposed;            // rows < cols: the operator is the transpose (scikit-learn: n_samples < n_features)
  bool full_width;            // l == r: the sketch spans everything, the identity replaces the Gaussian draw
};
inline RsvdPlan rsvd_plan(int64_t rows, int64_t cols, int k, int n_oversamples, int n_iter) {
  RsvdPlan pl{};
  pl.r = std::min(rows, cols);
  pl.l_req = k + n_oversamples;
  pl.l = (int)std::min<int64_t>(pl.l_req, pl.r);
  pl.status = k > pl.r ? RSVD_PLAN_RANK : pl.l > EOFX_MAX_SKETCH ? RSVD_PLAN_WIDTH : RSVD_PLAN_OK;
  pl.L = (int)round_up(pl.l, 32);
  pl.Lo = (int)round_up(k, 32);
  pl.n_iter = n_iter < 0 ? rsvd_auto_iters(k, rows, cols) : n_iter;
  pl.transposed = rows < cols;
  pl.full_width = pl.l == pl.r;
  return pl;
}

// The cross-covariance driver: C = X^T Y of two n-sample matrices of p1 / p2 columns (physical widths; P1 / P2 are the counts the
// rules see).  fast1 / fast2: gram_fast_ok of either matrix; fast_scratch1 / 2: gram_fast_scratch (0 where the route is refused).
// gram_route is THIS rank's wish (the ranks of a sharded fit vote on it); the sharded arena holds either route and the null-mode
// repair of a sharded factor, the local one the route taken.  arena_bytes is 0 unless status is RSVD_PLAN_OK.
struct CrossPlan : RsvdPlan {
  int64_t tall, small, tall_pad, small_pad;      // the operator A = C (p1 x p2), or C^T when transposed
  bool gram_route;
  size_t arena_bytes;
};
inline CrossPlan cross_plan(int64_t n, int64_t n_pad, int64_t p1, int64_t p1_pad, int64_t p2, int64_t p2_pad, int64_t P1, int64_t P2,
                            bool sharded, bool want_tsc, bool fast1, bool fast2, size_t fast_scratch1, size_t fast_scratch2, int k,
                            int n_oversamples, int n_iter, bool no_gram) {
  CrossPlan pl{};
  static_cast<RsvdPlan&>(pl) = rsvd_plan(P1, P2, k, n_oversamples, n_iter);
  pl.tall = pl.transposed ? p2 : p1;
  pl.small = pl.transposed ? p1 : p2;
  pl.tall_pad = pl.transposed ? p2_pad : p1_pad;
  pl.small_pad = pl.transposed ? p1_pad : p2_pad;
  pl.gram_route = want_tsc && n < P1 && n < P2 && fast1 && fast2 && !no_gram;
  if (pl.status != RSVD_PLAN_OK) return pl;
  const int64_t pp = std::max(p1_pad, p2_pad);
  const size_t panels = (size_t)n_pad * pl.L * 4 * 2;
  size_t need = rsvd_scratch_bytes(pp, pp, pl.l, k) + panels + atb_scratch_bytes(n_pad, pp, pl.L);
  if (want_tsc) need += (size_t)n_pad * n_pad * 4 * 2 + (1 << 20);      // the two sample-space Gram matrices
  const size_t need_gram = fast1 && fast2 ? std::max(fast_scratch1, fast_scratch2) + panels + atb_scratch_bytes(n_pad, n_pad, pl.L) : 0;
  const size_t need_plain = want_tsc ? atb_scratch_bytes(n_pad, pp, (int)n_pad) : 0;
  if (sharded)
    need += null_repair_bytes(pp, pl.Lo) + std::max(need_gram, need_plain);
  else
    need += pl.gram_route ? need_gram : need_plain;
  pl.arena_bytes = need;
  return pl;
}

// ---- the complex decomposition (eofx_rsvd_c64 and its Hilbert / sharded forms) ----------------------------------------------
// Scratch of one pass of the complex operator on a panel of L real columns, either direction: the split-K partials of the two
// streaming products, twice each (the two parts of a two-launch pass).
inline size_t c64_pass_scratch_bytes(int64_t n, int64_t p, int64_t n_pad, int64_t p_pad, int L) {
  return 2 * atb_scratch_bytes(p_pad, round_up(n, ATB_KG), L) + 2 * atb_scratch_bytes(n_pad, round_up(p, ATB_KG), L);
}
// eofx_cmat_mul_f32: the companion panel and the second product [big x L], the two partial results of a two-matrix launch that
// needs no split, and the pass itself
inline size_t c64_mul_scratch_bytes(int64_t n, int64_t p, int64_t n_pad, int64_t p_pad, int L) {
  const int64_t big = std::max(n_pad, p_pad);
  return (size_t)2 * big * L * 4 + (8 << 20) + (size_t)2 * big * L * 4 + c64_pass_scratch_bytes(n, p, n_pad, p_pad, L);
}

constexpr int KRYLOV_MAX_ORDER = 384;   // the host solves the Rayleigh-Ritz problem (~10 ms at order 240): blocks beyond are thick-restarted
constexpr int C64_IT_MIN = 2;           // "converge": products before the first stop
constexpr int C64_IT_CAP = 20;          // "converge": products at most (lobpcg's own limit under svds)
enum { C64_PLAN_OK = 0, C64_PLAN_SHARD_SIDE, C64_PLAN_RANK, C64_PLAN_WIDTH, C64_PLAN_MASKED, C64_PLAN_N_ITER };
// Sizes and routes of the complex driver for an n x p field (this rank's slice of p_total features when p_total > 0; masked:
// p_valid of the p columns hold data).  n_iter: a count, -1 scikit-learn's (auto_count), -2 "converge".  status: the first check
// that failed, in the order the driver reports them; nothing else is set then (but r, for the message of C64_PLAN_RANK, and l).
struct C64Plan {
  int status;
  int64_t r;                  // rank bound min(n, valid features over all ranks)
  int l;                      // sketch width (complex columns)
  bool adaptive;              // "converge"
  int n_iter, auto_count;     // products (resolved), scikit-learn's count
  int h, LP;                  // complex columns of a panel (32 | 64), real columns [Re(h) | Im(h)]
  int ko, Lo;                 // the same for the output panels [Re(ko) | Im(ko)]
  bool transposed;            // A_op = Z^H: the tall side is the features
  int64_t small, small_pad, tall_pad, big;
  bool krylov;                // block Krylov (else subspace iteration)
  int nbmax;                  // blocks kept before a thick restart
  int64_t ldk;                // row stride of the side-by-side blocks
  size_t arena_bytes;
};
inline C64Plan c64_plan(int64_t n, int64_t p, int64_t n_pad, int64_t p_pad, int64_t p_total, bool masked, int64_t p_valid, int k,
                        int n_oversamples, int n_iter, bool krylov_allowed) {
  C64Plan pl{};
  auto fail = [&](int status) { return pl.status = status, pl; };
  const bool shd = p_total > 0;
  if (shd && !(n < p_total)) return fail(C64_PLAN_SHARD_SIDE);
  pl.r = std::min(n, shd ? p_total : (masked ? p_valid : p));
  if (k > pl.r) return fail(C64_PLAN_RANK);
  pl.l = (int)std::min<int64_t>(k + n_oversamples, pl.r);
  if (pl.l > 64) return fail(C64_PLAN_WIDTH);
  if (!shd && masked && !(n < p_valid)) return fail(C64_PLAN_MASKED);
  pl.adaptive = n_iter == -2;
  pl.auto_count = k < 0.1 * (double)pl.r ? 7 : 4;
  if (n_iter == -1) n_iter = pl.auto_count;
  if (pl.adaptive) n_iter = C64_IT_CAP;
  if (n_iter < 0) return fail(C64_PLAN_N_ITER);
  pl.n_iter = n_iter;
  const int l = pl.l;
  pl.h = l <= 32 ? 32 : 64;
  pl.LP = 2 * pl.h;
  pl.ko = (int)round_up(k, 16);
  pl.Lo = 2 * pl.ko;
  pl.transposed = shd || n < p;
  pl.small = pl.transposed ? n : p;
  pl.small_pad = pl.transposed ? n_pad : p_pad;
  pl.tall_pad = pl.transposed ? p_pad : n_pad;
  pl.big = std::max(n_pad, p_pad);
  const int nb_fit = KRYLOV_MAX_ORDER / l;
  pl.krylov = n_iter >= 1 && nb_fit >= 3 && krylov_allowed;
  pl.nbmax = pl.krylov ? std::min(n_iter + 1, nb_fit) : 0;
  pl.ldk = (int64_t)pl.nbmax * pl.LP;
  const int LP = pl.LP, Lo = pl.Lo, nbmax = pl.nbmax;
  const int64_t small_pad = pl.small_pad, tall_pad = pl.tall_pad, big = pl.big;
  size_t need = (size_t)(2 * small_pad + 2 * tall_pad + 2 * big) * LP * 4 + (size_t)(small_pad + tall_pad) * Lo * 4;
  need += c64_pass_scratch_bytes(n, p, n_pad, p_pad, LP);
  need += (size_t)(4 * gram_parts(big, LP) + 8) * LP * LP * 8 + (size_t)big * (Lo + LP) * 4 + (8 << 20);
  if (pl.krylov)
    need += (size_t)nbmax * (2 * small_pad + tall_pad) * LP * 4 + (size_t)small_pad * LP * 4 + (size_t)(3 + nbmax) * nbmax * LP * LP * 8 +
            ((size_t)48 << 20);
  pl.arena_bytes = need;
  return pl;
}

// the lag operator: lags per group (see EOFX_LAG_GROUP_COLS), the lags of the last group, workgroups of its streaming kernels
inline int lag_groupsize(int E, int L) { return std::max(1, std::min(E, EOFX_LAG_GROUP_COLS / std::max(L, 1))); }
inline int lag_last_group(int E, int G) { return E - (E - 1) / G * G; }
inline int lag_blocks(int64_t total4) { return (int)std::max<int64_t>(1, std::min<int64_t>((total4 + 255) / 256, 8192)); }

// workgroups of a streaming pass of eofx_spca.hpp over `rows` rows whose partials hold `entries` doubles each: about 128 rows per
// workgroup, at most SPCA_GMAX, the partials within 32 MiB (a function of the shape alone: results never depend on the device)
inline int spca_grid(int64_t rows, int64_t entries) {
  const int64_t g = std::min<int64_t>(SPCA_GMAX, std::max<int64_t>(1, (rows + 127) / 128));
  const int64_t cap = std::max<int64_t>(1, ((int64_t)4 << 20) / std::max<int64_t>(1, entries));
  return (int)std::max<int64_t>(1, std::min(g, cap));
}

// Shape predicates of the routes through the NT kernel of eofx_gram.hpp (`has_source`: the matrix holds a layout the route can
// read; the 2^32 bounds are the 32-bit row offsets of the LDS-DMA loads).
// the fast Gram route of a matrix of n_pad x p (sample side up to 32768)
inline bool gram_fast_ok(int64_t n_pad, int64_t p, bool has_source) {
  return n_pad % GR_BM == 0 && n_pad <= EOFX_GRAM_MAX_SIDE && has_source && round_up(p, 2 * GR_BK) * 4 * GR_BM < ((int64_t)1 << 32) &&
         !std::getenv("EOFX_NO_FAST_GRAM");
}
// wide feature-side products Yp [p_pad x L] = X'^T Zn (L in the hundreds: the PCA pre-reduction's 1500-column panel took 83 ms
// through the 128-column streaming tiles, the field re-read 12 times at a third of the matrix cores' rate; through the NT
// kernel: transposed planes of the field once, planes of Zn^T, one MFMA-bound product)
inline bool tmul_nt_ok(int64_t n, int64_t p_pad, bool has_source, int L) {
  const int64_t kpad = round_up(n, 2 * GR_BK);
  return L >= 512 && p_pad % GR_BM == 0 && has_source && kpad * 4 * GR_BM < ((int64_t)1 << 32) && n >= 512 &&
         !std::getenv("EOFX_NO_TMUL_NT");
}
// out[rows x Lo] = P[rows x L] Mx[L x Lo] for WIDE operands
inline bool matmul_nt_ok(int64_t rows, int L, int Lo) {
  const int64_t kpad = round_up(L, 2 * GR_BK);
  return L >= 512 && Lo >= 256 && Lo % 4 == 0 && L % 4 == 0 && rows >= 1024 && rows % GR_BM == 0 &&
         kpad * 4 * GR_BM < ((int64_t)1 << 32) && !std::getenv("EOFX_NO_MATMUL_NT");
}
// The work list of gram_nt_kernel (eofx_gram.hpp; tests/test_gram_plan_cpu.py holds its invariants).  The kernels read GramItem and GramTile as they stand here (GramTile in place
// of HIP's int2: eofx_gram.hpp asserts size and layout).
// work item: tile (bi, bj), first stage, number of stages (EVEN), output slot (tile-major: slot = tile * S + split)
struct GramItem {
  int bi, bj, st0, nst, slot, pad0, pad1, pad2;
};
struct GramTile {
  int x, y;      // {bi, bj}
};
struct GramPlan {
  int nti = 0, ntj = 0, T = 0, S = 1, st_per_split = 0, grid = 0;
  std::vector<GramItem> items;   // [grid]: workgroup b -> item (XCD b % 8 walks its own patch of tiles split by split)
  std::vector<GramTile> tiles;   // [T]: slot order
};

inline unsigned gram_morton(unsigned i, unsigned j) {
  unsigned m = 0;
  for (int b = 0; b < 12; ++b) m |= ((i >> b) & 1u) << (2 * b + 1) | ((j >> b) & 1u) << (2 * b);
  return m;
}

// sym: only tiles bi <= bj (C = A A^T).  nst_total: stages (32 features each) of the contraction.
// S <= 0: chosen here (rounds of 32 workgroups per XCD x stages per split, ~40 stages of fixed cost per item).
inline void gram_plan_build(int nti, int ntj, bool sym, int nst_total, int S, GramPlan& pl) {
  pl.nti = nti;
  pl.ntj = ntj;
  pl.tiles.clear();
  for (int i = 0; i < nti; ++i)
    for (int j = sym ? i : 0; j < ntj; ++j) pl.tiles.push_back(GramTile{i, j});
  std::sort(pl.tiles.begin(), pl.tiles.end(), [](const GramTile& a, const GramTile& b) {
    return gram_morton((unsigned)a.x, (unsigned)a.y) < gram_morton((unsigned)b.x, (unsigned)b.y);
  });
  const int T = (int)pl.tiles.size();
  pl.T = T;
  int lo[9];
  for (int x = 0; x <= 8; ++x) lo[x] = (int)((int64_t)T * x / 8);
  int cmax = 0;
  for (int x = 0; x < 8; ++x) cmax = std::max(cmax, lo[x + 1] - lo[x]);
  if (S <= 0) {
    double best = 1e300;
    for (int s = 1; s <= 16 && s <= nst_total; ++s) {
      const int sps = ((nst_total + s - 1) / s + 1) / 2 * 2;
      const int s_eff = (nst_total + sps - 1) / sps;
      if (s_eff != s) continue;
      const double rounds = (double)((cmax * s + 31) / 32);
      const double cost = rounds * (sps + 40.0) + 2.0 * s;
      if (cost < best * 0.97) {
        best = cost;
        S = s;
      }
    }
  }
  const int sps = ((nst_total + S - 1) / S + 1) / 2 * 2;     // even (nst_total is: kpad % 64 == 0)
  S = (nst_total + sps - 1) / sps;
  pl.S = S;
  pl.st_per_split = sps;
  const int W = cmax * S;
  pl.grid = 8 * W;
  pl.items.assign((size_t)pl.grid, GramItem{0, 0, 0, 0, 0, 0, 0, 0});
  for (int x = 0; x < 8; ++x) {
    const int cnt = lo[x + 1] - lo[x];
    for (int s = 0; s < S; ++s)
      for (int t = 0; t < cnt; ++t) {
        const int w = s * cnt + t, tile = lo[x] + t;
        const int st0 = s * sps, nst = std::min(sps, nst_total - st0);
        pl.items[(size_t)8 * w + x] = GramItem{pl.tiles[tile].x, pl.tiles[tile].y, st0, nst, tile * S + s, 0, 0, 0};
      }
  }
}

// the statistics-carrying first pass of the fused fit (eofx_fit.hpp): in-place layout, the f16x3 passes, a 16-byte aligned field
inline bool fit_first_eligible(int keep_raw, int prec_power, bool aligned16, int64_t n, int64_t P, int l) {
  return keep_raw == 2 && prec_power == EOFX_PREC_F16X3 && n < P && l > 0 && l < n && round_up(l, 32) <= 64 && l % 32 != 0 &&
         P % 4 == 0 && aligned16 && n < ((int64_t)1 << 31) && !std::getenv("EOFX_NO_FUSED_FIT");
}
// the whole fused fit (eofx_fit_f32, eofx_fit_sharded_f32): the first pass as above, an unclamped sketch of the plan `sk` and a
// host sketch matrix with a row for every sample
inline bool fused_fit_eligible(int keep_raw, int prec_power, bool aligned16, int64_t n, int64_t P, int k, const RsvdPlan& sk,
                               int64_t omega_rows, bool omega_on_device) {
  return fit_first_eligible(keep_raw, prec_power, aligned16, n, P, sk.l) && k <= n && sk.l == sk.l_req && omega_rows >= n &&
         !omega_on_device;
}

// ---- preprocessing statistics ----------------------------------------------------------------------------------------------
// The column statistics of an n x P field (row stride ld): four features per thread and 16-byte loads where the field allows
// (vec4), RS row splits of rps rows so that about 2048 workgroups run.  sample_raw: the Hilbert stage follows on an in-place
// matrix (the sample-raw request of the context) and its one-kernel route takes this length two features at a time: the pass then also writes
// the raw field in the sample-contiguous layout (tr, colstats_tr_kernel, which moves 64 x 64 tiles) instead of a separate
// transposing copy behind the statistics pass.
struct ColstatsPlan {
  bool vec4, tr;
  int gxs, gx;         // workgroups along the features: one thread per feature (shift, finalize) / of the statistics kernel
  int64_t RS, rps;
};
inline ColstatsPlan colstats_plan(int64_t n, int64_t P, int64_t ld, bool aligned16, bool sample_raw, bool row_map) {
  ColstatsPlan pl;
  pl.vec4 = P % 4 == 0 && ld % 4 == 0 && aligned16;
  pl.gxs = (int)((P + 255) / 256);
  pl.gx = pl.vec4 ? (int)((P / 4 + 255) / 256) : pl.gxs;
  int64_t RS = std::max<int64_t>(1, (2048 + pl.gx - 1) / pl.gx);
  RS = std::min<int64_t>(RS, std::max<int64_t>(1, n / 64));
  pl.rps = (n + RS - 1) / RS;
  if (sample_raw && !row_map) pl.rps = round_up(pl.rps, 64);
  pl.RS = (n + pl.rps - 1) / pl.rps;
  pl.tr = pl.vec4 && !row_map && sample_raw && round_up(n, ATB_BM) <= 8192 && pl.rps % 64 == 0;
  return pl;
}
inline size_t colstats_scratch(int64_t n, int64_t P) {
  const int64_t gx = std::max<int64_t>(1, (P / 4 + 255) / 256);   // the four-features-per-thread kernel: fewer workgroups, more row splits
  int64_t RS = std::max<int64_t>(1, (2048 + gx - 1) / gx);      // (fewer than four features: gx was 0 -- a division by zero, round 5)
  RS = std::min<int64_t>(RS, std::max<int64_t>(1, n / 64));
  return (size_t)(RS + 1) * P * 32 + (size_t)P * 72 + (size_t)n * 16 + (1 << 20);
}
// workgroups of feature_summary_kernel
inline int summary_blocks(int64_t P) { return (int)std::max<int64_t>(1, std::min<int64_t>((P + 4095) / 4096, 256)); }

// apply_kernel<true> (16-byte loads): no column map, a row stride of whole float4, an aligned source
inline bool apply_vec(bool col_map, int64_t ld_src, bool aligned16) { return !col_map && ld_src % 4 == 0 && aligned16; }

// The layout a preprocessed matrix ends in (pv of P features and ns of n samples hold data; keep_raw / allow_masked: the layout
// asked for through the context's layout mode; stats_absmax: the column statistics of THIS field are at hand).
// raw mode: nothing is dropped or reordered, so the raw field itself -- read through the affine map -- is the feature-contiguous
// layout; only the sample-contiguous one is written (not even that in place).  P < 2^31 rows: int.
// masked in place (layout mode 3): all-NaN grid points (sanitizer.py:80-126 would drop them) stay in the matrix as zero
// columns -- scale 0 in the map, bits ANDed to +0 by the MASK kernels -- when they are a minority and the sketch lives
// on the sample side; a zero column changes no product, Gram matrix or norm, so the factors are those of the compacted
// matrix with zero rows in V at the masked features (the caller drops them).  1x the field in HBM instead of 3x.
struct ApplyPlan {
  bool raw, masked, in_place;
  bool col_map, vec;          // the written layouts: features are compacted through a column map / apply_kernel<true>
};
inline ApplyPlan apply_plan(int64_t n, int64_t P, int64_t pv, int64_t ns, int keep_raw, bool allow_masked, bool stats_absmax,
                            bool aligned16) {
  ApplyPlan pl;
  const bool raw_ok = keep_raw && ns == n && P % 4 == 0 && aligned16 && n < ((int64_t)1 << 31);
  pl.masked = raw_ok && keep_raw == 2 && allow_masked && stats_absmax && pv < P && 10 * pv >= 6 * P && n < pv;
  pl.raw = (raw_ok && pv == P) || pl.masked;
  pl.in_place = pl.raw && keep_raw == 2;
  pl.col_map = pv < P && !pl.masked;
  pl.vec = !pl.in_place && apply_vec(pl.col_map, P, aligned16);
  return pl;
}

// ---- block cross-covariance of multi-view CCA (eofx_viewcov.hpp) ---------------------------------------------------------
// off[0 .. m]: the first column of every view.  host = the view of every column, then (bi, bj) of every 128-tile on or above the
// diagonal that holds a wanted output (keep_diag, or two different views); the samples are cut into G splits of `chunk` slabs:
// a function of (n, the tile list) alone, no split empty.
struct ViewcovPlan {
  std::vector<int> host;      // [p] views, [2 ntiles] tiles
  int ntiles = 0;
  int64_t nslabs = 0, G = 1, chunk = 0;
};
enum { VIEWCOV_OFF_OK = 0, VIEWCOV_OFF_ENDS = 1, VIEWCOV_OFF_ORDER = 2 };
// -> VIEWCOV_OFF_OK, or what is wrong with off (*bad_view: the view v with off[v + 1] <= off[v])
inline int viewcov_plan(int64_t n, int p, const int* off, int m, bool keep_diag, ViewcovPlan& pl, int* bad_view = nullptr) {
  if (off[0] != 0 || off[m] != p) return VIEWCOV_OFF_ENDS;
  for (int v = 0; v < m; ++v)
    if (off[v + 1] <= off[v]) {
      if (bad_view) *bad_view = v;
      return VIEWCOV_OFF_ORDER;
    }
  std::vector<int>& host = pl.host;
  host.assign((size_t)p, 0);
  for (int v = 0; v < m; ++v) std::fill(host.begin() + off[v], host.begin() + off[v + 1], v);
  const int nb = (p + VIEWCOV_T - 1) / VIEWCOV_T;
  auto one_view = [&](int b) { return host[(size_t)b * VIEWCOV_T] == host[(size_t)std::min(p, (b + 1) * VIEWCOV_T) - 1]; };
  pl.ntiles = 0;
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = bi; bj < nb; ++bj) {
      if (!keep_diag && one_view(bi) && one_view(bj) && host[(size_t)bi * VIEWCOV_T] == host[(size_t)bj * VIEWCOV_T]) continue;
      host.push_back(bi);
      host.push_back(bj);
      ++pl.ntiles;
    }
  pl.nslabs = (n + VIEWCOV_K - 1) / VIEWCOV_K;
  int64_t G = pl.ntiles ? std::min<int64_t>(VIEWCOV_WGS / pl.ntiles, pl.nslabs / VIEWCOV_SPLIT_SLABS) : 1;
  G = std::max<int64_t>(G, 1);
  pl.chunk = (pl.nslabs + G - 1) / G;
  pl.G = (pl.nslabs + pl.chunk - 1) / pl.chunk;                // (no empty split)
  return VIEWCOV_OFF_OK;
}

// ---- filter covariances (eofx_lagcov.hpp, eofx_lowpass.hpp) ----------------------------------------------------------------
// ny tile pairs of 64 columns x G splits of the row tiles (a function of the shape alone), and the weights as the kernels'
// sliding windows read them: zero-padded by FIR_PADW on either side.
struct FilterPlan {
  int ny, G;
  std::vector<double> w;
};
// ny workgroup columns, at most gmax splits of the row tiles, and wpad[15 + i] = tap(i), i < taps
template <class Tap>
inline FilterPlan filter_plan(int64_t n, int ny, int64_t gmax, int taps, Tap tap) {
  FilterPlan pl{ny, (int)std::min<int64_t>((n + FIR_R - 1) / FIR_R, std::max<int64_t>(1, gmax)),
                std::vector<double>((size_t)taps + 2 * FIR_PADW, 0.0)};
  for (int i = 0; i < taps; ++i) pl.w[(size_t)(FIR_PADW + i)] = tap(i);
  return pl;
}
// w[0 .. ntau): wpad[15 + tau] = w[tau]
inline FilterPlan lagcov_plan(int64_t n, int p, const double* w, int ntau) {
  const int nb = (p + 63) / 64, ny = nb * ((nb + 3) / 4);
  return filter_plan(n, ny, LAGCOV_WGS / ny, ntau, [&](int i) { return w[i]; });
}
// w[0 .. h]: the symmetric wsym[15 + h + k] = w[|k|], k = -h .. h
inline FilterPlan lowpass_plan(int64_t n, int p, const double* w, int h) {
  const int nb = (p + 63) / 64, ny = nb * (nb + 1) / 2;
  return filter_plan(n, ny, std::min<int64_t>(LOWPASS_WGS / ny, LOWPASS_PART_MAX / ((int64_t)p * p)), 2 * h + 1,
                     [&](int i) { return w[i < h ? h - i : i - h]; });
}

}  // namespace eofx
