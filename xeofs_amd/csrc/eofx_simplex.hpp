// eofx_simplex.hpp -- the two operators of archetypal analysis (Cutler & Breiman 1994; Morup & Hansen 2012;
// single/archetypal.py): the Euclidean projection of many rows onto the probability simplex, and a register-resident
// projected-gradient solver for n independent k-variable simplex-constrained least-squares problems.
//
//   the projection    of a row u of m float32 onto D_m = {x >= 0, sum x = 1}:  out_j = max(u_j - tau, 0), tau the unique
//                     solution of sum_j max(u_j - tau, 0) = 1.  Michelot's fixed point, made monotone so that it ends:
//                         S_0 = all j,  tau_t = (sum_{j in S_t} u_j - 1) / |S_t|   (float64, a fixed summation order),
//                         thr_t = max(thr_{t-1}, tau_t),  S_{t+1} = {j : u_j > thr_t}   (the comparison in float64),
//                     until |S_{t+1}| = |S_t|.  The sets are nested, so equal counts are equal sets and there are at most m
//                     rounds (12 on every row tried, up to m = 16384).  tau is the last tau_t: evaluated over its own
//                     active set.  out_j = (float)((double)u_j - tau) for j in S, 0 elsewhere: rounded once.
//   the edges         a row that holds a NaN or an infinity comes back all NaN.  Where float64 cannot tell tau from the
//                     largest entry (S comes out empty: entries beyond 2^52, or m = 1 with |u| >= 2^53) the limit is
//                     returned: 1 / c at the c largest (equal) entries, 0 elsewhere.  m = 1 gives 1.
//   simplex_rows      u_ij = fmaf(-step, G_ij, V_ij) (u = V without G), out_i = the projection of u_i.
//       tier 0        m <= 1024 (SIMPLEX_REG_MMAX): a row lives in the registers of `lanes` lanes of one wave, `epl` entries
//                     each (entry j on lane j % lanes: a wave's loads are contiguous); m <= 64: lanes = the next power of
//                     two of m, epl = 1, and a wave holds 64 / lanes rows; above: lanes = 64, epl = 2, 4, 8 or 16.  Sums
//                     and counts: the lane's own entries ascending, then an xor butterfly over the lanes (every lane ends
//                     with the same bits).  256 threads: 256 / lanes rows per workgroup.
//       tier 1        1024 < m <= 16384 (SIMPLEX_MMAX): one workgroup per row, 256 threads up to m = 4096 and 1024 above,
//                     the row resident in LDS (4 m bytes: 64 KiB at m = 16384), read once from memory and written once.
//                     Thread t owns the entries t, t + threads, ...: it reads back only what it wrote (no barrier between
//                     the load and the rounds; consecutive lanes on consecutive banks).  Sums and counts: the thread's own
//                     entries ascending, the butterfly over the wave, the waves ascending through LDS.
//   simplex_pg        for every row i independently, `iters` times:
//                         acc_j = the float32 fmaf chain sum_l a_l M_lj, l ascending from 0 (M rounded once to float32),
//                         g_j = acc_j - q_ij,  u_j = fmaf(-inv_L, g_j, a_j),  a <- the projection of u  (sums j ascending).
//                     One thread per row: a, q and u in registers (3 KP of them, KP = the next power of two of k), M in
//                     LDS (every lane reads the same word: a broadcast), one launch for all the iterations.  64 threads per
//                     workgroup: n = 16384 rows are 256 workgroups, one per CU.
// No atomics; every order is a function of the shape alone: two runs are equal bit for bit.  Rows are independent: nothing
// but the row itself decides its result.  Nothing past column m (k) of a row is read or written; `out` may alias the input
// (a thread reads its entries before it writes them, and no other thread touches them).  gfx950 only.
//
// The constants and the plan are plain C++: a host compiler that does not define __HIPCC__ sees them and not the kernels
// (tests/simplex_shim.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "eofx.h"
#endif

namespace eofx {

constexpr int SIMPLEX_MMAX = 16384;         // entries of a row: 64 KiB of the 160 KiB of LDS of a CU
constexpr int SIMPLEX_KMAX = 32;            // variables of a projected-gradient problem: 96 registers of a thread
constexpr int SIMPLEX_REG_MMAX = 1024;      // the longest row of tier 0: 16 entries on each of 64 lanes
constexpr int SIMPLEX_WG = 256;             // threads of a tier 0 workgroup
constexpr int SIMPLEX_PG_WG = 64;           // threads (rows) of a simplex_pg workgroup

// launch shape of simplex_rows for r rows of m entries (1 <= m <= SIMPLEX_MMAX)
struct SimplexPlan {
  int tier;         // 0: registers of a share of a wave, 1: one workgroup per row, the row in LDS
  int lanes;        // tier 0: lanes per row, a power of two <= 64; tier 1: threads
  int epl;          // tier 0: entries per lane (1, 2, 4, 8, 16); tier 1: ceil(m / threads)
  int threads;      // workgroup size
  int rpb;          // rows per workgroup
  int64_t grid;     // workgroups
  size_t lds;       // dynamic LDS in bytes
};
inline SimplexPlan simplex_plan(int64_t r, int64_t m) {
  SimplexPlan pl;
  if (m <= SIMPLEX_REG_MMAX) {
    pl.tier = 0;
    int lanes = 1;
    while (lanes < m && lanes < 64) lanes <<= 1;
    int epl = 1;
    while ((int64_t)lanes * epl < m) epl <<= 1;
    pl.lanes = lanes, pl.epl = epl;
    pl.threads = SIMPLEX_WG;
    pl.rpb = SIMPLEX_WG / lanes;
    pl.lds = 0;
  } else {
    pl.tier = 1;
    pl.threads = m <= 4096 ? 256 : 1024;
    pl.lanes = pl.threads;
    pl.epl = (int)((m + pl.threads - 1) / pl.threads);
    pl.rpb = 1;
    pl.lds = (size_t)m * sizeof(float);
  }
  pl.grid = (r + pl.rpb - 1) / pl.rpb;
  return pl;
}
// KP of simplex_pg: the next power of two of k (1 <= k <= SIMPLEX_KMAX)
inline int simplex_pg_width(int k) {
  int kp = 1;
  while (kp < k) kp <<= 1;
  return kp;
}

#if defined(__HIPCC__)

__device__ __forceinline__ bool simplex_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the sum over the `lanes` lanes (a power of two <= 64) of the aligned group this lane is in: every lane gets the same bits
template <class T>
__device__ __forceinline__ T simplex_grp_sum(T v, int lanes) {
  for (int s = lanes >> 1; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ float simplex_grp_max(float v, int lanes) {
  for (int s = lanes >> 1; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}

// what a row's rounds leave behind: how an entry u becomes its output
struct SimplexRule {
  double tau, thr;
  float umax;
  int nmax;           // entries equal to umax
  bool bad, limit;    // a NaN or an infinity in the row; S came out empty
  __device__ __forceinline__ float operator()(float u) const {
    if (bad) return __uint_as_float(0x7fc00000u);
    if (limit) return u == umax ? (float)(1.0 / (double)nmax) : 0.f;
    return (double)u > thr ? (float)((double)u - tau) : 0.f;
  }
};

// ---- tier 0: grid ceil(r / (256 / lanes)), block 256.  E = entries per lane.
template <int E>
__global__ __launch_bounds__(SIMPLEX_WG) void simplex_rows_reg_kernel(const float* V, int64_t r, int m, int64_t ldv, const float* G,
                                                                      int64_t ldg, float step, float* out, int64_t ldo, int lanes) {
  const int sub = (int)threadIdx.x / lanes, ll = (int)threadIdx.x - sub * lanes;
  const int64_t row = (int64_t)blockIdx.x * (SIMPLEX_WG / lanes) + sub;
  const bool live = row < r;
  float u[E];
  SimplexRule rule;
  int bad = 0, nmax = 0;
  float umax = -INFINITY;
  double sum = 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = ll + e * lanes;
    u[e] = -INFINITY;                              // (padding: never above a threshold)
    if (live && j < m) {
      const float v = V[row * ldv + j];
      u[e] = G ? fmaf(-step, G[row * ldg + j], v) : v;
      bad |= !simplex_finite(u[e]);
      umax = fmaxf(umax, u[e]);
      sum += (double)u[e];
    }
  }
  bad = simplex_grp_sum(bad, lanes);
  umax = simplex_grp_max(umax, lanes);
  sum = simplex_grp_sum(sum, lanes);
#pragma unroll
  for (int e = 0; e < E; ++e) nmax += u[e] == umax;
  nmax = simplex_grp_sum(nmax, lanes);
  int cnt = m;
  rule.bad = bad != 0, rule.limit = false, rule.umax = umax, rule.nmax = nmax;
  rule.tau = (sum - 1.0) / (double)cnt;
  rule.thr = rule.tau;
  bool done = !live || rule.bad;
  while (__any(!done)) {                           // (wave-uniform: a row that is done repeats its last round, which changes nothing)
    int c = 0;
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if ((double)u[e] > rule.thr) {
        ++c;
        s += (double)u[e];
      }
    c = simplex_grp_sum(c, lanes);
    s = simplex_grp_sum(s, lanes);
    if (!done) {
      if (c == 0) rule.limit = true, done = true;
      else if (c == cnt) done = true;
      else {
        cnt = c;
        rule.tau = (s - 1.0) / (double)c;
        rule.thr = fmax(rule.thr, rule.tau);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = ll + e * lanes;
    if (live && j < m) out[row * ldo + j] = rule(u[e]);
  }
}

// ---- tier 1: grid r, block `threads` (256 or 1024), dynamic LDS 4 m bytes.
__global__ __launch_bounds__(1024) void simplex_rows_lds_kernel(const float* V, int64_t r, int m, int64_t ldv, const float* G, int64_t ldg,
                                                               float step, float* out, int64_t ldo) {
  extern __shared__ float simplex_row[];
  __shared__ double red_s[16];
  __shared__ float red_f[16];
  __shared__ int red_c[16], red_b[16];
  const int tid = (int)threadIdx.x, T = (int)blockDim.x, nw = T >> 6, w = tid >> 6, lane = tid & 63;
  const int64_t row = blockIdx.x;
  if (row >= r) return;                            // (block-uniform)
  const float* v_row = V + row * ldv;
  const float* g_row = G ? G + row * ldg : nullptr;
  int bad = 0, nmax = 0;
  float umax = -INFINITY;
  double sum = 0.0;
  for (int j = tid; j < m; j += T) {
    const float v = v_row[j];
    const float u = g_row ? fmaf(-step, g_row[j], v) : v;
    simplex_row[j] = u;
    bad |= !simplex_finite(u);
    umax = fmaxf(umax, u);
    sum += (double)u;
  }
  // the block's sum of (s, c) and maximum / or of (f, b): the butterfly over the wave, then the waves ascending
  const auto reduce = [&](double& s, int& c, float& f, int& b) {
    s = simplex_grp_sum(s, 64), c = simplex_grp_sum(c, 64), f = simplex_grp_max(f, 64), b = simplex_grp_sum(b, 64);
    __syncthreads();                               // (the arrays of the reduction before are read)
    if (lane == 0) red_s[w] = s, red_c[w] = c, red_f[w] = f, red_b[w] = b;
    __syncthreads();
    s = red_s[0], c = red_c[0], f = red_f[0], b = red_b[0];
    for (int x = 1; x < nw; ++x) s += red_s[x], c += red_c[x], f = fmaxf(f, red_f[x]), b += red_b[x];
  };
  int cnt = 0;
  reduce(sum, cnt, umax, bad);
  cnt = m;
  for (int j = tid; j < m; j += T) nmax += simplex_row[j] == umax;
  {
    double s0 = 0.0;
    float f0 = umax;
    int b0 = 0;
    reduce(s0, nmax, f0, b0);
  }
  SimplexRule rule;
  rule.bad = bad != 0, rule.limit = false, rule.umax = umax, rule.nmax = nmax;
  rule.tau = (sum - 1.0) / (double)cnt;
  rule.thr = rule.tau;
  bool done = rule.bad;                            // (block-uniform, like everything the reductions return)
  while (!done) {
    int c = 0, b0 = 0;
    double s = 0.0;
    float f0 = 0.f;
    for (int j = tid; j < m; j += T) {
      const double x = (double)simplex_row[j];
      if (x > rule.thr) {
        ++c;
        s += x;
      }
    }
    reduce(s, c, f0, b0);
    if (c == 0) rule.limit = true, done = true;
    else if (c == cnt) done = true;
    else {
      cnt = c;
      rule.tau = (s - 1.0) / (double)c;
      rule.thr = fmax(rule.thr, rule.tau);
    }
  }
  float* o_row = out + row * ldo;
  for (int j = tid; j < m; j += T) o_row[j] = rule(simplex_row[j]);
}

// ---- simplex_pg: grid ceil(n / 64), block 64.  M [k x k] float64 row-major, device.
template <int KP>
__global__ __launch_bounds__(SIMPLEX_PG_WG) void simplex_pg_kernel(const float* A, int64_t lda, const float* Q, int64_t ldq, const double* M,
                                                                   float inv_L, int iters, int64_t n, int k, float* out, int64_t ldo) {
  __shared__ float Ms[KP * KP];                    // Ms[j KP + l] = (float)M[l, j], zeros past k: column j of M is contiguous
  for (int t = (int)threadIdx.x; t < KP * KP; t += SIMPLEX_PG_WG) {
    const int j = t / KP, l = t - j * KP;
    Ms[t] = (l < k && j < k) ? (float)M[l * k + j] : 0.f;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * SIMPLEX_PG_WG + threadIdx.x;
  if (i >= n) return;
  float a[KP], q[KP], u[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    a[j] = j < k ? A[i * lda + j] : 0.f;           // (a zero times a zero of Ms: the chain passes the padding unchanged)
    q[j] = j < k ? Q[i * ldq + j] : 0.f;
  }
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    SimplexRule rule;
    bool bad = false;
    float umax = -INFINITY;
    double sum = 0.0;
    asm volatile("" ::: "memory");                 // (M is read from LDS again in every iteration: KP^2 words do not fit the registers)
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int l = 0; l < KP; ++l) acc = fmaf(a[l], Ms[j * KP + l], acc);
      u[j] = -INFINITY;
      if (j < k) {
        u[j] = fmaf(-inv_L, acc - q[j], a[j]);
        bad |= !simplex_finite(u[j]);
        umax = fmaxf(umax, u[j]);
        sum += (double)u[j];
      }
    }
    int nmax = 0, cnt = k;
#pragma unroll
    for (int j = 0; j < KP; ++j) nmax += u[j] == umax;
    rule.bad = bad, rule.limit = false, rule.umax = umax, rule.nmax = nmax;
    rule.tau = (sum - 1.0) / (double)cnt;
    rule.thr = rule.tau;
    bool done = bad;
    while (!done) {
      int c = 0;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if ((double)u[j] > rule.thr) {
          ++c;
          s += (double)u[j];
        }
      if (c == 0) rule.limit = true, done = true;
      else if (c == cnt) done = true;
      else {
        cnt = c;
        rule.tau = (s - 1.0) / (double)c;
        rule.thr = fmax(rule.thr, rule.tau);
      }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) a[j] = j < k ? rule(u[j]) : 0.f;
  }
#pragma unroll
  for (int j = 0; j < KP; ++j)
    if (j < k) out[i * ldo + j] = a[j];
}

#endif  // __HIPCC__

}  // namespace eofx
