// eofx_ica.hpp -- the operator of independent component analysis (Hyvarinen & Oja 2000; Hannachi et al. 2009; single/ica.py):
// the parallel FastICA fixed-point iteration of R independent restarts on one white score panel Z [n x q].  One iteration is
// two plain launches in stream order -- no cooperative launch, no grid-wide barrier, no spin-wait.
//
//   project           s_j = the float32 fmaf chain sum_i w_ji z_i from 0, i ascending, w_ji = (float)W_ji rounded once.
//   evaluate          in float32 (u = alpha s, e = expf(-s s / 2), p = s s):
//                       logcosh  g = tanhf(u)   g' = alpha fmaf(-g, g, 1)   G = (|u| + log1pf(expf(-2 |u|)) - ln 2) / alpha
//                       exp      g = s e        g' = fmaf(-s, s, 1) e       G = -e     (g' = 0 where e = 0)
//                       cube     g = p s        g' = 3 p                    G = p p / 4
//   sum               in float64:  M_ji = sum_rows g_j z_i,  b_j = sum g'_j,  h_j = sum G_j,  nused = the rows without a NaN or
//                     an infinity -- the others take part in nothing.
//   step              W1 = M / nused - diag(b / nused) W;  W+ = (W1 W1^T)^-1/2 W1, the orthogonal polar factor of W1, float64.
//                     nused = 0, a W1 that is not finite, sigma_min^2 <= q 2^-52 sigma_max^2 (the singular values of W1), or a
//                     Jacobi iteration that still rotates in its 60th sweep: status = 2 and W stays.  Otherwise lim = max_j | |sum_i W+_ji W_ji| - 1 |, W = W+, ++iters and status = 1
//                     when lim < tol (scikit-learn's rule).
//
//   ica_moments_kernel<FUN, QP>   grid (B, R), 256 threads.  Reads status[r] first and returns, the whole workgroup, before any
//                     barrier when the restart is not running (force = the moment pass alone, max_iter = 0, runs for all).
//                     W as float32 in LDS [q x QP], read as 16-byte broadcasts; a thread's row in QP registers (QP = 4, 8, 16
//                     or 32 >= q; zeros past q pass through the chain unchanged).  A workgroup walks its rows in slabs of 256,
//                     a wave 64 rows of a slab: the wave stages z and then, one after the other, g, g' and G as float32 in
//                     LDS and multiplies on the fp64 matrix cores (eofx_mfma64.hpp) -- g^T z into T x T tiles of 16 x 16
//                     (T = max(1, QP / 16)), g'^T e and G^T e into T tiles each, e the column (1, 0, .., 0): float32 operands
//                     widened to float64 make every product exact, and the sums b and h ride the same instruction.  The
//                     owner-lane LDS accumulators of the Lloyd kernel would do 64 dependent LDS read-modify-writes per slab
//                     and lane where this does 16 matrix instructions per tile; the pass is bound by its launches and by
//                     reading Z, not by either.  After the last slab the four waves' tiles are added in LDS,
//                     wave ascending, and the q^2 + 2 q + 1 float64 partial sums go to the workgroup's own slot of scratch.
//   ica_update_kernel   grid R, 256 threads.  Adds the partials with b ascending, forms W1, and finds the polar factor by a
//                     one-sided (Hestenes) Jacobi SVD in LDS, round-robin pairs as in eofx_spca.hpp: the columns of A = W1^T
//                     are rotated until orthogonal, A J = U Sigma, so that W1 = J Sigma U^T and W+ = J U^T -- no squaring of
//                     the condition number.  The up to 16 pairs of a round take 16 lanes each: a lane holds two rows of its
//                     pair's columns, the three inner products are reduced by an xor butterfly, and a round costs one barrier.
//                     Writes lim, W, iters, status; W1, gmean, nused where asked for.
//
// Every order of summation is a function of (n, q) alone; no atomics; two runs are equal bit for bit; a restart's result does
// not depend on the others.  Nothing past column q of a row of Z is read.  gfx950 only.
//
// The constants and the plan are plain C++: a host compiler that does not define __HIPCC__ sees them and not the kernels
// (tests/ica_shim.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "eofx.h"
#include "eofx_mfma64.hpp"
#endif

namespace eofx {

constexpr int ICA_QMAX = 32;               // sources: a row in 32 registers
constexpr int ICA_NMAX = 4194304;          // rows
constexpr int ICA_RMAX = 1024;             // restarts of one call
constexpr int ICA_ITER_MAX = 64;           // iterations of one call: 128 launches
constexpr int ICA_WG = 256;                // threads of a workgroup
constexpr int ICA_BMAX = 512;              // row blocks of a restart at the most
constexpr int ICA_SWEEP_MAX = 60;          // Jacobi sweeps of one decorrelation; a last sweep that still rotated is status 2

// launch shape for n rows of q columns (within the limits above): a function of (n, q) alone
struct IcaPlan {
  int64_t blocks;   // B: row blocks of a restart
  int64_t rows;     // rows per block, a multiple of 256
  int qp;           // the register-width tier: 4, 8, 16 or 32 >= q
  int qw;           // columns of a staged row: max(qp, 16), the width of T tiles
  int slot;         // float64 partial sums of a block: q^2 + 2 q + 1
  size_t lds;       // dynamic LDS of the moments kernel in bytes
};
inline IcaPlan ica_plan(int64_t n, int q) {
  IcaPlan pl;
  const int64_t per = (int64_t)ICA_WG * ICA_BMAX;
  const int64_t f = (n + per - 1) / per;
  pl.rows = ICA_WG * (f < 1 ? 1 : f);
  pl.blocks = (n + pl.rows - 1) / pl.rows;
  int qp = 4;
  while (qp < q) qp <<= 1;
  pl.qp = qp, pl.qw = qp < 16 ? 16 : qp;
  pl.slot = q * q + 2 * q + 1;
  const int nw = ICA_WG / 64, t = pl.qw / 16;
  const size_t stage = (size_t)nw * 2 * 64 * (pl.qw + 1) * sizeof(float);            // z and one of g, g', G per wave
  const size_t red = (size_t)nw * (t * t + 2 * t) * 256 * sizeof(double);            // the waves' tiles, after the last slab
  pl.lds = (size_t)q * qp * sizeof(float) + (stage > red ? stage : red);
  return pl;
}
// float64 words of scratch for R restarts: R B (q^2 + 2 q + 1), from the context's arena, which grows to it and keeps it --
// 2.2 MB at (n, q, R) = (10000, 32, 50), 357 MB at (10000, 32, 1024), 4.6 GB at the limits (4194304, 32, 1024)
inline size_t ica_scratch(int64_t n, int q, int64_t R) {
  const IcaPlan pl = ica_plan(n, q);
  return (size_t)R * (size_t)pl.blocks * (size_t)pl.slot;
}

#if defined(__HIPCC__)

__device__ __forceinline__ bool ica_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// g, g', G of the contrast FUN at s
template <int FUN>
__device__ __forceinline__ void ica_contrast(float s, float alpha, float& g, float& gp, float& G) {
  if (FUN == 0) {
    const float u = alpha * s, a = fabsf(u);
    g = tanhf(u);
    gp = alpha * fmaf(-g, g, 1.f);
    G = ((a + log1pf(expf(-2.f * a))) - 0.69314718055994531f) / alpha;
  } else if (FUN == 1) {
    const float e = expf(-0.5f * (s * s));
    g = s * e;
    gp = e == 0.f ? 0.f : fmaf(-s, s, 1.f) * e;                  // (0 and not inf 0 where s s overflows)
    G = -e;
  } else {
    const float p = s * s;
    g = p * s;
    gp = 3.f * p;
    G = 0.25f * (p * p);
  }
}

// ---- grid (B, R), block 256, dynamic LDS pl.lds.  part [R x B x slot] float64.
template <int FUN, int QP>
__global__ __launch_bounds__(ICA_WG) void ica_moments_kernel(const float* __restrict__ Z, int64_t n, int q, int64_t ldz,
                                                              const double* __restrict__ W, const int32_t* __restrict__ status,
                                                              int force, float alpha, IcaPlan pl, double* __restrict__ part) {
  const int64_t rr = blockIdx.y;
  if (!force && status[rr] != 0) return;                          // (uniform over the workgroup; before any barrier)
  extern __shared__ __align__(16) unsigned char ica_lds[];
  constexpr int NW = ICA_WG / 64, QW = QP < 16 ? 16 : QP, QS = QW + 1, T = QW / 16;
  float* Ws = (float*)ica_lds;                                    // [q x QP]
  float* stage = Ws + q * QP;
  double* red = (double*)stage;                                   // (the stage again, after the last slab)
  const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
  float* zs = stage + (size_t)w * 2 * 64 * QS;                    // [64 x QS] the wave's rows
  float* as = zs + 64 * QS;                                       // [64 x QS] g, then g', then G
  const Mfma64Lane ln = mfma64_lane();

  const double* Wr = W + rr * q * q;
  for (int t = tid; t < q * QP; t += ICA_WG) {
    const int j = t / QP, i = t - j * QP;
    Ws[t] = i < q ? (float)Wr[j * q + i] : 0.f;
  }
  for (int t = tid; t < NW * 2 * 64 * QS; t += ICA_WG) stage[t] = 0.f;   // (the columns past q of a staged row stay zero)
  __syncthreads();

  f64x4 accM[T][T], accB[T], accH[T];
  mfma64_zero(accM), mfma64_zero(accB), mfma64_zero(accH);
  int used = 0;
  const double e0 = ln.c == 0 ? 1.0 : 0.0;                        // the column (1, 0, .., 0) of the sums b and h
  const int64_t row0 = (int64_t)blockIdx.x * pl.rows;
  const int slabs = (int)(pl.rows / ICA_WG);
  for (int sl = 0; sl < slabs; ++sl) {
    const int64_t row = row0 + (int64_t)sl * ICA_WG + tid;
    const bool live = row < n;
    float z[QP];
    bool ok = live;
#pragma unroll
    for (int i = 0; i < QP; ++i) {
      z[i] = (live && i < q) ? Z[row * ldz + i] : 0.f;
      ok = ok && ica_finite(z[i]);
    }
    used += ok ? 1 : 0;
#pragma unroll
    for (int i = 0; i < QP; ++i) zs[lane * QS + i] = ok ? z[i] : 0.f;
    float gp[QP], G[QP];
#pragma unroll
    for (int j = 0; j < QP; ++j) {
      float g = 0.f;
      gp[j] = 0.f, G[j] = 0.f;
      if (j < q && ok) {
        const float4* wj = (const float4*)(Ws + j * QP);
        float s = 0.f;
#pragma unroll
        for (int i4 = 0; i4 < QP / 4; ++i4) {
          const float4 v = wj[i4];
          s = fmaf(v.x, z[4 * i4 + 0], s);
          s = fmaf(v.y, z[4 * i4 + 1], s);
          s = fmaf(v.z, z[4 * i4 + 2], s);
          s = fmaf(v.w, z[4 * i4 + 3], s);
        }
        ica_contrast<FUN>(s, alpha, g, gp[j], G[j]);
      }
      as[lane * QS + j] = g;
    }
    __syncthreads();                                              // (z and g of the wave's 64 rows are staged)
#pragma unroll 4
    for (int st = 0; st < 16; ++st) {
      const int r = 4 * st + ln.k;
      double a[T], b[T];
#pragma unroll
      for (int x = 0; x < T; ++x) a[x] = (double)as[r * QS + 16 * x + ln.c], b[x] = (double)zs[r * QS + 16 * x + ln.c];
#pragma unroll
      for (int x = 0; x < T; ++x)
#pragma unroll
        for (int y = 0; y < T; ++y) mfma64_step(accM[x][y], a[x], b[y]);
    }
    __syncthreads();                                              // (g is read)
#pragma unroll
    for (int j = 0; j < QP; ++j) as[lane * QS + j] = gp[j];
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < 16; ++st) {
      const int r = 4 * st + ln.k;
#pragma unroll
      for (int x = 0; x < T; ++x) mfma64_step(accB[x], (double)as[r * QS + 16 * x + ln.c], e0);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < QP; ++j) as[lane * QS + j] = G[j];
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < 16; ++st) {
      const int r = 4 * st + ln.k;
#pragma unroll
      for (int x = 0; x < T; ++x) mfma64_step(accH[x], (double)as[r * QS + 16 * x + ln.c], e0);
    }
    __syncthreads();                                              // (the stage is free again)
  }
  // the waves' tiles into LDS: wave w, tile t at red[(w NT + t) 256 + row 16 + col], NT = T T + 2 T
  constexpr int NT = T * T + 2 * T;
  double* red_w = red + (size_t)w * NT * 256;
#pragma unroll
  for (int x = 0; x < T; ++x) {
#pragma unroll
    for (int y = 0; y < T; ++y)
      mfma64_each(accM[x][y], [&](int r, int c, double v) { red_w[(x * T + y) * 256 + r * 16 + c] = v; });
    mfma64_each(accB[x], [&](int r, int c, double v) { red_w[(T * T + x) * 256 + r * 16 + c] = v; });
    mfma64_each(accH[x], [&](int r, int c, double v) { red_w[(T * T + T + x) * 256 + r * 16 + c] = v; });
  }
  for (int s = 32; s >= 1; s >>= 1) used += __shfl_xor(used, s, 64);
  __shared__ int s_used[NW];
  if (lane == 0) s_used[w] = used;
  __syncthreads();
  double* out = part + (rr * pl.blocks + blockIdx.x) * (int64_t)pl.slot;
  const int qq = q * q;
  for (int e = tid; e < pl.slot; e += ICA_WG) {
    double v = 0.0;
    if (e < qq) {
      const int j = e / q, i = e - j * q;
      const int t = (j >> 4) * T + (i >> 4), o = (j & 15) * 16 + (i & 15);
      for (int x = 0; x < NW; ++x) v += red[((size_t)x * NT + t) * 256 + o];
    } else if (e < qq + 2 * q) {
      const int which = (e - qq) / q, j = (e - qq) - which * q;
      const int t = T * T + which * T + (j >> 4), o = (j & 15) * 16;
      for (int x = 0; x < NW; ++x) v += red[((size_t)x * NT + t) * 256 + o];
    } else {
      int m = 0;
      for (int x = 0; x < NW; ++x) m += s_used[x];
      v = (double)m;
    }
    out[e] = v;
  }
}

// ---- grid R, block 256.  advance = 0: the moment pass alone (W1, gmean, nused; W, status, iters, lim untouched).
__global__ __launch_bounds__(ICA_WG) void ica_update_kernel(const double* __restrict__ part, int64_t B, int q, double tol, int advance,
                                                             double* __restrict__ W, int32_t* __restrict__ status,
                                                             int32_t* __restrict__ iters, double* __restrict__ W1o,
                                                             double* __restrict__ gmean, double* __restrict__ lim,
                                                             long long* __restrict__ nused) {
  const int64_t rr = blockIdx.x;
  if (advance && status[rr] != 0) return;                         // (uniform; before any barrier)
  __shared__ double sum[ICA_QMAX * ICA_QMAX + 2 * ICA_QMAX + 1];
  __shared__ double M[ICA_QMAX * ICA_QMAX];                       // column c of A = W1^T, i.e. row c of W1, at M[c q ...]
  __shared__ double J[ICA_QMAX * ICA_QMAX];                       // column c at J[c q ...]
  __shared__ double Wo[ICA_QMAX * ICA_QMAX];                      // the W of entry
  __shared__ double sig[ICA_QMAX], dots[ICA_QMAX];
  __shared__ int rot, bad;
  const int tid = (int)threadIdx.x, qq = q * q, slot = qq + 2 * q + 1, pr = tid >> 4, sub = tid & 15;
  const double* prt = part + rr * B * slot;
  for (int e = tid; e < slot; e += ICA_WG) {
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) s += prt[b * slot + e];
    sum[e] = s;
  }
  for (int e = tid; e < qq; e += ICA_WG) Wo[e] = W[rr * qq + e];
  if (tid == 0) bad = 0;
  __syncthreads();
  const double cnt = sum[slot - 1];
  for (int e = tid; e < qq; e += ICA_WG) {
    const int j = e / q;
    const double v = sum[e] / cnt - (sum[qq + j] / cnt) * Wo[e];
    M[e] = v;
    J[e] = (j == e - j * q) ? 1.0 : 0.0;
    if (W1o) W1o[rr * qq + e] = v;
    if (!(fabs(v) <= 1.7976931348623157e308)) bad = 1;           // (a NaN or an infinity; every writer writes 1)
  }
  if (gmean && tid < q) gmean[rr * q + tid] = sum[qq + q + tid] / cnt;
  if (nused && tid == 0) *nused = (long long)cnt;                 // (the same value from every restart: it belongs to Z)
  if (!advance) return;                                           // (uniform)
  __syncthreads();
  if (bad || !(cnt > 0.0)) {                                      // (one LDS word and one sum, the same for all threads)
    if (tid == 0) status[rr] = 2;
    return;
  }
  // one-sided Jacobi: round-robin pairs of columns (Brent & Luk), a sweep is m - 1 rounds of disjoint rotations
  const int m = q + (q & 1), half = m / 2;
  const double eps = 2.220446049250313e-16 * (double)q;
  bool settled = m <= 1;
  for (int sweep = 0; sweep < ICA_SWEEP_MAX && m > 1; ++sweep) {
    if (tid == 0) rot = 0;
    __syncthreads();
    for (int round = 0; round < m - 1; ++round) {
      // pair pr of the round on the 16 lanes (pr, 0 .. 15) of one wave: lane `sub` holds the rows sub, sub + 16 of both columns,
      // of M and of J, and nobody else reads or writes them in this round -- one barrier a round
      int Pc = 0, Qc = q;
      if (pr < half) {
        int i1, i2;
        if (pr == 0) {
          i1 = round;
          i2 = m - 1;
        } else {
          i1 = (round + pr) % (m - 1);
          i2 = (round - pr + m - 1) % (m - 1);
        }
        Pc = min(i1, i2), Qc = max(i1, i2);
      }
      const bool on = Qc < q;
      double a = 0.0, b = 0.0, g = 0.0;
      if (on)
        for (int r = sub; r < q; r += 16) {
          const double x = M[Pc * q + r], y = M[Qc * q + r];
          a += x * x;
          b += y * y;
          g += x * y;
        }
      for (int sh = 8; sh >= 1; sh >>= 1) {                       // (an xor butterfly: the 16 lanes end on the same bits)
        a += __shfl_xor(a, sh, 64);
        b += __shfl_xor(b, sh, 64);
        g += __shfl_xor(g, sh, 64);
      }
      if (on && g != 0.0 && fabs(g) > eps * sqrt(a * b)) {
        const double zeta = (b - a) / (2.0 * g);
        const double tt = fabs(zeta) > 1e150 ? 0.5 / zeta : (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + tt * tt), sn = tt * c;
        if (sub == 0) rot = 1;
        for (int r = sub; r < q; r += 16) {
          const double x = M[Pc * q + r], y = M[Qc * q + r];
          M[Pc * q + r] = c * x - sn * y;
          M[Qc * q + r] = sn * x + c * y;
          const double u = J[Pc * q + r], v = J[Qc * q + r];
          J[Pc * q + r] = c * u - sn * v;
          J[Qc * q + r] = sn * u + c * v;
        }
      }
      __syncthreads();
    }
    const bool any = rot != 0;
    __syncthreads();
    if (!any) {
      settled = true;
      break;
    }
  }
  if (!settled) {                                                 // (one LDS word decided it, the same for all threads)
    if (tid == 0) status[rr] = 2;
    return;
  }
  if (tid < q) {
    double s = 0.0;
    for (int r = 0; r < q; ++r) s += M[tid * q + r] * M[tid * q + r];
    sig[tid] = s;                                                 // sigma^2
  }
  __syncthreads();
  double smin = sig[0], smax = sig[0];
  for (int c = 1; c < q; ++c) smin = fmin(smin, sig[c]), smax = fmax(smax, sig[c]);
  if (!(smax <= 1.7976931348623157e308) || !(smin > (double)q * 2.220446049250313e-16 * smax)) {      // (the same for all threads)
    if (tid == 0) status[rr] = 2;
    return;
  }
  // W+ = J U^T, U the normalised columns of M;  into the registers of the element's owner, then over M's place
  constexpr int PER = ICA_QMAX * ICA_QMAX / ICA_WG;
  double wp[PER];
#pragma unroll
  for (int x = 0; x < PER; ++x) {
    const int e = tid + x * ICA_WG;
    double s = 0.0;
    if (e < qq) {
      const int j = e / q, i = e - j * q;
      for (int c = 0; c < q; ++c) s += J[c * q + j] * (M[c * q + i] / sqrt(sig[c]));
    }
    wp[x] = s;
  }
  __syncthreads();
#pragma unroll
  for (int x = 0; x < PER; ++x)
    if (tid + x * ICA_WG < qq) M[tid + x * ICA_WG] = wp[x];
  __syncthreads();
  if (tid < q) {
    double s = 0.0;
    for (int i = 0; i < q; ++i) s += M[tid * q + i] * Wo[tid * q + i];
    dots[tid] = fabs(fabs(s) - 1.0);
  }
  __syncthreads();
  double l = dots[0];
  for (int j = 1; j < q; ++j) l = fmax(l, dots[j]);
  for (int e = tid; e < qq; e += ICA_WG) W[rr * qq + e] = M[e];
  if (tid == 0) {
    if (lim) lim[rr] = l;
    iters[rr] += 1;
    status[rr] = l < tol ? 1 : 0;
  }
}

#endif  // __HIPCC__

}  // namespace eofx
