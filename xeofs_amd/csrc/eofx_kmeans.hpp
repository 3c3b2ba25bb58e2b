// eofx_kmeans.hpp -- the operator of weather-regime clustering (Michelangeli, Vautard & Legras 1995; single/kmeans.py): Lloyd's
// k-means iteration of R independent restarts on one score panel Z [n x q], every restart running all of its iterations in
// one launch.
//
//   assign            d_ic = the float32 fmaf chain sum_j (z_ij - c_cj)^2 from 0, j ascending: t = z_ij - c_cj (rounded once),
//                     d = fmaf(t, t, d).  The direct form: a sum of non-negative terms, relative error about (q + 2) 2^-24.
//                     label_i = the c with the smallest d_ic, the lowest index among equals; mind2_i = that d_ic.  A row that
//                     holds a NaN or an infinity gets label -1 and mind2 = NaN and takes part in nothing: not in a count, a
//                     centroid, the inertia or the test for a changed label.
//   update            counts_c = the rows labelled c;  c_cj = (float)(sum_{i: label_i = c} (double)z_ij / counts_c): the sum
//                     in float64 in the order below, the division in float64, one rounding.  A cluster without rows keeps
//                     its centroid.
//   the loop          it = 0;  assign;  stop when it > 0 and no label differs from the assignment before (converged = 1) or
//                     when it == max_iter (converged = 0);  otherwise update, ++it, and again.  iters = it counts updates.
//                     The last thing a launch does is an assignment against the centroids it returns: labels, counts, mind2
//                     and inertia always belong to the returned C.  The first assignment of a launch has none before it and
//                     never counts as converged: max_iter = 0 is the assignment alone against C0, converged = 0.
//   inertia           the float64 sum of the float32 mind2_i: a thread's rows ascending, an xor butterfly over the wave, the
//                     waves ascending.
//   chaining          the state between two iterations is C alone, so one launch with max_iter = T returns the C, labels,
//                     counts, mind2 and inertia of T chained launches with max_iter = 1, bit for bit (a chain goes on
//                     counting one update per launch after the fixed point, which changes nothing).
//   the kernel        one workgroup of 256 threads per restart.  Thread t owns the rows t, t + 256, ...: one row at a time
//                     in QP registers (QP = the next power of two of q, at least 4; zeros past q pass through the chain
//                     unchanged), re-read from L2 in every iteration.  The centroids sit in LDS as [k x QP] and are read as
//                     broadcasts of 16 bytes.  The sums: a wave stages its 64 rows and labels in LDS; lane (g, j) = (lane /
//                     QP, lane % QP), g < G, j < q, then walks the rows g, g + G, ... of the wave in ascending order and adds
//                     z_rj to the float64 accumulator (wave, g, label_r, j) in LDS, which no other lane reads or writes; lane
//                     (g, 0) counts.  G = 64 / QP, halved while G k q > 1024: the accumulators take at most 4 x 1024 x 8 B =
//                     32 KiB.  A centroid entry is then the sum over the waves ascending and, within a wave, g ascending.
//                     Every order is a function of (n, q, k) alone.
//   the way out       the decision to leave the loop is one LDS word, written by thread 0 from the reduced count of changed
//                     labels and read by every thread after a barrier; every barrier is reached by all 256 threads (all loop
//                     bounds are functions of the shape).  The loop runs at most max_iter + 1 <= KMEANS_ITER_MAX + 1 times.
// No atomics; two runs are equal bit for bit.  Nothing past column q of a row of Z is read; nothing but the outputs is
// written; C may alias C0.  gfx950 only.
//
// The constants and the plan are plain C++: a host compiler that does not define __HIPCC__ sees them and not the kernel
// (tests/kmeans_shim.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "eofx.h"
#endif

namespace eofx {

constexpr int KMEANS_KMAX = 32;             // clusters
constexpr int KMEANS_QMAX = 32;             // columns of the score panel: a row in 32 registers
constexpr int KMEANS_NMAX = 262144;         // rows: 1024 per thread
constexpr int KMEANS_RMAX = 4096;           // restarts of one launch
constexpr int KMEANS_ITER_MAX = 1000;       // updates of one launch
constexpr int KMEANS_WG = 256;              // threads of a workgroup: one restart
constexpr int KMEANS_ACC_MAX = 1024;        // float64 accumulators of a wave: 8 KiB
constexpr int KMEANS_RED_BYTES = 64;        // 4 float64 + the inertia + 4 int32 + the word that ends the loop, padded to 16

// launch shape for n rows of q columns, k clusters and R restarts (within the limits above)
struct KmeansPlan {
  int64_t grid;     // workgroups: R
  int threads;      // KMEANS_WG
  int qp;           // the register-width tier: 4, 8, 16 or 32 >= q
  int groups;       // G: row groups of a wave in the accumulation
  int rpt;          // rows per thread: ceil(n / 256)
  size_t acc_off, c_off, stage_off, cnt_off, lab_off;   // byte offsets into the dynamic LDS
  size_t lds;       // dynamic LDS in bytes
};
inline KmeansPlan kmeans_plan(int64_t n, int q, int k, int64_t R) {
  KmeansPlan pl;
  pl.grid = R;
  pl.threads = KMEANS_WG;
  int qp = 4;
  while (qp < q) qp <<= 1;
  int g = 64 / qp;
  while (g > 1 && (int64_t)g * k * q > KMEANS_ACC_MAX) g >>= 1;
  pl.qp = qp, pl.groups = g;
  pl.rpt = (int)((n + KMEANS_WG - 1) / KMEANS_WG);
  const int nw = KMEANS_WG / 64;
  size_t off = KMEANS_RED_BYTES;                                         // (the words of the reductions come first)
  pl.acc_off = off, off += (size_t)nw * g * k * q * sizeof(double);      // (a multiple of 8)
  off = (off + 15) & ~(size_t)15;
  pl.c_off = off, off += (size_t)k * qp * sizeof(float);                 // (a multiple of 16: the broadcasts are 16 bytes wide)
  pl.stage_off = off, off += (size_t)nw * 64 * (qp + 1) * sizeof(float); // (a row stride of qp + 1 words: odd)
  pl.cnt_off = off, off += (size_t)nw * g * k * sizeof(int32_t);
  pl.lab_off = off, off += (size_t)KMEANS_WG * sizeof(int32_t);
  pl.lds = off;
  return pl;
}

#if defined(__HIPCC__)

__device__ __forceinline__ bool kmeans_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ---- grid R, block 256, dynamic LDS pl.lds.
template <int QP>
__global__ __launch_bounds__(KMEANS_WG) void kmeans_lloyd_kernel(const float* Z, int64_t n, int q, int64_t ldz, const float* C0, int k,
                                                                  int max_iter, KmeansPlan pl, int32_t* labels, float* C, int32_t* counts,
                                                                  double* inertia, int32_t* iters, int32_t* converged, float* mind2) {
  extern __shared__ __align__(16) unsigned char kmeans_lds[];     // (all of the LDS is dynamic: its base stays 16-byte aligned)
  double* red_d = (double*)kmeans_lds;             // [4]
  double& s_inertia = red_d[4];
  int* red_i = (int*)(kmeans_lds + 40);            // [4]
  int& s_stop = red_i[4];                          // 0: go on, 1: converged, 2: max_iter reached
  double* acc = (double*)(kmeans_lds + pl.acc_off);
  float* Cs = (float*)(kmeans_lds + pl.c_off);
  float* stage = (float*)(kmeans_lds + pl.stage_off);
  int* cnt = (int*)(kmeans_lds + pl.cnt_off);
  int* slab = (int*)(kmeans_lds + pl.lab_off);
  constexpr int NW = KMEANS_WG / 64, QS = QP + 1;
  const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int G = pl.groups, rpt = pl.rpt;
  const int64_t rr = blockIdx.x;
  const int nacc = NW * G * k * q, ncnt = NW * G * k;
  int32_t* lab_r = labels + rr * n;
  float* md_r = mind2 ? mind2 + rr * n : nullptr;
  // the lane's share of the accumulation: group g, column j
  const int ag = lane / QP, aj = lane - ag * QP;
  const bool aon = ag < G && aj < q;
  double* acc_l = acc + (size_t)(w * G + ag) * k * q + aj;     // + label q
  int* cnt_l = cnt + (w * G + ag) * k;                         // + label
  float* st_w = stage + w * 64 * QS;
  int* lab_w = slab + w * 64;

  for (int t = tid; t < k * QP; t += KMEANS_WG) {
    const int c = t / QP, j = t - c * QP;
    Cs[t] = j < q ? C0[(rr * k + c) * q + j] : 0.f;
  }
  int it = 0, stop = 0;
  for (int round = 0; round <= max_iter; ++round) {              // (stop is set at round == max_iter at the latest)
    for (int t = tid; t < nacc; t += KMEANS_WG) acc[t] = 0.0;
    for (int t = tid; t < ncnt; t += KMEANS_WG) cnt[t] = 0;
    __syncthreads();                                             // (the centroids and the zeros are in place)
    int changed = 0;
    double inert = 0.0;
    for (int b = 0; b < rpt; ++b) {
      const int64_t row = (int64_t)b * KMEANS_WG + tid;
      const bool live = row < n;
      float z[QP];
      bool ok = live;
#pragma unroll
      for (int j = 0; j < QP; ++j) {
        z[j] = (live && j < q) ? Z[row * ldz + j] : 0.f;
        ok = ok && kmeans_finite(z[j]);
      }
      int best = -1;
      float dbest = __uint_as_float(0x7fc00000u);
      if (ok) {
        for (int c = 0; c < k; ++c) {
          const float4* cc = (const float4*)(Cs + c * QP);
          float d = 0.f;
#pragma unroll
          for (int j4 = 0; j4 < QP / 4; ++j4) {
            const float4 v = cc[j4];
            float t;
            t = z[4 * j4 + 0] - v.x, d = fmaf(t, t, d);
            t = z[4 * j4 + 1] - v.y, d = fmaf(t, t, d);
            t = z[4 * j4 + 2] - v.z, d = fmaf(t, t, d);
            t = z[4 * j4 + 3] - v.w, d = fmaf(t, t, d);
          }
          if (c == 0 || d < dbest) best = c, dbest = d;
        }
        inert += (double)dbest;
      }
      if (live) {
        if (round > 0 && lab_r[row] != best) ++changed;          // (the thread's own store of the round before)
        lab_r[row] = best;
        if (md_r) md_r[row] = dbest;
      }
      // the wave's 64 rows and labels into LDS, then every accumulator's owner lane walks its rows
#pragma unroll
      for (int j = 0; j < QP; ++j) st_w[lane * QS + j] = z[j];
      lab_w[lane] = best;
      __syncthreads();
      if (aon) {
        for (int r = ag; r < 64; r += G) {
          const int c = lab_w[r];
          if (c >= 0) {
            acc_l[c * q] += (double)st_w[r * QS + aj];
            if (aj == 0) cnt_l[c] += 1;
          }
        }
      }
      __syncthreads();                                           // (the stage is free again)
    }
    for (int s = 32; s >= 1; s >>= 1) changed += __shfl_xor(changed, s, 64), inert += __shfl_xor(inert, s, 64);
    if (lane == 0) red_i[w] = changed, red_d[w] = inert;
    __syncthreads();
    if (tid == 0) {
      int ch = 0;
      double s = 0.0;
      for (int x = 0; x < NW; ++x) ch += red_i[x], s += red_d[x];
      s_inertia = s;
      s_stop = (round > 0 && ch == 0) ? 1 : (round >= max_iter ? 2 : 0);
    }
    __syncthreads();
    stop = s_stop;                                               // (one LDS word, the same for all 256 threads)
    if (stop) break;
    for (int e = tid; e < k * q; e += KMEANS_WG) {
      const int c = e / q, j = e - c * q;
      int m = 0;
      double s = 0.0;
      for (int x = 0; x < NW * G; ++x) m += cnt[x * k + c], s += acc[(size_t)(x * k + c) * q + j];
      if (m > 0) Cs[c * QP + j] = (float)(s / (double)m);
    }
    ++it;
    __syncthreads();                                             // (the sums are read before they are zeroed)
  }
  for (int e = tid; e < k * q; e += KMEANS_WG) {
    const int c = e / q, j = e - c * q;
    C[(rr * k + c) * q + j] = Cs[c * QP + j];
  }
  if (tid < k) {
    int m = 0;
    for (int x = 0; x < NW * G; ++x) m += cnt[x * k + tid];
    counts[rr * k + tid] = m;
  }
  if (tid == 0) inertia[rr] = s_inertia, iters[rr] = it, converged[rr] = stop == 1;
}

#endif  // __HIPCC__

}  // namespace eofx
