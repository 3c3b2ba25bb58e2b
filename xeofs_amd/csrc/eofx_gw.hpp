// eofx_gw.hpp -- geographically weighted PCA (xeofs/single/gwpca.py, xeofs/utils/optional/numba_utils.py:13-76).
//
// For every location i of the preprocessed field X (n locations x p features) the reference weighs ALL n locations by a
// kernel of their distance to i and takes the PCA of the weighted neighbourhood:
//     w_ij = K(d_ij / b),   W_i = sum_j w_ij,   mu_i = sum_j w_ij x_j / W_i,
//     C_i  = sum_j w_ij (x_j - mu_i)(x_j - mu_i)^T,   eigenpairs of C_i / W_i.
// Here the locations are cut into spatially compact tiles of GW_T (host side, eofx_abi.hip: Morton order, a bound per
// tile, the CSR list of neighbour tiles whose weights are not all exactly 0 in float64) and
//   gw_cov_kernel       accumulates, per centre tile and neighbour tile, the packed upper triangle of the AUGMENTED
//                       moment matrix sum_j w_ij [y_j; 1][y_j; 1]^T with y_j = x_j - r (r = the centre tile's mean: a shift
//                       shared by the tile that keeps the cancellation small).  Its last column holds sum w y and W.
//   gw_finalize_kernel  C / W = (S_yy - S_y S_y^T / W) / W (dense, symmetric) and the total variance trace(C) / W,
//   gw_syev_kernel      the batched symmetric eigensolver (p <= 64): cyclic Jacobi with round-robin (parallel) ordering,
//                       matrix and eigenvectors in LDS, one workgroup per matrix.
// Float64 throughout, no atomics, every sum in a fixed order: results are reproducible bit for bit.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"
#include "eofx_gwplan.hpp"    // GW_T, GW_EARTH_RADIUS

namespace eofx {

constexpr int GW_R = 8;           // accumulators per thread of gw_cov_kernel (256 * GW_R packed entries per workgroup)
constexpr int GW_PMAX = 256;      // features: the neighbour tile [GW_T x (p + 1)] float64 must fit in LDS
constexpr int GW_EIG_PMAX = 64;   // gw_syev_kernel: a [64 x 65] matrix and eigenvectors in LDS

// geo[3 s + .]: {lon, lat (radians), cos lat} for haversine, {x, y, 0} for euclidean
__device__ __forceinline__ double gw_weight(const double* gi, const double* gj, int metric, int kernel, double bw) {
  double d;
  if (metric == EOFX_GW_METRIC_HAVERSINE) {      // distance_metrics.py _haversine_distance_nb
    const double slat = sin(0.5 * (gj[1] - gi[1])), slon = sin(0.5 * (gj[0] - gi[0]));
    const double a = fmin(fmax(slat * slat + gi[2] * gj[2] * (slon * slon), 0.0), 1.0);
    d = GW_EARTH_RADIUS * (2.0 * atan2(sqrt(a), sqrt(1.0 - a)));
  } else {
    const double dx = gj[0] - gi[0], dy = gj[1] - gi[1];
    d = sqrt(dx * dx + dy * dy);
  }
  const double u = d / bw;
  if (kernel == EOFX_GW_KERNEL_BISQUARE) {       // kernels.py: (1 - u^2)^2 where d <= b, else 0
    const double t = 1.0 - u * u;
    return d <= bw ? t * t : 0.0;
  }
  if (kernel == EOFX_GW_KERNEL_GAUSSIAN) return exp(-0.5 * (u * u));
  return exp(-0.5 * u);                          // exponential: the 0.5 is the reference's
}

// grid (centre tiles, passes), block 256.  Centre tile ct = sorted centre positions [ct GW_T, +GW_T) of this chunk
// (perm_c: sorted position -> row of X), neighbour tile t = sorted positions [t GW_T, +GW_T) of all n locations.
// Pass y owns the packed entries [y 256 GW_R, (y + 1) 256 GW_R) of the tile's GW_T x P2a block (P2a = (p+1)(p+2)/2).
// S[(ct GW_T + i) P2a + ab] = sum over the listed neighbour tiles (ascending), j ascending, of w_ij z_ja z_jb, z = [y; 1].
__global__ __launch_bounds__(256) void gw_cov_kernel(const float* __restrict__ X, int64_t ldx, int p,
                                                     const double* __restrict__ geo_n, const int64_t* __restrict__ perm_n,
                                                     int64_t n, const double* __restrict__ geo_c,
                                                     const int64_t* __restrict__ perm_c, int64_t nc,
                                                     const int* __restrict__ rowptr, const int* __restrict__ cols, int metric,
                                                     int kernel, double bw, double* __restrict__ S) {
  __shared__ double ys[GW_T * (GW_PMAX + 1)];
  __shared__ double w[GW_T * GW_T];
  __shared__ double r[GW_PMAX];
  __shared__ double gc[GW_T * 3];
  const int q = p + 1, tid = threadIdx.x, ct = blockIdx.x;
  const int64_t P2a = (int64_t)q * (q + 1) / 2;
  const int64_t c0 = (int64_t)ct * GW_T;
  const int tc = (int)min((int64_t)GW_T, nc - c0);
  for (int a = tid; a < p; a += 256) {
    double s = 0.0;
    for (int i = 0; i < tc; ++i) s += (double)X[perm_c[c0 + i] * ldx + a];
    r[a] = s / (double)tc;
  }
  if (tid < GW_T * 3) gc[tid] = tid / 3 < tc ? geo_c[c0 * 3 + tid] : 0.0;
  int ei[GW_R], ea[GW_R], eb[GW_R];
  double acc[GW_R];
  const int64_t total = (int64_t)GW_T * P2a;
#pragma unroll
  for (int k = 0; k < GW_R; ++k) {
    const int64_t e = ((int64_t)blockIdx.y * GW_R + k) * 256 + tid;
    acc[k] = 0.0;
    ei[k] = -1;
    ea[k] = eb[k] = 0;
    if (e < total) {
      int ab = (int)(e % P2a), a = 0;
      while (ab >= q - a) {
        ab -= q - a;
        ++a;
      }
      ei[k] = (int)(e / P2a);
      ea[k] = a;
      eb[k] = a + ab;
    }
  }
  __syncthreads();
  for (int t = rowptr[ct]; t < rowptr[ct + 1]; ++t) {
    const int64_t n0 = (int64_t)cols[t] * GW_T;
    const int tn = (int)min((int64_t)GW_T, n - n0);
    {
      const int i = tid / GW_T, j = tid % GW_T;
      w[tid] = (i < tc && j < tn) ? gw_weight(&gc[3 * i], &geo_n[3 * (n0 + j)], metric, kernel, bw) : 0.0;
    }
    for (int e = tid; e < GW_T * q; e += 256) {
      const int j = e / q, a = e % q;
      double v = 0.0;
      if (j < tn) v = a < p ? (double)X[perm_n[n0 + j] * ldx + a] - r[a] : 1.0;
      ys[e] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GW_R; ++k) {
      if (ei[k] >= 0) {
        const double* wr = &w[ei[k] * GW_T];
        double s = acc[k];
        for (int j = 0; j < GW_T; ++j) s += (wr[j] * ys[j * q + ea[k]]) * ys[j * q + eb[k]];
        acc[k] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < GW_R; ++k) {
    if (ei[k] >= 0 && ei[k] < tc) {
      const int64_t e = ((int64_t)blockIdx.y * GW_R + k) * 256 + tid;
      S[c0 * P2a + e] = acc[k];
    }
  }
}

__device__ __forceinline__ int64_t gw_packed(int q, int a, int b) {    // a <= b < q, row-major upper triangle
  return (int64_t)a * q - (int64_t)a * (a - 1) / 2 + (b - a);
}

// one workgroup per centre (sorted position s of the chunk): A[row] = C / W (p x p, dense), tv[perm_c[s] - first] =
// trace(C) / W; row = s when sorted_out (the chunk's sorted order, gw_syev_kernel maps it back), else perm_c[s] - first
__global__ __launch_bounds__(256) void gw_finalize_kernel(const double* __restrict__ S, int p, const int64_t* __restrict__ perm_c,
                                                          int64_t first, int sorted_out, double* __restrict__ A,
                                                          double* __restrict__ tv) {
  const int q = p + 1;
  const int64_t P2a = (int64_t)q * (q + 1) / 2, s = blockIdx.x;
  const double* Sp = S + s * P2a;
  const int64_t loc = perm_c[s] - first;
  const double W = Sp[gw_packed(q, p, p)];
  double* Ap = A + (sorted_out ? s : loc) * p * p;
  for (int e = threadIdx.x; e < p * p; e += 256) {
    const int r = e / p, c = e % p, a = min(r, c), b = max(r, c);
    Ap[e] = (Sp[gw_packed(q, a, b)] - Sp[gw_packed(q, a, p)] * Sp[gw_packed(q, b, p)] / W) / W;
  }
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int a = 0; a < p; ++a) t += (Sp[gw_packed(q, a, a)] - Sp[gw_packed(q, a, p)] * Sp[gw_packed(q, a, p)] / W) / W;
    tv[loc] = t;
  }
}

// a strict total order for the eigenvalue sort: descending, NaN after every number, ties by index
__device__ __forceinline__ bool gw_before(double x, int i, double y, int j) {
  const bool nx = x != x, ny = y != y;
  if (nx != ny) return ny;
  if (!nx && x != y) return x > y;
  return i < j;
}

// Batched symmetric eigensolver, p <= 64, one workgroup per matrix.  A [batch x p x p] float64 (the upper triangle is
// read), w [batch x k] = the k largest eigenvalues (descending, index-stable ties, negative rounding clamped to 0),
// V [batch x p x k] = their eigenvectors (row out_index[b] of w and V when out_index is given), each column signed by the rule of get_deterministic_sign_multiplier
// (xeofs/linalg/_numpy/_svd.py:13-33: positive where |max| >= |min|).  Cyclic Jacobi: each round applies p/2 disjoint
// rotations (round-robin ordering, Brent & Luk 1985) to the columns and then the rows of A and to the columns of V; a
// sweep is p - 1 rounds (p even; a dummy index when p is odd); the loop ends when the off-diagonal Frobenius norm is
// at most p eps times the whole, or after max_sweeps.
template <typename VT>
__global__ __launch_bounds__(256) void gw_syev_kernel(const double* __restrict__ A, int p, int k, int max_sweeps,
                                                      const int64_t* __restrict__ out_index, double* __restrict__ w,
                                                      VT* __restrict__ V) {
  constexpr int LD = GW_EIG_PMAX + 1;
  __shared__ double a[GW_EIG_PMAX * LD];
  __shared__ double v[GW_EIG_PMAX * LD];
  __shared__ double red0[256], red1[256];
  __shared__ double cs[GW_EIG_PMAX / 2], sn[GW_EIG_PMAX / 2];
  __shared__ int pp[GW_EIG_PMAX / 2], qq[GW_EIG_PMAX / 2];
  __shared__ int order[GW_EIG_PMAX];
  __shared__ double sgn[GW_EIG_PMAX];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, row = out_index ? out_index[b] : b;
  const double* Ab = A + b * p * p;
  for (int e = tid; e < p * p; e += 256) {
    const int r = e / p, c = e % p;
    a[r * LD + c] = Ab[(int64_t)min(r, c) * p + max(r, c)];
    v[r * LD + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  const int m = p + (p & 1), half = m / 2;
  const double tol = (double)p * 2.220446049250313e-16;
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < p * p; e += 256) {
      const int r = e / p, c = e % p;
      const double x = a[r * LD + c];
      if (r == c)
        dg += x * x;
      else
        off += x * x;
    }
    red0[tid] = off;
    red1[tid] = dg;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        red0[tid] += red0[tid + s];
        red1[tid] += red1[tid + s];
      }
      __syncthreads();
    }
    const bool done = red0[0] <= tol * tol * (red0[0] + red1[0]);
    __syncthreads();
    if (done) break;
    for (int round = 0; round < m - 1; ++round) {
      if (tid < half) {
        int i1, i2;
        if (tid == 0) {
          i1 = round;
          i2 = m - 1;
        } else {
          i1 = (round + tid) % (m - 1);
          i2 = (round - tid + m - 1) % (m - 1);
        }
        const int P = min(i1, i2), Q = max(i1, i2);
        double c = 1.0, s = 0.0;
        if (Q < p) {
          const double apq = a[P * LD + Q];
          if (apq != 0.0) {
            const double tau = (a[Q * LD + Q] - a[P * LD + P]) / (2.0 * apq);
            const double t = fabs(tau) > 1e150 ? 0.5 / tau : (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
          }
        }
        pp[tid] = P;
        qq[tid] = Q;
        cs[tid] = c;
        sn[tid] = s;
      }
      __syncthreads();
      for (int e = tid; e < half * p; e += 256) {       // A <- A J, V <- V J (columns P, Q of every row)
        const int kk = e / p, r = e % p, P = pp[kk], Q = qq[kk];
        if (Q < p && sn[kk] != 0.0) {
          const double c = cs[kk], s = sn[kk];
          const double x = a[r * LD + P], y = a[r * LD + Q];
          a[r * LD + P] = c * x - s * y;
          a[r * LD + Q] = s * x + c * y;
          const double vx = v[r * LD + P], vy = v[r * LD + Q];
          v[r * LD + P] = c * vx - s * vy;
          v[r * LD + Q] = s * vx + c * vy;
        }
      }
      __syncthreads();
      for (int e = tid; e < half * p; e += 256) {       // A <- J^T A (rows P, Q)
        const int kk = e / p, col = e % p, P = pp[kk], Q = qq[kk];
        if (Q < p && sn[kk] != 0.0) {
          const double c = cs[kk], s = sn[kk];
          const double x = a[P * LD + col], y = a[Q * LD + col];
          a[P * LD + col] = c * x - s * y;
          a[Q * LD + col] = s * x + c * y;
        }
      }
      __syncthreads();
      if (tid < half && qq[tid] < p && sn[tid] != 0.0) {   // the rotation annihilates (P, Q) up to rounding
        a[pp[tid] * LD + qq[tid]] = 0.0;
        a[qq[tid] * LD + pp[tid]] = 0.0;
      }
      __syncthreads();
    }
  }
  if (tid < p) {        // rank of eigenvalue tid under gw_before: a permutation whatever the values
    const double d = a[tid * LD + tid];
    int rank = 0;
    for (int j = 0; j < p; ++j) rank += gw_before(a[j * LD + j], j, d, tid) ? 1 : 0;
    order[rank] = tid;
  }
  __syncthreads();
  if (tid < k) {
    const int col = order[tid];
    double mx = v[col], mn = v[col];
    for (int r = 1; r < p; ++r) {
      mx = fmax(mx, v[r * LD + col]);
      mn = fmin(mn, v[r * LD + col]);
    }
    sgn[tid] = fabs(mx) >= fabs(mn) ? 1.0 : -1.0;
    const double d = a[col * LD + col];
    w[row * k + tid] = d != d ? d : fmax(d, 0.0);     // NaN input stays visible
  }
  __syncthreads();
  for (int e = tid; e < p * k; e += 256) {
    const int r = e / k, mode = e % k;
    V[row * p * k + e] = (VT)(sgn[mode] * v[r * LD + order[mode]]);
  }
}

}  // namespace eofx
