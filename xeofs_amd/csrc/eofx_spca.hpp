// eofx_spca.hpp -- sparse PCA by variable projection (Erichson et al. 2020; xeofs/single/_numpy/_sparse_pca.py:383-563).
//
// With the thin SVD C = U diag(D) V^T of the (compressed) data matrix, V [p x l] orthonormal, every p-long quantity of the
// non-robust iteration stays a streaming pass over the rows of V and B [p x k]:
//     P  = V^T B                    (l x k),       M = D^2 P,      Z = V M,  polar(Z) = V polar(M) = V Qa,
//     W  = D^2 (Qa - P)             (l x k),       G = V W - beta B,
//     b_j <- prox(b_j + nu (v_j W - beta b_j), kappa)        row by row,
//     obj = 1/2 sum_i D_i^2 (|q_i - p'_i|^2 + 1 - |q_i|^2) + alpha sum|B| + beta/2 sum B^2,   P' = V^T B_new
// (the last line is 1/2 |D V^T (I - B A^T)|^2 + ... with A = V Qa, A^T A = I; q_i, p'_i are rows of Qa, P').
//   spca_update_kernel   the streaming pass: the new rows of B and the per-workgroup partials of P', sum|B|, sum B^2;
//   spca_sum_kernel      the fixed-order sum of per-workgroup partials (one workgroup per entry);
//   spca_step_kernel     one workgroup: the objective and the convergence test, then M = D^2 P, its polar factor by
//                        one-sided (Hestenes) Jacobi in LDS, and W;
//   spca_gram_kernel     per-workgroup partials of X^T Y over rows (setup, the general and the robust routes),
//   spca_rowmul_kernel   Y = X M row by row (X [rows x a], M [a x b] small),
//   spca_prox_kernel     out = prox(X + s Y, kappa) elementwise (the general and the robust routes).
// Float64 throughout, no atomics, every sum in a fixed order: two runs are equal bit for bit.  gfx950 only.
#pragma once
#include "eofx.h"
#include "eofx_kernels.hpp"

namespace eofx {

constexpr int SPCA_KMAX = 64;       // modes of the kernel route
constexpr int SPCA_LMAX = 128;      // columns of V (k + oversample, or min(n, p) on the exact route)
constexpr int SPCA_R = 32;          // rows of V and B staged per chunk in spca_update_kernel
constexpr int SPCA_ACC = SPCA_LMAX * SPCA_KMAX / 256;   // entries of P' per thread
constexpr int SPCA_GRAM_E = 8;      // entries of X^T Y per thread of spca_gram_kernel

// ctl[] of the loop state (device, int): finished flag, iterations completed
constexpr int SPCA_CTL_DONE = 0, SPCA_CTL_ITERS = 1;

__device__ __forceinline__ double spca_prox(double x, int reg, double kappa) {
  if (reg == EOFX_SPCA_L0) return x * x < 2.0 * kappa ? 0.0 : x;   // soft_l0: zero where x^2 < 2 kappa
  const double a = fabs(x) - kappa;                                  // soft_l1: sign(x) max(|x| - kappa, 0)
  return a > 0.0 ? copysign(a, x) : 0.0;
}

// rows [g per, (g + 1) per) of the `rows` rows belong to workgroup g
__device__ __forceinline__ void spca_rows(int64_t rows, int64_t& r0, int64_t& r1) {
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  r0 = min(rows, (int64_t)blockIdx.x * per);
  r1 = min(rows, r0 + per);
}

// grid G (<= SPCA_GMAX), block 256, dynamic LDS (l k + SPCA_R (l + k) + 512) doubles.
// apply = 0: B is not changed (the partials of the start B); apply = 1: b_j <- prox(b_j + nu (v_j W - beta b_j), kappa).
// part [(l k + 2) x G] (entry-major): over the workgroup's rows (ascending) the sums of v_j^T b_j, then of |b| and b^2
// (the last two through a fixed tree over the threads).
__global__ __launch_bounds__(256) void spca_update_kernel(const double* __restrict__ V, int64_t p, int l, int k,
                                                          double* __restrict__ B, const double* __restrict__ W, double nu,
                                                          double beta, double kappa, int reg, int apply,
                                                          const int* __restrict__ ctl, double* __restrict__ part) {
  if (ctl[SPCA_CTL_DONE]) return;                       // finished: the state stays that of the stopping iteration
  extern __shared__ double spca_lds[];
  double* Ws = spca_lds;                                // [l x k]
  double* Vs = Ws + l * k;                              // [SPCA_R x l]
  double* Bs = Vs + SPCA_R * l;                         // [SPCA_R x k]
  double* red = Bs + SPCA_R * k;                        // [2 x 256]
  const int tid = threadIdx.x, lk = l * k;
  const int64_t G = gridDim.x;
  if (apply)
    for (int e = tid; e < lk; e += 256) Ws[e] = W[e];
  double acc[SPCA_ACC];
#pragma unroll
  for (int i = 0; i < SPCA_ACC; ++i) acc[i] = 0.0;
  double s1 = 0.0, s2 = 0.0;
  int64_t r0, r1;
  spca_rows(p, r0, r1);
  __syncthreads();
  for (int64_t c0 = r0; c0 < r1; c0 += SPCA_R) {
    const int rc = (int)min((int64_t)SPCA_R, r1 - c0);
    for (int e = tid; e < rc * l; e += 256) Vs[e] = V[c0 * l + e];
    __syncthreads();
    for (int e = tid; e < rc * k; e += 256) {
      const int r = e / k, c = e % k;
      double b = B[c0 * k + e];
      if (apply) {
        double s = 0.0;
        for (int a = 0; a < l; ++a) s += Vs[r * l + a] * Ws[a * k + c];
        b = spca_prox(b + nu * (s - beta * b), reg, kappa);
        B[c0 * k + e] = b;
      }
      Bs[e] = b;
      s1 += fabs(b);
      s2 += b * b;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SPCA_ACC; ++i) {
      const int e = i * 256 + tid;
      if (e < lk) {
        const int a = e / k, c = e % k;
        double s = acc[i];
        for (int r = 0; r < rc; ++r) s += Vs[r * l + a] * Bs[r * k + c];
        acc[i] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < SPCA_ACC; ++i) {
    const int e = i * 256 + tid;
    if (e < lk) part[(int64_t)e * G + blockIdx.x] = acc[i];
  }
  red[tid] = s1;
  red[256 + tid] = s2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[256 + tid] += red[256 + tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[(int64_t)lk * G + blockIdx.x] = red[0];
    part[(int64_t)(lk + 1) * G + blockIdx.x] = red[256];
  }
}

// grid = count, block 256: out[e] = sum over g < G of part[e G + g]; thread t sums g = t, t + 256, ... in order, then a
// fixed tree over the threads.  ctl may be null.
__global__ __launch_bounds__(256) void spca_sum_kernel(const double* __restrict__ part, int G, const int* __restrict__ ctl,
                                                       double* __restrict__ out) {
  if (ctl && ctl[SPCA_CTL_DONE]) return;
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const double* src = part + (int64_t)blockIdx.x * G;
  double s = 0.0;
  for (int g = tid; g < G; g += 256) s += src[g];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = red[0];
}

// a strict total order: descending, ties by index
__device__ __forceinline__ bool spca_before(double x, int i, double y, int j) { return x != y ? x > y : i < j; }

// One workgroup.  st: [P (l k) | sum|B| | sum B^2 | Qa (l k) | W (l k) | dtilde (k) | obj (max_iter)], P = V^T B after t
// updates (spca_sum_kernel).  Call t > 0: obj[t - 1] = the objective of iteration t - 1; the loop ends (ctl DONE, ITERS = t)
// when t == max_iter or, with check, when t - 1 > 0 and |obj[t - 2] - obj[t - 1]| / obj[t - 1] < tol -- Qa and dtilde
// then stay those of iteration t - 1.  Otherwise Qa = the polar factor of M = D^2 P, dtilde its singular values
// (descending) and W = D^2 (Qa - P).  Columns of M of numerically zero norm get the deterministic orthonormal completion:
// in descending order, the first unit vectors e_m not in the span of the columns already there.
__global__ __launch_bounds__(256) void spca_step_kernel(const double* __restrict__ D2, int l, int k, double alpha, double beta,
                                                        int t, int max_iter, int check, double tol, double* __restrict__ st,
                                                        int* __restrict__ ctl) {
  if (ctl[SPCA_CTL_DONE]) return;
  __shared__ double M[SPCA_LMAX * SPCA_KMAX];         // column c at M[c l ...]
  __shared__ double J[SPCA_KMAX * SPCA_KMAX];         // column c at J[c k ...]
  __shared__ double red[256];
  __shared__ double cs[SPCA_KMAX / 2], sn[SPCA_KMAX / 2], sig[SPCA_KMAX];
  __shared__ int pp[SPCA_KMAX / 2], qq[SPCA_KMAX / 2], order[SPCA_KMAX], rot;
  const int tid = threadIdx.x, lk = l * k;
  const double* P = st;
  const double s1 = st[lk], s2 = st[lk + 1];
  double* Qa = st + lk + 2;
  double* W = Qa + lk;
  double* dt = W + lk;
  double* obj = dt + k;
  if (t > 0) {
    double r = 0.0;
    for (int a = tid; a < l; a += 256) {
      double dq = 0.0, q2 = 0.0;
      for (int c = 0; c < k; ++c) {
        const double q = Qa[a * k + c], d = q - P[a * k + c];
        dq += d * d;
        q2 += q * q;
      }
      r += D2[a] * (dq + (1.0 - q2));
    }
    red[tid] = r;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    const double o = 0.5 * red[0] + alpha * s1 + 0.5 * beta * s2;
    bool done = t >= max_iter;
    if (check && t - 1 > 0 && fabs(obj[t - 2] - o) / o < tol) done = true;
    __syncthreads();
    if (tid == 0) {
      obj[t - 1] = o;
      ctl[SPCA_CTL_ITERS] = t;
      if (done) ctl[SPCA_CTL_DONE] = 1;
    }
    if (done) return;
  }
  // M = D^2 P (by columns), J = I
  for (int e = tid; e < lk; e += 256) {
    const int a = e / k, c = e % k;
    M[c * l + a] = D2[a] * P[e];
  }
  for (int e = tid; e < k * k; e += 256) J[e] = (e / k == e % k) ? 1.0 : 0.0;
  __syncthreads();
  // one-sided Jacobi: round-robin pairs of columns (Brent & Luk), a sweep is m - 1 rounds of disjoint rotations
  const int m = k + (k & 1), half = m / 2;
  const double eps = 2.220446049250313e-16 * (double)l;
  for (int sweep = 0; sweep < 60 && m > 1; ++sweep) {
    if (tid == 0) rot = 0;
    __syncthreads();
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
        const int Pc = min(i1, i2), Qc = max(i1, i2);
        double c = 1.0, s = 0.0;
        if (Qc < k) {
          double a = 0.0, b = 0.0, g = 0.0;
          for (int r = 0; r < l; ++r) {
            const double x = M[Pc * l + r], y = M[Qc * l + r];
            a += x * x;
            b += y * y;
            g += x * y;
          }
          if (g != 0.0 && fabs(g) > eps * sqrt(a * b)) {
            const double zeta = (b - a) / (2.0 * g);
            const double tt = fabs(zeta) > 1e150 ? 0.5 / zeta
                                                 : (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            c = 1.0 / sqrt(1.0 + tt * tt);
            s = tt * c;
            rot = 1;
          }
        }
        pp[tid] = Pc;
        qq[tid] = Qc;
        cs[tid] = c;
        sn[tid] = s;
      }
      __syncthreads();
      const int len = l + k;
      for (int e = tid; e < half * len; e += 256) {       // columns Pc, Qc of M (rows < l) and of J
        const int kk = e / len, r = e % len, Pc = pp[kk], Qc = qq[kk];
        if (Qc < k && sn[kk] != 0.0) {
          const double c = cs[kk], s = sn[kk];
          double* X = r < l ? M : J;
          const int ld = r < l ? l : k, rr = r < l ? r : r - l;
          const double x = X[Pc * ld + rr], y = X[Qc * ld + rr];
          X[Pc * ld + rr] = c * x - s * y;
          X[Qc * ld + rr] = s * x + c * y;
        }
      }
      __syncthreads();
    }
    const bool any = rot != 0;
    __syncthreads();
    if (!any) break;
  }
  if (tid < k) {
    double s = 0.0;
    for (int r = 0; r < l; ++r) s += M[tid * l + r] * M[tid * l + r];
    sig[tid] = sqrt(s);
  }
  __syncthreads();
  if (tid < k) {
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += spca_before(sig[j], j, sig[tid], tid) ? 1 : 0;
    order[rank] = tid;
  }
  __syncthreads();
  const double smax = sig[order[0]];
  if (tid < k) dt[tid] = sig[order[tid]];
  // U = the normalised columns; numerically zero ones are completed below (thread 0)
  for (int e = tid; e < lk; e += 256) {
    const int c = e / l, r = e % l;
    const double s = sig[c];
    M[c * l + r] = (s > 0.0 && s > smax * eps) ? M[c * l + r] / s : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    int next = 0;
    for (int o = 0; o < k; ++o) {
      const int c = order[o];
      if (sig[c] > 0.0 && sig[c] > smax * eps) continue;
      double* u = &M[c * l];
      while (next < l) {
        for (int r = 0; r < l; ++r) u[r] = r == next ? 1.0 : 0.0;
        ++next;
        for (int pass = 0; pass < 2; ++pass) {
          for (int o2 = 0; o2 < k; ++o2) {
            const int c2 = order[o2];
            const bool have = c2 != c && ((sig[c2] > 0.0 && sig[c2] > smax * eps) || o2 < o);
            if (!have) continue;
            double d = 0.0;
            for (int r = 0; r < l; ++r) d += M[c2 * l + r] * u[r];
            for (int r = 0; r < l; ++r) u[r] -= d * M[c2 * l + r];
          }
        }
        double nn = 0.0;
        for (int r = 0; r < l; ++r) nn += u[r] * u[r];
        nn = sqrt(nn);
        if (nn > 0.5) {
          for (int r = 0; r < l; ++r) u[r] /= nn;
          break;
        }
      }
    }
  }
  __syncthreads();
  // Qa = U J^T, W = D^2 (Qa - P)
  for (int e = tid; e < lk; e += 256) {
    const int a = e / k, c = e % k;
    double q = 0.0;
    for (int i = 0; i < k; ++i) q += M[i * l + a] * J[i * k + c];
    Qa[e] = q;
    W[e] = D2[a] * (q - P[e]);
  }
}

// grid (G, ceil(a b / (256 SPCA_GRAM_E))), block 256: part[e G + g] = sum over the rows of workgroup g (ascending) of
// X[r][i] Y[r][j], e = i b + j.  A row stride of 0 repeats one row (Y = a row of ones: column sums of X).
__global__ __launch_bounds__(256) void spca_gram_kernel(const double* __restrict__ X, int64_t ldx, int a,
                                                        const double* __restrict__ Y, int64_t ldy, int b, int64_t rows,
                                                        double* __restrict__ part) {
  const int64_t ab = (int64_t)a * b, G = gridDim.x;
  int64_t r0, r1;
  spca_rows(rows, r0, r1);
  double acc[SPCA_GRAM_E];
  int ei[SPCA_GRAM_E], ej[SPCA_GRAM_E];
#pragma unroll
  for (int u = 0; u < SPCA_GRAM_E; ++u) {
    const int64_t e = ((int64_t)blockIdx.y * SPCA_GRAM_E + u) * 256 + threadIdx.x;
    acc[u] = 0.0;
    ei[u] = e < ab ? (int)(e / b) : -1;
    ej[u] = e < ab ? (int)(e % b) : 0;
  }
  for (int64_t r = r0; r < r1; ++r) {
    const double* xr = X + r * ldx;
    const double* yr = Y + r * ldy;
#pragma unroll
    for (int u = 0; u < SPCA_GRAM_E; ++u)
      if (ei[u] >= 0) acc[u] += xr[ei[u]] * yr[ej[u]];
  }
#pragma unroll
  for (int u = 0; u < SPCA_GRAM_E; ++u)
    if (ei[u] >= 0) part[((int64_t)ei[u] * b + ej[u]) * G + blockIdx.x] = acc[u];
}

// Y [rows x b] (row stride ldy) = X [rows x a] (row stride ldx) M [a x b]; one thread per output entry
__global__ __launch_bounds__(256) void spca_rowmul_kernel(const double* __restrict__ X, int64_t ldx, int a,
                                                          const double* __restrict__ Mx, int b, int64_t rows,
                                                          double* __restrict__ Y, int64_t ldy) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * b) return;
  const int64_t r = e / b;
  const int c = (int)(e % b);
  const double* xr = X + r * ldx;
  double s = 0.0;
  for (int i = 0; i < a; ++i) s += xr[i] * Mx[(int64_t)i * b + c];
  Y[r * ldy + c] = s;
}

// out[e] = prox(X[e] + s Y[e], kappa) (Y null: prox(X[e]))
__global__ __launch_bounds__(256) void spca_prox_kernel(const double* __restrict__ X, const double* __restrict__ Y, double s,
                                                        int64_t count, int reg, double kappa, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  out[e] = spca_prox(Y ? X[e] + s * Y[e] : X[e], reg, kappa);
}

}  // namespace eofx
