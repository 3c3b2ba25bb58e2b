// eofx_lag.hpp -- the delay embedding of Extended EOF analysis (xeofs/single/eeof.py:124-150) as an operator.
//
// The embedded matrix of E lags spaced tau samples apart,
//     X_ext[t, (e, j)] = X[t + e tau, j],      t < n' = n - (E - 1) tau,  e < E,
// is never written.  Both products of the randomized SVD run on the resident field X with the lags moved onto the small
// sample-side panel (S_e = the row window [e tau, e tau + n')):
//     X_ext^T Z = X^T [S_0^T Z | ... | S_{E-1}^T Z]           lag_spread_kernel, one wide X^T W, lag_gather_kernel
//     X_ext   Y = sum_e S_e (X [Y_0 | ... | Y_{E-1}])_e       lag_relayout_kernel, one wide X Y, lag_fold_kernel
// The inner EOF centres every embedded column over its own window, so the operator carries the window means mu[e, j] as
// a rank-one correction (- mu (1^T Z) after the first product, - 1 (mu^T Y) after the second).  Feature-side panels of
// the embedded operator are lag-major: row e * p_pad + j, zero padding rows j >= p in every lag block.  All sums are
// float64 in a fixed order (no atomics): results are reproducible bit for bit.  gfx950 only.
#pragma once
#include "eofx_kernels.hpp"

namespace eofx {

// One element of the resident matrix in whichever layout it holds: 0 = feature-contiguous X [n_pad x p_pad], 1 = the
// raw field read through the Scaler's affine map (in place / raw mode), 2 = sample-contiguous X^T [p_pad x n_pad].
struct LagSrc {
  const float* a = nullptr;
  int64_t ld = 0;
  int mode = 0;
  const float* aff = nullptr;   // {shift hi, shift lo, scale}[aff_ld] (mode 1)
  int64_t aff_ld = 0;
};
__device__ __forceinline__ float lag_load(const LagSrc& s, int64_t t, int64_t j) {
  if (s.mode == 2) return s.a[j * s.ld + t];
  const float v = s.a[t * s.ld + j];
  if (s.mode == 1) {
    const float sl = s.aff[2 * s.aff_ld + j];
    return sl == 0.f ? 0.f : aff_map(v, s.aff[j], s.aff[s.aff_ld + j], sl);
  }
  return v;
}

// Window statistics in ONE read of the field: thread j walks its feature from t = 0 to n - 1 with a running float64 sum
// F(t); at the window boundaries (ev: sorted (row, lag, sign) triples, rows e tau and e tau + n') it adds +-F to the
// window sum of that lag, so  sum_{window e} x = F(e tau + n') - F(e tau).  The sum of squares over all windows is
// sum_t cnt(t) x_t^2 with cnt(t) the number of windows that hold row t.  mean[e * p_pad + j] = window mean (0 on the
// padding features), tvpart[j] = sum_e (sum_window x^2 - n' mu^2) / (n' - 1).
__global__ __launch_bounds__(256) void lag_stats_kernel(LagSrc src, int64_t n, int64_t p, int64_t p_pad, int tau, int E,
                                                        int64_t nprime, const int64_t* __restrict__ ev, int nev,
                                                        double* __restrict__ mean, double* __restrict__ tvpart) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p_pad) return;
  for (int e = 0; e < E; ++e) mean[(int64_t)e * p_pad + j] = 0.0;
  if (j >= p) {
    tvpart[j] = 0.0;
    return;
  }
  double F = 0.0, q = 0.0;
  int k = 0;
  for (int64_t t = 0; t < n; ++t) {
    for (; k < nev && ev[3 * k] == t; ++k) mean[ev[3 * k + 1] * p_pad + j] += (double)ev[3 * k + 2] * F;
    const double x = (double)lag_load(src, t, j);
    const int64_t hi = min((int64_t)(E - 1), t / tau), lo = t >= nprime ? (t - nprime + tau) / tau : 0;
    F += x;
    q += (double)(hi >= lo ? hi - lo + 1 : 0) * (x * x);
  }
  for (; k < nev; ++k) mean[ev[3 * k + 1] * p_pad + j] += (double)ev[3 * k + 2] * F;
  double m2 = 0.0;
  for (int e = 0; e < E; ++e) {
    const double mu = mean[(int64_t)e * p_pad + j] / (double)nprime;
    mean[(int64_t)e * p_pad + j] = mu;
    m2 += mu * mu;
  }
  tvpart[j] = (q - (double)nprime * m2) / (double)(nprime - 1);
}

// out[0] = sum of v[0 .. count) in a fixed order (one workgroup: strided partial sums, then a tree)
__global__ __launch_bounds__(256) void lag_sum_kernel(const double* __restrict__ v, int64_t count, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) s += v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// W[t, g L + c] = Z[t - (e0 + g) tau, c] inside the window of lag e0 + g, else 0; W is [rows_pad x Lg], Z [n' rows x L]
__global__ __launch_bounds__(256) void lag_spread_kernel(const float* __restrict__ Z, int64_t nprime, int L, int64_t rows_pad,
                                                         int Lg, int e0, int tau, float* __restrict__ W) {
  const int lg4 = Lg / 4;
  const int64_t total = rows_pad * lg4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / lg4;
    const int col = 4 * (int)(i - t * lg4);
    const int g = col / L, c = col - g * L;
    const int64_t src = t - (int64_t)(e0 + g) * tau;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (src >= 0 && src < nprime) v = *reinterpret_cast<const f32x4*>(Z + src * L + c);
    reinterpret_cast<f32x4*>(W)[i] = v;
  }
}

// Ye[(e0 + g) p_pad + j, c] = P[j, g L + c] - mu[e0 + g, j] cs[c] for j < p, 0 on the padding rows (float64 arithmetic)
__global__ __launch_bounds__(256) void lag_gather_kernel(const float* __restrict__ P, int Lg, int64_t p, int64_t p_pad, int L,
                                                         int e0, int ng, const double* __restrict__ mean,
                                                         const double* __restrict__ cs, float* __restrict__ Ye) {
  const int l4 = L / 4;
  const int64_t total = (int64_t)ng * p_pad * l4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / l4;                       // row within the group's lag blocks: g p_pad + j
    const int c = 4 * (int)(i - r * l4);
    const int g = (int)(r / p_pad);
    const int64_t j = r - (int64_t)g * p_pad;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (j < p) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(P + j * Lg + g * L + c);
      const double mu = mean[(int64_t)(e0 + g) * p_pad + j];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = (float)((double)v[q] - mu * cs[c + q]);
    }
    reinterpret_cast<f32x4*>(Ye)[((int64_t)e0 * p_pad + r) * l4 + c / 4] = o;
  }
}

// Yg[j, g L + c] = Ye[(e0 + g) p_pad + j, c]: the group's lag blocks side by side, one wide feature-side panel
__global__ __launch_bounds__(256) void lag_relayout_kernel(const float* __restrict__ Ye, int64_t p_pad, int L, int e0, int ng,
                                                           float* __restrict__ Yg) {
  const int Lg = ng * L, lg4 = Lg / 4;
  const int64_t total = p_pad * lg4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t j = i / lg4;
    const int col = 4 * (int)(i - j * lg4);
    const int g = col / L, c = col - g * L;
    reinterpret_cast<f32x4*>(Yg)[i] = *reinterpret_cast<const f32x4*>(Ye + ((int64_t)(e0 + g) * p_pad + j) * L + c);
  }
}

// part[b, c] = sum over the rows r of block b's range of w[r] P[r, c] (float64; the rows of a lag-major feature-side panel
// weighted by the window means: mu^T Y).  panel_colsum_final_kernel adds the partials in a fixed order.
__global__ __launch_bounds__(256) void lag_wcolsum_part_kernel(const float* __restrict__ P, const double* __restrict__ w,
                                                               int64_t rows, int L, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int col = threadIdx.x & 63, rq = threadIdx.x >> 6;
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
  for (int cb = 0; cb < L; cb += 64) {
    double s = 0.0;
    if (cb + col < L)
      for (int64_t r = r0 + rq; r < r1; r += 4) s += w[r] * (double)P[r * L + cb + col];
    red[rq][col] = s;
    __syncthreads();
    if (rq == 0 && cb + col < L) part[(int64_t)blockIdx.x * L + cb + col] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
    __syncthreads();
  }
}

// The shifted sum over the group's lag blocks of the wide product P = X Yg [rows_pad x Lg]:
//   s[t, c] = (first ? 0 : acc[t, c]) + sum_{g ascending} P[t + (e0 + g) tau, g L + c]      for t < n'
// kept in the float64 accumulator between groups; the last group writes Wn[t, c] = s - cs[c] (0 for n' <= t < n'_pad).
__global__ __launch_bounds__(256) void lag_fold_kernel(const float* __restrict__ P, int Lg, int L, int e0, int ng, int tau,
                                                       int64_t nprime, int64_t nprime_pad, double* __restrict__ acc, int first,
                                                       int last, const double* __restrict__ cs, float* __restrict__ Wn) {
  const int l4 = L / 4;
  const int64_t total = nprime_pad * l4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / l4;
    const int c = 4 * (int)(i - t * l4);
    if (t >= nprime) {
      if (last) reinterpret_cast<f32x4*>(Wn)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    double s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = first ? 0.0 : acc[t * L + c + q];
    for (int g = 0; g < ng; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(P + (t + (int64_t)(e0 + g) * tau) * Lg + g * L + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += (double)v[q];
    }
    if (last) {
      f32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = (float)(s[q] - cs[c + q]);
      reinterpret_cast<f32x4*>(Wn)[i] = o;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[t * L + c + q] = s[q];
    }
  }
}

// out[t, e p + j] = X[t + e tau, j] for t < n' (the embedded matrix, row-major n' x E p, not centred)
__global__ __launch_bounds__(256) void lag_embed_kernel(LagSrc src, int64_t p, int E, int tau, int64_t nprime,
                                                        float* __restrict__ out) {
  const int64_t width = (int64_t)E * p, total = nprime * width;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / width, r = i - t * width;
    const int64_t e = r / p, j = r - e * p;
    out[i] = lag_load(src, t + e * tau, j);
  }
}

}  // namespace eofx
