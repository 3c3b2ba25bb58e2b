// eofx_hilbert_host.hpp -- the host setup of the Hilbert stage (hilbert_transform.py:40-114): the impulse response of the filter,
// the circular length, the filter tables of the device routes in the order their kernels read them, the correction vectors of the
// padded transform and the whole stage as one n x n operator.  Float64 on the host, plain C++17, no HIP
// (tests/test_hilbert_host_cpu.py).  eofx_abi.hip keeps the uploads, the hipFFT plans and the caches.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <thread>
#include <vector>

namespace hfft {
// Frequency held by LDS position pos after the forward stages (host side: order of the filter table)
inline int64_t position_frequency(int L, int64_t pos) {
  const int rl_bits = L & 3;
  int64_t k = 0, weight = 1, span = (int64_t)1 << L;
  if (rl_bits) {
    span >>= rl_bits;
    k += (pos / span) * weight;
    pos %= span;
    weight <<= rl_bits;
  }
  while (span > 1) {
    span >>= 4;
    k += (pos / span) * weight;
    pos %= span;
    weight <<= 4;
  }
  return k;
}
}  // namespace hfft

namespace eofx {

// impulse response of Im(analytic-signal filter) of period N at integer lag d (0 at d = 0 mod N):
// N even: (2/N) cot(pi d/N) for odd d, 0 for even d;  N odd: (cot(pi d/N) - (-1)^d / sin(pi d/N)) / N
inline double hilbert_kappa(int64_t N, int64_t d) {
  int64_t m = d % N;
  if (m < 0) m += N;
  if (m == 0) return 0.0;
  const double x = M_PI * (double)d / (double)N;
  if (N % 2 == 0) return (m % 2) ? (2.0 / (double)N) / std::tan(x) : 0.0;
  const double sgn = (std::llabs(d) % 2) ? -1.0 : 1.0;
  return (1.0 / std::tan(x) - sgn / std::sin(x)) / (double)N;
}

// forward transform of a power-of-two length, float64, in place (host; filter table of the one-kernel Hilbert route)
inline void host_fft_f64(std::vector<std::complex<double>>& a) {
  const size_t N = a.size();
  for (size_t i = 1, j = 0; i < N; ++i) {
    size_t bit = N >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= N; len <<= 1) {
    std::vector<std::complex<double>> w(len / 2);
    for (size_t k = 0; k < len / 2; ++k) {
      const double ang = -2.0 * M_PI * (double)k / (double)len;
      w[k] = std::complex<double>(std::cos(ang), std::sin(ang));
    }
    for (size_t i = 0; i < N; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const std::complex<double> x = a[i + k], y = a[i + k + len / 2] * w[k];
        a[i + k] = x + y;
        a[i + k + len / 2] = x - y;
      }
  }
}

// circular length of the convolution behind the Hilbert stage: power of two >= 2 n, and >= 1024 so that half of it
// covers the padded series length (n_pad = round_up(n, 512) <= P / 2: the one-kernel route writes samples [0, P / 2));
// that route (eofx_hfft.hpp) holds 2^14 complex points in LDS: circular lengths up to 2^15
inline int64_t hilbert_length(int64_t n, int* log2_out) {
  int L = 10;
  while (((int64_t)1 << L) < 2 * n) ++L;
  if (log2_out) *log2_out = L;
  return (int64_t)1 << L;
}
constexpr int HFFT_MAX_LOG2 = 15;   // 2^14 complex points in LDS: two features up to P = 2^14, one feature (even / odd samples) at P = 2^15

// The four correction vectors of the padded transform, float64 [4][n] (threaded):
// u1 = K_pre e_rev, u2 = K_pos e, u3 = (K_pre + K_pos) 1, u4 = K_pre (t - n) + K_pos (t + n)
// with K_pre[t][s] = kappa((n + t) - s), K_pos[t][s] = kappa((n + t) - (2n + s)), e[t] = exp(-t / n / decay)
inline void hilbert_pad_vectors(int64_t n, int64_t N, double decay, std::vector<double>& u) {
  std::vector<double> e((size_t)n), kap((size_t)(4 * n + 1));
  for (int64_t t = 0; t < n; ++t) e[t] = std::exp(-(double)t / (double)n / decay);
  for (int64_t d = -2 * n; d <= 2 * n; ++d) kap[(size_t)(d + 2 * n)] = hilbert_kappa(N, d);
  u.assign((size_t)4 * n, 0.0);
  auto work = [&](int64_t lo, int64_t hi) {
    for (int64_t t = lo; t < hi; ++t) {
      double a1 = 0, a2 = 0, a3 = 0, a4 = 0;
      for (int64_t sidx = 0; sidx < n; ++sidx) {
        const double kp = kap[(size_t)((n + t - sidx) + 2 * n)];
        const double kq = kap[(size_t)((t - n - sidx) + 2 * n)];
        a1 += kp * e[n - 1 - sidx];
        a2 += kq * e[sidx];
        a3 += kp + kq;
        a4 += kp * (double)(sidx - n) + kq * (double)(sidx + n);
      }
      u[(size_t)t] = a1; u[(size_t)(n + t)] = a2; u[(size_t)(2 * n + t)] = a3; u[(size_t)(3 * n + t)] = a4;
    }
  };
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(16, n / 256));
  std::vector<std::thread> th;
  const int64_t step = (n + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) th.emplace_back(work, t * step, std::min<int64_t>(n, (t + 1) * step));
  for (auto& t : th) t.join();
}

// Filter table of the one-kernel route (eofx_hfft.hpp) for series length n, kernel period N and circular length P = 2^L: the kernel
// is real and odd, so its spectrum is i h[k] with h real: one float per frequency, stored in the order the forward stages leave
// the spectrum in LDS; 1/P of the unnormalised inverse folded in.
//   L <= 14: hp[pos] = h[position_frequency(L, pos)]
//   L = 15:  one feature per workgroup through the half-length transform (M = P/2 positions): the two tables of the
//            split-filter-merge step, hp[pos] = hm = h[k] - h[M-k] and hp[M + pos] = hp2 = (h[k] + h[M-k]) / 2  (h[M] = 0),
//            k = position_frequency(L - 1, pos)
inline std::vector<float> hilbert_fused_table(int64_t n, int64_t N, int L) {
  const int64_t P = (int64_t)1 << L;
  std::vector<std::complex<double>> c((size_t)P, 0.0);
  for (int64_t d = -(n - 1); d <= n - 1; ++d) c[(size_t)((d % P + P) % P)] = hilbert_kappa(N, d) / (double)P;
  host_fft_f64(c);
  std::vector<float> hp((size_t)P);
  if (L <= 14) {
    for (int64_t pos = 0; pos < P; ++pos) hp[(size_t)pos] = (float)c[(size_t)hfft::position_frequency(L, pos)].imag();
  } else {
    const int64_t M = P / 2;
    for (int64_t pos = 0; pos < M; ++pos) {
      const int64_t k = hfft::position_frequency(L - 1, pos);
      const double hk = c[(size_t)k].imag(), hkp = k ? c[(size_t)(M - k)].imag() : 0.0;
      hp[(size_t)pos] = (float)(hk - hkp);
      hp[(size_t)(M + pos)] = (float)(0.5 * (hk + hkp));
    }
  }
  return hp;
}
// hipFFT route: circular embedding of the Toeplitz kernel, lags -(n-1) .. n-1, scaled by 1/P (unnormalised inverse); P + 2 floats
inline std::vector<float> hilbert_circular_kernel(int64_t n, int64_t N, int64_t P) {
  std::vector<float> c((size_t)(P + 2), 0.f);
  for (int64_t d = -(n - 1); d <= n - 1; ++d) c[(size_t)((d % P + P) % P)] = (float)(hilbert_kappa(N, d) / (double)P);
  return c;
}
// The correction vectors as the device routes read them, float32 [4 n + 4]: [4][n] (hipFFT route), or interleaved per sample
// [n][4] followed by the four means over the samples of the (float32-rounded) vectors -- the one-kernel route adds
// coefficient * mean to the output's mean
inline std::vector<float> hilbert_pad_table(int64_t n, int64_t N, double decay, bool interleaved) {
  std::vector<double> ud;
  hilbert_pad_vectors(n, N, decay, ud);
  std::vector<float> hu((size_t)4 * n + 4, 0.f);
  for (int64_t t = 0; t < n; ++t)
    for (int k = 0; k < 4; ++k) hu[(size_t)(interleaved ? 4 * t + k : k * n + t)] = (float)ud[(size_t)k * n + t];
  if (interleaved)
    for (int k = 0; k < 4; ++k) {
      double m = 0.0;
      for (int64_t t = 0; t < n; ++t) m += (double)hu[(size_t)(4 * t + k)];
      hu[(size_t)(4 * n + k)] = (float)(m / (double)n);
    }
  return hu;
}

// The Hilbert stage as ONE linear map along the samples: for a series y [n] (padding "exp": linear fit, exponential pads,
// transform of the 3n-long series, middle third -- reference utils/hilbert_transform.py:47-92; no padding: the circular
// transform of the series itself), minus the mean over the samples,
//   Im = Hc y,   Hc = C (T + u1 (e_0 - a0)^T + u2 (e_{n-1} - a0 - (n-1) a1)^T + u3 a0^T + u4 a1^T),   C = I - 1 1^T / n
// with T[t][s] = kappa(N, t - s), a0^T y = c0 and a1^T y = c1 the coefficients of the linear fit, and u1..u4 the
// correction vectors of hilbert_pad_vectors.  Built in float64 on the host, held as a resident n x n matrix (both layouts)
// per (n, padding, decay): eofx_rsvd_hilbert_c64 applies it to the SAMPLE-side panels instead of materialising Im.
// Hc [n x n] row-major float32 on the host: Im = Hc A for the Hilbert stage of eofx_hilbert_f32 along the samples (built in float64)
// -> false when the host has no room for n x n floats
inline bool build_hilbert_operator_host(int64_t n, int padding, double decay, std::vector<float>& hc) {
  const int64_t N = padding ? 3 * n : n;
  std::vector<double> kap((size_t)(2 * n + 1)), pre((size_t)(2 * n + 2), 0.0);   // kappa(N, d), d = -n .. n, and its prefix sums
  for (int64_t d = -n; d <= n; ++d) kap[(size_t)(d + n)] = hilbert_kappa(N, d);
  for (size_t i = 0; i < kap.size(); ++i) pre[i + 1] = pre[i] + kap[i];
  std::vector<double> u, rowv((size_t)4 * n, 0.0), ubar(4, 0.0);
  if (padding) {
    hilbert_pad_vectors(n, N, decay, u);
    const double tbar = 0.5 * (double)(n - 1), stt = (double)n * ((double)n * (double)n - 1.0) / 12.0;
    for (int64_t sidx = 0; sidx < n; ++sidx) {
      const double a1 = n > 1 ? ((double)sidx - tbar) / stt : 0.0, a0 = 1.0 / (double)n - tbar * a1;
      rowv[(size_t)sidx] = (sidx == 0 ? 1.0 : 0.0) - a0;                                      // amp_pre = y[0] - c0
      rowv[(size_t)(n + sidx)] = (sidx == n - 1 ? 1.0 : 0.0) - a0 - (double)(n - 1) * a1;    // amp_pos = y[n-1] - fit(n-1)
      rowv[(size_t)(2 * n + sidx)] = a0;
      rowv[(size_t)(3 * n + sidx)] = a1;
    }
    for (int k = 0; k < 4; ++k) {
      double m = 0.0;
      for (int64_t t = 0; t < n; ++t) m += u[(size_t)k * n + t];
      ubar[k] = m / (double)n;
    }
  }
  try {
    hc.resize((size_t)n * n);
  } catch (const std::bad_alloc&) {
    return false;
  }
  auto work = [&](int64_t lo, int64_t hi) {
    for (int64_t t = lo; t < hi; ++t) {
      float* row = hc.data() + (size_t)t * n;
      double ut[4] = {0, 0, 0, 0};
      if (padding)
        for (int k = 0; k < 4; ++k) ut[k] = u[(size_t)k * n + t] - ubar[k];
      for (int64_t sidx = 0; sidx < n; ++sidx) {
        // column mean of T: (1/n) sum_t kappa(t - s) = (pre[n - s + n] - pre[-s + n]) / n
        const double cm = (pre[(size_t)(2 * n - sidx)] - pre[(size_t)(n - sidx)]) / (double)n;
        double v = kap[(size_t)(t - sidx + n)] - cm;
        if (padding)
          v += ut[0] * rowv[(size_t)sidx] + ut[1] * rowv[(size_t)(n + sidx)] + ut[2] * rowv[(size_t)(2 * n + sidx)] +
               ut[3] * rowv[(size_t)(3 * n + sidx)];
        row[sidx] = (float)v;
      }
    }
  };
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(16, n / 256));
  std::vector<std::thread> th;
  const int64_t step = (n + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) th.emplace_back(work, t * step, std::min<int64_t>(n, (t + 1) * step));
  for (auto& t : th) t.join();
  return true;
}

}  // namespace eofx
