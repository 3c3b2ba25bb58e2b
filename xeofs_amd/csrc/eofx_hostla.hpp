// The float64 host algebra of the SVD drivers between their GPU passes (eofx_abi.hip): Cholesky-QR factors, [Re | Im] panels (a complex panel of
// h columns is a real panel of 2 h columns), null-mode repair, the block-Krylov Rayleigh-Ritz step.  Plain C++ like eofx_hosteig.hpp; row-major.
#pragma once
#include "eofx_hosteig.hpp"

namespace hostla {
using hosteig::zdouble;
static inline double conj_of(double x) { return x; }        // (std::conj(double) is complex)
static inline zdouble conj_of(const zdouble& x) { return std::conj(x); }
static bool all_finite(const double* v, size_t n) { return std::all_of(v, v + n, [](double x) { return std::isfinite(x); }); }
// X = R^-1 for the upper triangular R (n x n; X zero on entry), column by column; columns marked in `dead` stay zero
template <class T>
static void upper_inverse(const T* R, int n, const char* dead, T* X) {
  for (int c = 0; c < n; ++c) {
    if (dead && dead[c]) continue;
    X[(size_t)c * n + c] = 1.0 / R[(size_t)c * n + c];
    for (int r = c - 1; r >= 0; --r) {
      T sum(0.0);
      for (int t = r + 1; t <= c; ++t) sum += R[(size_t)r * n + t] * X[(size_t)t * n + c];
      X[(size_t)r * n + c] = -sum / R[(size_t)r * n + r];
    }
  }
}
// Tm = R^-1 (l x l) for H = P^H P = R^H R (row stride ld, upper triangle read).  A dependent column -- pivot not above tol x its ORIGINAL
// diagonal entry (as chol_rinv_kernel) or, with dref, tolref x dref[j] -- is a zero column of Tm and keeps its coefficients in Rout.
template <class T>
static void chol_rinv(const T* H, int ld, int l, std::vector<T>& Tm, double tol, std::vector<T>* Rout = nullptr, int* n_live = nullptr, const double* dref = nullptr, double tolref = 0.0) {
  std::vector<T> A((size_t)l * l, T(0.0));
  std::vector<double> d0(l);
  std::vector<char> dead(l, 0);
  for (int r = 0; r < l; ++r) {
    d0[r] = std::real(H[(size_t)r * ld + r]);
    for (int c = r; c < l; ++c) A[(size_t)r * l + c] = H[(size_t)r * ld + c];
  }
  for (int j = 0; j < l; ++j) {
    const double d = std::real(A[(size_t)j * l + j]);
    const bool dj = !(d > tol * d0[j]) || !(d0[j] > 0.0) || (dref && !(d > tolref * dref[j]));
    dead[j] = dj;
    const double rjj = dj ? 1.0 : std::sqrt(d);
    const double piv = dj ? 0.0 : 1.0 / rjj;
    A[(size_t)j * l + j] = rjj;
    T* rowj = &A[(size_t)j * l];
    for (int c = j + 1; c < l; ++c) rowj[c] *= piv;
    for (int r = j + 1; r < l; ++r) {
      const T f = conj_of(rowj[r]);
      if (f == T(0.0)) continue;
      T* rowr = &A[(size_t)r * l];
      for (int c = r; c < l; ++c) rowr[c] -= f * rowj[c];
    }
  }
  if (Rout) *Rout = A;
  for (int j = 0; j < l && Rout; ++j)
    if (dead[j]) (*Rout)[(size_t)j * l + j] = T(0.0);
  if (n_live) *n_live = (int)std::count(dead.begin(), dead.end(), 0);
  Tm.assign((size_t)l * l, T(0.0));
  upper_inverse(A.data(), l, dead.data(), Tm.data());
}
// the layout of launch_rinv's host route: G and Rinv are L x L, only the leading l x l block is used, the rest of Rinv is zero
static void chol_rinv_padded(const double* G, int L, int l, double* Rinv, double tol) {
  std::vector<double> X;
  chol_rinv(G, L, l, X, tol);
  for (int r = 0; r < L; ++r)
    for (int c = 0; c < L; ++c) Rinv[(size_t)r * L + c] = (r < l && c < l) ? X[(size_t)r * l + c] : 0.0;
}
// spectrum w (descending) of the small-side Gram matrix after the first iteration: sigma_1 / sigma_l above PEAKED_RATIO (orth_tall_rule)?
constexpr double PEAKED_RATIO = 30.0;
static inline bool peaked_spectrum(const double* w, int l) { return !(w[l - 1] > 0.0) || std::sqrt(w[0] / w[l - 1]) > PEAKED_RATIO; }
// complex l x l block P^H Q of the real cross-Gram block g = [Pr | Pi]^T [Qr | Qi] (row stride ldc, h columns per half)
static void cplx_block(const double* g, int64_t ldc, int h, int l, std::vector<zdouble>& out) {
  out.assign((size_t)l * l, zdouble(0.0, 0.0));
  for (int i = 0; i < l; ++i)
    for (int j = 0; j < l; ++j)
      out[(size_t)i * l + j] = zdouble(g[(size_t)i * ldc + j] + g[(size_t)(h + i) * ldc + h + j], g[(size_t)i * ldc + h + j] - g[(size_t)(h + i) * ldc + j]);
}
// H <- (H + H^H) / 2, exactly Hermitian
static void hermitise(std::vector<zdouble>& H, int l) {
  for (int i = 0; i < l; ++i)
    for (int j = i; j < l; ++j) {
      const zdouble v = 0.5 * (H[(size_t)i * l + j] + std::conj(H[(size_t)j * l + i]));
      H[(size_t)i * l + j] = v;
      H[(size_t)j * l + i] = std::conj(v);
    }
}
// Hermitian l x l Gram P^H P from the real LP x LP Gram of [Pr | Pi] (h = LP / 2); false: not finite
static bool hermitian_from_real(const double* G, int LP, int l, std::vector<zdouble>& H) {
  cplx_block(G, LP, LP / 2, l, H);
  hermitise(H, l);
  return all_finite(reinterpret_cast<const double*>(H.data()), 2 * H.size());
}
// real LP x Lo matrix E with [Pr|Pi] E = [Re(P M) | Im(P M)] for M (l x mcols, row stride ldm) diag(colscale); h = LP/2, ho = Lo/2
static void embed_right(const zdouble* M, int ldm, int l, int mcols, int LP, int Lo, std::vector<double>& E, const double* colscale = nullptr) {
  const int h = LP / 2, ho = Lo / 2;
  E.assign((size_t)LP * Lo, 0.0);
  for (int i = 0; i < l; ++i)
    for (int j = 0; j < mcols; ++j) {
      const zdouble v = colscale ? M[(size_t)i * ldm + j] * colscale[j] : M[(size_t)i * ldm + j];
      E[(size_t)i * Lo + j] = v.real();
      E[(size_t)(h + i) * Lo + j] = -v.imag();
      E[(size_t)i * Lo + ho + j] = v.imag();
      E[(size_t)(h + i) * Lo + ho + j] = v.real();
    }
}
static std::vector<zdouble> zmatmul(const std::vector<zdouble>& X, const std::vector<zdouble>& Y, int l) {    // l x l
  std::vector<zdouble> Z((size_t)l * l, zdouble(0.0, 0.0));
  for (int i = 0; i < l; ++i)
    for (int t = 0; t < l; ++t) {
      const zdouble x = X[(size_t)i * l + t];
      if (x == zdouble(0.0, 0.0)) continue;
      for (int j = 0; j < l; ++j) Z[(size_t)i * l + j] += x * Y[(size_t)t * l + j];
    }
  return Z;
}
// One round of fix_null_columns' block Gram-Schmidt as a right factor: from the Gram matrix hG [Lo x Lo] of a panel whose columns
// before `first` are orthonormal, hM [Lo x Lo] = [I, -C_GN R^-1; 0, R^-1], R the Cholesky factor of S = C_NN - C_GN^T C_GN.  Otherwise
// hM is untouched and flag [Lo] marks the columns of [first, k) to replace: NULLCOL_BAD (with stop_at_bad) -- zero or not finite; NULLCOL_DEPENDENT.
enum { NULLCOL_OK = 0, NULLCOL_BAD = 1, NULLCOL_DEPENDENT = 2 };
static int null_column_transform(const double* hG, int Lo, int first, int k, bool stop_at_bad, double* hM, int* flag) {
  const int m = k - first;
  bool bad = false;
  std::fill(flag, flag + Lo, 0);
  for (int j = first; j < k; ++j) {
    const double d = hG[(size_t)j * Lo + j];
    if (!std::isfinite(d) || !(d > 1e-30)) flag[j] = 1, bad = true;
    for (int i = 0; i < k && !flag[j]; ++i)
      if (!std::isfinite(hG[(size_t)i * Lo + j])) flag[j] = 1, bad = true;
  }
  if (bad && stop_at_bad) return NULLCOL_BAD;
  std::vector<double> S((size_t)m * m), Ri((size_t)m * m, 0.0);
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) {
      double v = hG[(size_t)(first + a) * Lo + first + b];
      for (int g = 0; g < first; ++g) v -= hG[(size_t)g * Lo + first + a] * hG[(size_t)g * Lo + first + b];
      S[(size_t)a * m + b] = v;
    }
  // right-looking Cholesky with a pivot floor: a column left with < 1e-6 of its squared length lay inside the span before it
  bool dependent = false;
  std::vector<double> A(S);
  for (int j = 0; j < m; ++j) {
    const double d = A[(size_t)j * m + j];
    if (!(d > 1e-6 * std::max(S[(size_t)j * m + j], 1e-300)) || !std::isfinite(d)) {
      flag[first + j] = 1;          // (all such columns are found in one sweep: this one drops out of the factorisation)
      dependent = true;
      for (int c = j; c < m; ++c) A[(size_t)j * m + c] = 0.0;
      A[(size_t)j * m + j] = 1.0;
      continue;
    }
    const double rjj = std::sqrt(d);
    A[(size_t)j * m + j] = rjj;
    for (int c = j + 1; c < m; ++c) A[(size_t)j * m + c] /= rjj;
    for (int r = j + 1; r < m; ++r) {
      const double f = A[(size_t)j * m + r];
      for (int c = r; c < m; ++c) A[(size_t)r * m + c] -= f * A[(size_t)j * m + c];
    }
  }
  if (dependent) return NULLCOL_DEPENDENT;
  upper_inverse(A.data(), m, nullptr, Ri.data());
  std::fill(hM, hM + (size_t)Lo * Lo, 0.0);
  for (int i = 0; i < first; ++i) hM[(size_t)i * Lo + i] = 1.0;
  for (int a = 0; a < m; ++a)
    for (int b = a; b < m; ++b) hM[(size_t)(first + a) * Lo + first + b] = Ri[(size_t)a * m + b];
  for (int g = 0; g < first; ++g)
    for (int b = 0; b < m; ++b) {
      double v = 0.0;
      for (int a = 0; a <= b; ++a) v += hG[(size_t)g * Lo + first + a] * Ri[(size_t)a * m + b];
      hM[(size_t)g * Lo + first + b] = -v;
    }
  return NULLCOL_OK;
}
// The complex driver's repair of hp [small x Lo] = [Re (ko) | Im (ko)] (float32): columns [first_null, k) are re-orthonormalised against
// all before them (Gram-Schmidt, two rounds; a zero, non-finite or dependent column becomes the first unit vector that is independent).
static void null_repair_c(float* hp, int64_t small, int Lo, int ko, int first_null, int k) {
  auto col = [&](int j, std::vector<zdouble>& v) {
    v.resize((size_t)small);
    for (int64_t r = 0; r < small; ++r) v[(size_t)r] = zdouble(hp[(size_t)r * Lo + j], hp[(size_t)r * Lo + ko + j]);
  };
  std::vector<std::vector<zdouble>> basis((size_t)k);
  for (int j = 0; j < first_null; ++j) col(j, basis[(size_t)j]);
  auto project_out = [&](std::vector<zdouble>& v, int upto) {
    for (int round = 0; round < 2; ++round)
      for (int c = 0; c < upto; ++c) {
        zdouble dot(0.0, 0.0);
        for (int64_t r = 0; r < small; ++r) dot += std::conj(basis[(size_t)c][(size_t)r]) * v[(size_t)r];
        for (int64_t r = 0; r < small; ++r) v[(size_t)r] -= dot * basis[(size_t)c][(size_t)r];
      }
    double nn = 0.0;
    for (int64_t r = 0; r < small; ++r) nn += std::norm(v[(size_t)r]);
    return std::sqrt(nn);
  };
  int64_t next_unit = 0;
  for (int j = first_null; j < k; ++j) {
    std::vector<zdouble> v;
    col(j, v);
    double nn0 = 0.0;
    for (const zdouble& x : v) nn0 += std::norm(x);
    double nn = std::isfinite(nn0) && nn0 > 0.0 ? project_out(v, j) / std::sqrt(nn0) : 0.0;
    while (!(nn > 1e-3) && next_unit < small) {          // inside the span of the others (or not finite): a unit vector instead
      v.assign((size_t)small, zdouble(0.0, 0.0));
      v[(size_t)next_unit++] = zdouble(1.0, 0.0);
      nn = project_out(v, j);
      if (nn > 0.1) break;
      nn = 0.0;
    }
    double nrm = 0.0;
    for (const zdouble& x : v) nrm += std::norm(x);
    nrm = std::sqrt(nrm);
    for (int64_t r = 0; r < small; ++r) {
      const zdouble x = nrm > 0.0 ? v[(size_t)r] / nrm : zdouble(0.0, 0.0);
      v[(size_t)r] = x;
      hp[(size_t)r * Lo + j] = (float)x.real();
      hp[(size_t)r * Lo + ko + j] = (float)x.imag();
    }
    basis[(size_t)j] = v;
  }
}
// ---- block Krylov: K = [Z_0 .. Z_{nb-1}], blocks of l complex columns in [Re | Im] panels of LP real columns; M Z_i = W_i Rf[i] (empty = I)
// |W_j|^2 = |V_j|^2 + |K^H W_j|^2: the diagonal of the Gram matrix Hv of V = W - K (K^H W) plus the column norms of hC = K^T W
static void product_norms(const std::vector<zdouble>& Hv, const double* hC, int nb, int LP, int l, std::vector<double>& dref) {
  std::vector<zdouble> blk;
  dref.resize(l);
  for (int j = 0; j < l; ++j) dref[j] = Hv[(size_t)j * l + j].real();
  for (int c = 0; c < nb; ++c) {
    cplx_block(hC + (size_t)c * LP * LP, LP, LP / 2, l, blk);
    for (int i = 0; i < l; ++i)
      for (int j = 0; j < l; ++j) dref[j] += std::norm(blk[(size_t)i * l + j]);
  }
}
// H = K^H M K over the first nbr blocks (order nbr l, split real / imaginary, exactly Hermitian) from the real cross-Gram
// hCf = K[:nrow]^T W[:nWr]: raw[j nbr + i] = (K_j^H W_i) Rf[i]; Hqq (optional) replaces the last diagonal block (the newest block
// has no product yet: P^H P of its tall panel).  nrow = nbr + 1 keeps the coupling row for ritz_residual.
static void ritz_assemble(const double* hCf, int nrow, int nWr, int nbr, int LP, int l, const std::vector<std::vector<zdouble>>& Rf, const std::vector<zdouble>* Hqq,
                          std::vector<std::vector<zdouble>>& raw, std::vector<double>& Hr, std::vector<double>& Hi) {
  const int64_t ldc = (int64_t)nWr * LP;
  const int m = nbr * l;
  std::vector<zdouble> blk;
  raw.assign((size_t)nrow * nbr, std::vector<zdouble>());
  for (int i = 0; i < nWr; ++i)
    for (int j = 0; j < nrow; ++j) {
      cplx_block(hCf + (size_t)j * LP * ldc + (size_t)i * LP, ldc, LP / 2, l, blk);
      raw[(size_t)j * nbr + i] = Rf[i].empty() ? blk : zmatmul(blk, Rf[i], l);
    }
  if (Hqq) raw[(size_t)(nbr - 1) * nbr + nbr - 1] = *Hqq;
  Hr.assign((size_t)m * m, 0.0);
  Hi.assign((size_t)m * m, 0.0);
  for (int a = 0; a < nbr; ++a)
    for (int c = a; c < nbr; ++c) {
      const std::vector<zdouble>& u = raw[(size_t)a * nbr + c];     // block (a, c)
      const std::vector<zdouble>& v = raw[(size_t)c * nbr + a];     // block (c, a): its conjugate transpose is another reading of (a, c)
      if (u.empty() && v.empty()) continue;
      const double wu = u.empty() ? 0.0 : (v.empty() ? 1.0 : 0.5), wvv = v.empty() ? 0.0 : (u.empty() ? 1.0 : 0.5);
      for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j) {
          zdouble val(0.0, 0.0);
          if (!u.empty()) val += wu * u[(size_t)i * l + j];
          if (!v.empty()) val += wvv * std::conj(v[(size_t)j * l + i]);
          const size_t ij = (size_t)(a * l + i) * m + c * l + j, ji = (size_t)(c * l + j) * m + a * l + i;
          Hr[ij] = val.real();
          Hi[ij] = val.imag();
          if (a != c) {
            Hr[ji] = val.real();
            Hi[ji] = -val.imag();
          }
        }
    }
}
// res[j] = norm of the part of M K y_j outside the first nbr blocks: the coupling to block nbr (row nbr of raw; y = Xr + i Xi)
static void ritz_residual(const std::vector<std::vector<zdouble>>& raw, int nbr, int nWr, int l, const double* Xr, const double* Xi, std::vector<double>& res) {
  res.assign(l, 0.0);
  for (int j = 0; j < l; ++j) {
    double r2 = 0.0;
    for (int i2 = 0; i2 < l; ++i2) {           // row i2 of block nbr of M K y_j
      zdouble acc(0.0, 0.0);
      for (int c = 0; c < nWr; ++c) {
        const std::vector<zdouble>& cb = raw[(size_t)nbr * nbr + c];
        if (cb.empty()) continue;
        for (int t = 0; t < l; ++t) acc += cb[(size_t)i2 * l + t] * zdouble(Xr[(size_t)(c * l + t) * l + j], Xi[(size_t)(c * l + t) * l + j]);
      }
      r2 += std::norm(acc);
    }
    res[j] = std::sqrt(r2);
  }
}
// block b of the Ritz vectors y = Xr + i Xi (order nbr l x l) as a complex l x l matrix
static std::vector<zdouble> ritz_block(const double* Xr, const double* Xi, int b, int l) {
  std::vector<zdouble> yb((size_t)l * l);
  for (size_t e = 0; e < yb.size(); ++e) yb[e] = zdouble(Xr[(size_t)b * l * l + e], Xi[(size_t)b * l * l + e]);
  return yb;
}
// The "converge" rule of the block-Krylov driver (measurements: DESIGN.md): continue until every WANTED singular value is good to 2e-6
// and every gap-separated wanted vector to |cos| >= 1 - 5e-6, inside the parity tolerances (1e-5; |cos| >= 1 - 1e-5 at 2 % separation).
// The error of a Ritz value theta_j (= sigma^2) is estimated from its OWN history: Ritz values of a growing Krylov space rise monotonically
// and geometrically; with D_c the rise between two checks and rho = D_c / D_{c-1}, the distance to go is D_c rho / (1 - rho) (no ratio yet: D_c).
// A check is a host Rayleigh-Ritz solve: every third product from three before scikit-learn's count on, none once the rate says the limit comes first.
struct RitzHistory {
  static constexpr double val_tol = 4e-6, vec_tol = 1e-5, sep_rel = 0.04;
  static constexpr int check_every = 3;
  int next_check;               // the product count at which the next check is due (limit + 1: no further checks)
  double worst = 0.0;           // of the last check: largest (estimate / tolerance) over the wanted modes, <= 1 = converged
  double factor = 0.0;          // > 0 once the rate rule has fired (no further checks): worst's ratio to the check before
  double worst_prev = -1.0;
  std::vector<double> th_prev, rise_prev;
  RitzHistory(int auto_count, int it_min) : next_check(std::max(std::max(auto_count, it_min) - check_every, it_min)) {}
  // wv: the leading l Ritz values (descending) after `products` products, of which at most `limit` are made; k wanted.  true: stop
  bool feed(const double* wv, int k, int l, int products, int limit) {
    worst = th_prev.empty() ? 1e300 : 0.0;
    std::vector<double> rise(k, 0.0);
    for (int j = 0; j < k && !th_prev.empty(); ++j) {
      const double th = std::max(wv[j], 1e-300);
      rise[j] = std::fabs(wv[j] - th_prev[j]) / th;
      double rho = 0.5;                                 // no ratio yet: the rise itself is the estimate
      if (!rise_prev.empty() && rise_prev[j] > 0.0) rho = std::min(0.7, std::max(0.02, rise[j] / rise_prev[j]));
      const double est = rise[j] * rho / (1.0 - rho);
      double score = est / val_tol;
      double gap = 1e300;                               // relative gap to the nearest other Ritz value
      if (j > 0) gap = std::min(gap, (wv[j - 1] - wv[j]) / th);
      if (j + 1 < l) gap = std::min(gap, (wv[j] - wv[j + 1]) / th);
      if (gap >= sep_rel && gap < 1e300) score = std::max(score, est / gap / vec_tol);     // sin^2 of the vector's angle ~ error / gap
      worst = std::max(worst, score);
    }
    if (worst <= 1.0) return true;
    next_check = products + check_every;
    if (!rise_prev.empty() && worst_prev > 0.0 && worst < 1e299) {      // two estimates: will the limit come first?
      const double f = worst / worst_prev;                               // factor per check interval
      const double checks_needed = f < 1.0 ? std::log(worst) / std::log(1.0 / f) : 1e9;
      if ((double)products + checks_needed * check_every > (double)limit + check_every) next_check = limit + 1, factor = f;
    }
    if (!th_prev.empty()) {
      rise_prev = rise;
      worst_prev = worst;
    }
    th_prev.assign(wv, wv + k);
    return false;
  }
};
}  // namespace hostla
