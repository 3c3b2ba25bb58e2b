// extern "C" wrappers around the header-only host algebra (xeofs_amd/csrc/eofx_hostla.hpp, eofx_hosteig.hpp) for
// tests/test_hostla_cpu.py, which compiles this file with the host C++ compiler and loads it through ctypes.  Complex
// arrays are interleaved (re, im) doubles, i.e. numpy's complex128.  With -DHOSTLA_SELFTEST the file is a stand-alone
// program that runs every wrapper on fixed inputs (for a sanitizer build: c++ -fsanitize=address,undefined).
#include <cstdio>
#include <cstring>

#include "eofx_hostla.hpp"

using hostla::zdouble;

namespace {
template <class T>
int chol_rinv_any(const T* H, int ld, int l, T* Tm, double tol, T* Rout, int* n_live, const double* dref, double tolref) {
  std::vector<T> t, r;
  int live = 0;
  hostla::chol_rinv(H, ld, l, t, tol, Rout ? &r : nullptr, &live, dref, tolref);
  std::copy(t.begin(), t.end(), Tm);
  if (Rout) std::copy(r.begin(), r.end(), Rout);
  if (n_live) *n_live = live;
  return live;
}
typedef std::vector<std::vector<zdouble>> zblocks;
zblocks rf_blocks(const zdouble* Rf, const int* has_rf, int nb, int l) {
  zblocks out(nb);
  for (int b = 0; b < nb; ++b)
    if (has_rf[b]) out[b].assign(Rf + (size_t)b * l * l, Rf + (size_t)(b + 1) * l * l);
  return out;
}
}  // namespace

extern "C" {
int hl_chol_rinv_d(const double* H, int ld, int l, double* Tm, double tol, double* Rout, int* n_live, const double* dref, double tolref) {
  return chol_rinv_any(H, ld, l, Tm, tol, Rout, n_live, dref, tolref);
}
int hl_chol_rinv_z(const zdouble* H, int ld, int l, zdouble* Tm, double tol, zdouble* Rout, int* n_live, const double* dref, double tolref) {
  return chol_rinv_any(H, ld, l, Tm, tol, Rout, n_live, dref, tolref);
}
void hl_chol_rinv_padded(const double* G, int L, int l, double* Rinv, double tol) { hostla::chol_rinv_padded(G, L, l, Rinv, tol); }
int hl_eigh(const double* A, int n, double* w, double* V) { return hosteig::eigh(A, n, w, V); }
int hl_heigh(const zdouble* H, int l, double* w, zdouble* V) {
  std::vector<zdouble> h(H, H + (size_t)l * l), v;
  std::vector<double> ww;
  const int rc = hosteig::heigh(h, l, ww, v);
  if (rc != 0) return rc;
  std::copy(ww.begin(), ww.end(), w);
  std::copy(v.begin(), v.end(), V);
  return 0;
}
int hl_zheigh_top_embedded(const double* Hr, const double* Hi, int m, int nev, double* w, double* Xr, double* Xi) {
  return hosteig::zheigh_top_embedded(Hr, Hi, m, nev, w, Xr, Xi);
}
int hl_peaked_spectrum(const double* w, int l) { return hostla::peaked_spectrum(w, l) ? 1 : 0; }
int hl_hermitian_from_real(const double* G, int LP, int l, zdouble* H) {
  std::vector<zdouble> h;
  const bool finite = hostla::hermitian_from_real(G, LP, l, h);
  std::copy(h.begin(), h.end(), H);
  return finite ? 1 : 0;
}
void hl_embed_right(const zdouble* M, int ldm, int l, int mcols, int LP, int Lo, double* E, const double* colscale) {
  std::vector<double> e;
  hostla::embed_right(M, ldm, l, mcols, LP, Lo, e, colscale);
  std::copy(e.begin(), e.end(), E);
}
void hl_zmatmul(const zdouble* X, const zdouble* Y, int l, zdouble* Z) {
  const std::vector<zdouble> z = hostla::zmatmul(std::vector<zdouble>(X, X + (size_t)l * l), std::vector<zdouble>(Y, Y + (size_t)l * l), l);
  std::copy(z.begin(), z.end(), Z);
}
int hl_null_column_transform(const double* hG, int Lo, int first, int k, int stop_at_bad, double* hM, int* flag) {
  return hostla::null_column_transform(hG, Lo, first, k, stop_at_bad != 0, hM, flag);
}
void hl_null_repair_c(float* hp, int64_t small, int Lo, int ko, int first_null, int k) { hostla::null_repair_c(hp, small, Lo, ko, first_null, k); }
void hl_product_norms(const zdouble* Hv, const double* hC, int nb, int LP, int l, double* dref) {
  std::vector<double> d;
  hostla::product_norms(std::vector<zdouble>(Hv, Hv + (size_t)l * l), hC, nb, LP, l, d);
  std::copy(d.begin(), d.end(), dref);
}
// Rf: nWr blocks of l x l (has_rf[b] = 0: identity); Hqq: nullptr or l x l; res: nullptr, or [l] with Xr / Xi [nbr l x l]
void hl_ritz(const double* hCf, int nrow, int nWr, int nbr, int LP, int l, const zdouble* Rf, const int* has_rf, const zdouble* Hqq,
             double* Hr, double* Hi, const double* Xr, const double* Xi, double* res) {
  zblocks rf = rf_blocks(Rf, has_rf, nWr, l), raw;
  std::vector<zdouble> hqq;
  if (Hqq) hqq.assign(Hqq, Hqq + (size_t)l * l);
  std::vector<double> hr, hi, r;
  hostla::ritz_assemble(hCf, nrow, nWr, nbr, LP, l, rf, Hqq ? &hqq : nullptr, raw, hr, hi);
  std::copy(hr.begin(), hr.end(), Hr);
  std::copy(hi.begin(), hi.end(), Hi);
  if (res && nrow > nbr) {
    hostla::ritz_residual(raw, nbr, nWr, l, Xr, Xi, r);
    std::copy(r.begin(), r.end(), res);
  }
}
void hl_ritz_block(const double* Xr, const double* Xi, int b, int l, zdouble* out) {
  const std::vector<zdouble> yb = hostla::ritz_block(Xr, Xi, b, l);
  std::copy(yb.begin(), yb.end(), out);
}
// feeds `checks` rows of l Ritz values, one per check, check c after products[c]; -> "stop" and next_check after each, the last factor
double hl_ritz_history(const double* wv, const int* products, int checks, int k, int l, int auto_count, int it_min, int limit, int* verdicts,
                       int* next_checks) {
  hostla::RitzHistory hist(auto_count, it_min);
  for (int c = 0; c < checks; ++c) {
    verdicts[c] = hist.feed(wv + (size_t)c * l, k, l, products[c], limit) ? 1 : 0;
    next_checks[c] = hist.next_check;
  }
  return hist.factor;
}
}

#ifdef HOSTLA_SELFTEST
namespace {
uint64_t lcg_state = 0x2545F4914F6CDD1Dull;
double lcg() {      // uniform in [-1, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((lcg_state >> 11) & 0xFFFFFFFFull) / 2147483648.0 - 1.0;
}
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    std::fprintf(stderr, "hostla selftest: FAILED %s\n", what);
  }
}
// Gram matrix P^H P of a random rows x l panel; dep >= 0: column dep = column 0 + column 1; zero >= 0: a zero column
template <class T>
T draw();
template <>
double draw<double>() { return lcg(); }
template <>
zdouble draw<zdouble>() { return zdouble(lcg(), lcg()); }
template <class T>
std::vector<T> gram(int rows, int l, int dep, int zero) {
  std::vector<T> P((size_t)rows * l), H((size_t)l * l, T(0.0));
  for (auto& x : P) x = draw<T>();
  for (int r = 0; r < rows; ++r) {
    if (dep >= 0) P[(size_t)r * l + dep] = P[(size_t)r * l] + P[(size_t)r * l + 1];
    if (zero >= 0) P[(size_t)r * l + zero] = T(0.0);
  }
  for (int r = 0; r < rows; ++r)
    for (int i = 0; i < l; ++i)
      for (int j = 0; j < l; ++j) H[(size_t)i * l + j] += hostla::conj_of(P[(size_t)r * l + i]) * P[(size_t)r * l + j];
  return H;
}
template <class T, class F>
void chol_cases(F fn, const char* name) {
  for (int l : {1, 2, 7, 64, 100})
    for (int deadcase = 0; deadcase < (l >= 7 ? 2 : 1); ++deadcase) {
      const std::vector<T> H = gram<T>(4 * l, l, deadcase ? 5 : -1, deadcase ? 3 : -1);
      std::vector<T> Tm((size_t)l * l), R((size_t)l * l);
      std::vector<double> dref(l, 1e30);
      int live = -1;
      fn(H.data(), l, l, Tm.data(), 1e-13, R.data(), &live, nullptr, 0.0);
      expect(live == (deadcase ? l - 2 : l), name);
      fn(H.data(), l, l, Tm.data(), 1e-13, nullptr, &live, dref.data(), 1e-10);
      expect(live == 0, "chol_rinv dref rule");
    }
}
}  // namespace

int main() {
  chol_cases<double>(hl_chol_rinv_d, "chol_rinv<double> live count");
  chol_cases<zdouble>(hl_chol_rinv_z, "chol_rinv<complex> live count");
  {
    const int l = 100, L = 128;
    std::vector<double> H = gram<double>(4 * l, l, 77, -1), G((size_t)L * L, 0.0), R((size_t)L * L, 1.0);
    for (int i = 0; i < l; ++i)
      for (int j = 0; j < l; ++j) G[(size_t)i * L + j] = H[(size_t)i * l + j];
    hl_chol_rinv_padded(G.data(), L, l, R.data(), 1e-13);
    bool zero = true;
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j)
        if ((i >= l || j >= l || j < i || j == 77) && R[(size_t)i * L + j] != 0.0) zero = false;
    expect(zero, "chol_rinv_padded structure");
  }
  for (int l : {1, 2, 7, 64}) {
    const std::vector<zdouble> H = gram<zdouble>(3 * l, l, -1, -1);
    std::vector<zdouble> V((size_t)l * l);
    std::vector<double> w(l), Hr((size_t)l * l), Hi((size_t)l * l), Xr((size_t)l * l), Xi((size_t)l * l), A((size_t)l * l), Vr((size_t)l * l);
    expect(hl_heigh(H.data(), l, w.data(), V.data()) == 0, "heigh");
    for (size_t e = 0; e < H.size(); ++e) Hr[e] = A[e] = H[e].real(), Hi[e] = H[e].imag();
    std::vector<double> w2(l);
    expect(hl_zheigh_top_embedded(Hr.data(), Hi.data(), l, (l + 1) / 2, w2.data(), Xr.data(), Xi.data()) == 0, "zheigh_top_embedded");
    expect(hl_eigh(A.data(), l, w2.data(), Vr.data()) == 0, "eigh");
    expect(hl_peaked_spectrum(w.data(), l) == (std::sqrt(w[0] / w[l - 1]) > hostla::PEAKED_RATIO ? 1 : 0), "peaked_spectrum");
    std::vector<zdouble> Z((size_t)l * l);
    hl_ritz_block(Xr.data(), Xi.data(), l - 1, 1, Z.data());
    hl_zmatmul(H.data(), V.data(), l, Z.data());
  }
  for (int hl : {0, 1, 2}) {      // (h, l) of the [Re | Im] helpers
    const int h = hl == 2 ? 64 : 32, l = hl == 0 ? 7 : (hl == 1 ? 32 : 40), LP = 2 * h, Lo = 32, ko = 16, mcols = 5;
    std::vector<double> G((size_t)LP * LP), E((size_t)LP * Lo);
    for (auto& x : G) x = lcg();
    std::vector<zdouble> H((size_t)l * l), M((size_t)l * mcols);
    for (auto& x : M) x = draw<zdouble>();
    hl_hermitian_from_real(G.data(), LP, l, H.data());
    bool herm = true;
    for (int i = 0; i < l; ++i)
      for (int j = 0; j < l; ++j) herm = herm && H[(size_t)i * l + j] == std::conj(H[(size_t)j * l + i]);
    expect(herm, "hermitian_from_real");
    hl_embed_right(M.data(), mcols, l, mcols, LP, Lo, E.data(), nullptr);
    expect(E[(size_t)h * Lo + ko] == M[0].real(), "embed_right");
    std::vector<double> dref(l);
    hl_product_norms(H.data(), G.data(), 1, LP, l, dref.data());
  }
  for (int first : {0, 2, 4}) {    // null-column transform: k = 5, first = k - 1 included; then a zero and a dependent column
    const int Lo = 32, k = 5, rows = 40;
    for (int variant = 0; variant < 3; ++variant) {
      std::vector<double> P((size_t)rows * Lo), G((size_t)Lo * Lo, 0.0), M((size_t)Lo * Lo, -7.0);
      for (auto& x : P) x = lcg();
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < first; ++c) P[(size_t)r * Lo + c] = r == c ? 1.0 : 0.0;      // orthonormal leading columns
      for (int r = 0; r < rows; ++r) {
        if (variant == 1) P[(size_t)r * Lo + k - 1] = 0.0;
        if (variant == 2 && first > 0) P[(size_t)r * Lo + k - 1] = 2.0 * P[(size_t)r * Lo];
      }
      for (int r = 0; r < rows; ++r)
        for (int i = 0; i < Lo; ++i)
          for (int j = 0; j < Lo; ++j) G[(size_t)i * Lo + j] += P[(size_t)r * Lo + i] * P[(size_t)r * Lo + j];
      std::vector<int> flag(Lo, 0);
      const int rc = hl_null_column_transform(G.data(), Lo, first, k, 1, M.data(), flag.data());
      const int want = variant == 0 ? hostla::NULLCOL_OK : (variant == 1 ? hostla::NULLCOL_BAD : (first > 0 ? hostla::NULLCOL_DEPENDENT : hostla::NULLCOL_OK));
      expect(rc == want, "null_column_transform status");
      expect(rc == hostla::NULLCOL_OK || (flag[k - 1] == 1 && M[0] == -7.0), "null_column_transform flags");
    }
  }
  for (int first_null : {3, 5}) {  // complex repair: small = 9, k = 6, first_null = k - 1 included
    const int small = 9, k = 6, ko = 16, Lo = 32;
    std::vector<float> hp((size_t)small * Lo, 0.f);
    for (int r = 0; r < small; ++r)
      for (int j = 0; j < k; ++j) {
        hp[(size_t)r * Lo + j] = j < first_null ? (r == j ? 1.f : 0.f) : (float)lcg();
        hp[(size_t)r * Lo + ko + j] = j < first_null ? 0.f : (float)lcg();
      }
    for (int r = 0; r < small; ++r) {
      hp[(size_t)r * Lo + k - 1] = hp[(size_t)r * Lo + ko + k - 1] = 0.f;                    // a zero column
      if (first_null == 3) hp[(size_t)r * Lo + 4] = hp[(size_t)r * Lo + 1], hp[(size_t)r * Lo + ko + 4] = 0.f;     // inside the span
    }
    hl_null_repair_c(hp.data(), small, Lo, ko, first_null, k);
    double nn = 0.0;
    for (int r = 0; r < small; ++r) nn += (double)hp[(size_t)r * Lo + k - 1] * hp[(size_t)r * Lo + k - 1] + (double)hp[(size_t)r * Lo + ko + k - 1] * hp[(size_t)r * Lo + ko + k - 1];
    expect(std::fabs(nn - 1.0) < 1e-5, "null_repair_c unit column");
  }
  {                                // Rayleigh-Ritz assembly: 3 blocks + the coupling row, every combination of the options
    const int l = 4, LP = 64, nb = 4;
    for (int nWr : {2, 3})
      for (int with_last = 0; with_last < 2; ++with_last) {
        const int nbr = 3, nrow = nWr == 3 ? nb : nbr;
        std::vector<double> hCf((size_t)nrow * LP * nWr * LP), Hr((size_t)nbr * l * nbr * l), Hi(Hr.size()), Xr((size_t)nbr * l * l), Xi(Xr.size()), res(l);
        for (auto& x : hCf) x = lcg();
        for (auto& x : Xr) x = lcg();
        for (auto& x : Xi) x = lcg();
        std::vector<zdouble> Rf((size_t)nWr * l * l), Hqq((size_t)l * l);
        for (auto& x : Rf) x = draw<zdouble>();
        for (auto& x : Hqq) x = draw<zdouble>();
        const int has_rf[3] = {0, 1, 0};
        hl_ritz(hCf.data(), nrow, nWr, nbr, LP, l, Rf.data(), has_rf, with_last ? Hqq.data() : nullptr, Hr.data(), Hi.data(), Xr.data(), Xi.data(), res.data());
        bool herm = true;
        const int m = nbr * l;
        for (int i = 0; i < m; ++i)
          for (int j = 0; j < m; ++j) herm = herm && (i / l == j / l || (Hr[(size_t)i * m + j] == Hr[(size_t)j * m + i] && Hi[(size_t)i * m + j] == -Hi[(size_t)j * m + i]));
        expect(herm, "ritz_assemble Hermitian off-diagonal blocks");
      }
  }
  {
    const int l = 3, k = 2, checks = 4;
    const double wv[checks * l] = {1.0, 0.5, 0.1, 1.1, 0.6, 0.1, 1.11, 0.61, 0.1, 1.111, 0.611, 0.1};
    const int products[checks] = {4, 7, 10, 13};
    int verdicts[checks], next[checks];
    hl_ritz_history(wv, products, checks, k, l, 7, 2, 20, verdicts, next);
    expect(next[0] == 7 && verdicts[0] == 0, "RitzHistory");
  }
  std::printf("hostla selftest: %d failures\n", failures);
  return failures ? 1 : 0;
}
#endif
