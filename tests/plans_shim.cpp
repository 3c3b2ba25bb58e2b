// extern "C" wrappers around the GPU-free headers of the engine (xeofs_amd/csrc/eofx_plans.hpp, eofx_sketch.hpp,
// eofx_hilbert_host.hpp, eofx_gwplan.hpp) for tests/test_plans_cpu.py, test_gram_plan_cpu.py, test_sketch_cpu.py,
// test_hilbert_host_cpu.py and test_gwplan_cpu.py, which compile this file with the host C++ compiler (tests/plans_shim.py) and load it through ctypes.
// With -DPLANS_SELFTEST the file is a stand-alone program that runs every wrapper on fixed inputs (for a sanitizer build:
// c++ -fsanitize=address,undefined, or -fsanitize=thread -pthread).
#include <cstdio>
#include <cstring>

#include "eofx_gwplan.hpp"
#include "eofx_hilbert_host.hpp"
#include "eofx_plans.hpp"
#include "eofx_sketch.hpp"

using namespace eofx;

extern "C" {
// ---- eofx_plans.hpp
void pl_constants(int* out) {
  const int c[] = {ATB_BM, ATB_KG, AXB_BM, AXB_KG, EOFX_LAG_GROUP_COLS, VIEWCOV_T, VIEWCOV_WGS, LAGCOV_PADW, LOWPASS_PADW, GW_T,
                   KRYLOV_MAX_ORDER, C64_IT_MIN, C64_IT_CAP};
  std::copy(c, c + 13, out);
}
int pl_atb_wide(int L) { return atb_wide(L) ? 1 : 0; }
// widths of the tiles in launch order (96: the partial 128-column tile) -> their number
int pl_tiles(int L, int wide, int* widths) {
  const ColTiles t = atb_tiles(L, wide != 0);
  int k = 0, next = 0;
  for (int i = 0; i < t.n; ++i) {
    if (t.t[i].col_base != next) return -1;      // the tiles must cover the panel in order
    for (int j = 0; j < t.t[i].count; ++j) widths[k++] = t.t[i].width;
    next += t.t[i].count * t.t[i].width;
  }
  return next == L && k == t.columns() ? k : -1;
}
int pl_atb_plan(int64_t M, int64_t K, int L, int wide, int64_t* kps) {
  const AtbPlan p = atb_plan(M, K, L, wide != 0);
  *kps = p.kps;
  return p.S;
}
int pl_axb_plan(int64_t rows_pad, int64_t K, int64_t* kps) {
  const AtbPlan p = axb_plan(rows_pad, K);
  *kps = p.kps;
  return p.S;
}
int64_t pl_atb_scratch_bytes(int64_t M, int64_t K, int L) { return (int64_t)atb_scratch_bytes(M, K, L); }
int pl_gram_parts(int64_t rows, int L) { return gram_parts(rows, L); }
int pl_rsvd_auto_iters(int k, int64_t n, int64_t p) { return rsvd_auto_iters(k, n, p); }
int pl_orth_tall_rule(int64_t tall_pad, int L, int prec) { return orth_tall_rule(tall_pad, L, prec) ? 1 : 0; }
int pl_spca_grid(int64_t rows, int64_t entries) { return spca_grid(rows, entries); }
int pl_lag_blocks(int64_t total4) { return lag_blocks(total4); }
int pl_lag_groupsize(int E, int L) { return lag_groupsize(E, L); }
// the lags per group in launch order, as eofx_lag_tmul_f32 / eofx_lag_mul_f32 walk them -> the number of groups
int pl_lag_groups(int E, int L, int* out) {
  const int G = lag_groupsize(E, L), Gl = lag_last_group(E, G);
  int k = 0;
  for (int e0 = 0; e0 < E; e0 += G) out[k++] = e0 + G >= E ? Gl : G;
  return k;
}
int pl_tmul_nt_ok(int64_t n, int64_t p_pad, int has_source, int L) { return tmul_nt_ok(n, p_pad, has_source != 0, L) ? 1 : 0; }
int pl_matmul_nt_ok(int64_t rows, int L, int Lo) { return matmul_nt_ok(rows, L, Lo) ? 1 : 0; }
int pl_gram_fast_ok(int64_t n_pad, int64_t p, int has_source) { return gram_fast_ok(n_pad, p, has_source != 0) ? 1 : 0; }
// The work list of gram_nt_kernel (S <= 0: the plan's own choice).  head [4] = {S, st_per_split, T, grid}; items [grid][5] = {bi, bj,
// st0, nst, slot} when grid <= cap_items; tiles [T][2] when T <= cap_tiles (call with zero capacities for the sizes) -> 0, or 1
// when a list did not fit, or -1 when a padding word of an item is not zero
int pl_gram_plan(int nti, int ntj, int sym, int nst_total, int S, int* head, int* items, int64_t cap_items, int* tiles, int64_t cap_tiles) {
  GramPlan pl;
  gram_plan_build(nti, ntj, sym != 0, nst_total, S, pl);
  const int h[] = {pl.S, pl.st_per_split, pl.T, pl.grid};
  std::copy(h, h + 4, head);
  if ((int64_t)pl.items.size() != pl.grid || (int64_t)pl.tiles.size() != pl.T || pl.nti != nti || pl.ntj != ntj) return -1;
  if (pl.grid > cap_items || pl.T > cap_tiles) return 1;
  for (const GramItem& it : pl.items) {
    if (it.pad0 | it.pad1 | it.pad2) return -1;
    const int o[] = {it.bi, it.bj, it.st0, it.nst, it.slot};
    items = std::copy(o, o + 5, items);
  }
  for (const GramTile& t : pl.tiles) {
    *tiles++ = t.x;
    *tiles++ = t.y;
  }
  return 0;
}
int pl_fit_first_eligible(int keep_raw, int prec, int aligned16, int64_t n, int64_t P, int l) {
  return fit_first_eligible(keep_raw, prec, aligned16 != 0, n, P, l) ? 1 : 0;
}
// out: kernel (0 scalar, 1 vec4, 2 transposing), RS, rps, gx, gxs
void pl_colstats_plan(int64_t n, int64_t P, int64_t ld, int aligned16, int sample_raw, int row_map, int64_t* out) {
  const ColstatsPlan p = colstats_plan(n, P, ld, aligned16 != 0, sample_raw != 0, row_map != 0);
  const int64_t o[] = {p.tr ? 2 : p.vec4 ? 1 : 0, p.RS, p.rps, p.gx, p.gxs};
  std::copy(o, o + 5, out);
}
int64_t pl_colstats_scratch(int64_t n, int64_t P) { return (int64_t)colstats_scratch(n, P); }
int pl_summary_blocks(int64_t P) { return summary_blocks(P); }
// out: raw, masked, in_place, col_map, vec
void pl_apply_plan(int64_t n, int64_t P, int64_t pv, int64_t ns, int keep_raw, int allow_masked, int stats_absmax, int aligned16, int* out) {
  const ApplyPlan p = apply_plan(n, P, pv, ns, keep_raw, allow_masked != 0, stats_absmax != 0, aligned16 != 0);
  const int o[] = {p.raw, p.masked, p.in_place, p.col_map, p.vec};
  std::copy(o, o + 5, out);
}
// view [p], tiles [2 x at most cap], out3 = {G, chunk, nslabs} -> ntiles, or minus the status of a bad off
int pl_viewcov_plan(int64_t n, int p, const int* off, int m, int keep_diag, int* view, int* tiles, int cap, int64_t* out3) {
  ViewcovPlan pl;
  const int bad = viewcov_plan(n, p, off, m, keep_diag != 0, pl);
  if (bad != VIEWCOV_OFF_OK) return -bad;
  if (pl.ntiles > cap || (int64_t)pl.host.size() != (int64_t)p + 2 * pl.ntiles) return -100;
  std::copy(pl.host.begin(), pl.host.begin() + p, view);
  std::copy(pl.host.begin() + p, pl.host.end(), tiles);
  out3[0] = pl.G;
  out3[1] = pl.chunk;
  out3[2] = pl.nslabs;
  return pl.ntiles;
}
// wpad [ntau + 30] / wsym [2 h + 31]; nyG = {ny, G} -> the length of the padded vector
int pl_lagcov_plan(int64_t n, int p, const double* w, int ntau, double* wpad, int* nyG) {
  const FilterPlan pl = lagcov_plan(n, p, w, ntau);
  std::copy(pl.w.begin(), pl.w.end(), wpad);
  nyG[0] = pl.ny;
  nyG[1] = pl.G;
  return (int)pl.w.size();
}
int pl_lowpass_plan(int64_t n, int p, const double* w, int h, double* wsym, int* nyG) {
  const FilterPlan pl = lowpass_plan(n, p, w, h);
  std::copy(pl.w.begin(), pl.w.end(), wsym);
  nyG[0] = pl.ny;
  nyG[1] = pl.G;
  return (int)pl.w.size();
}

// out [19]: status, r, l, adaptive, n_iter, auto_count, h, LP, ko, Lo, transposed, small, small_pad, tall_pad, big, krylov, nbmax,
// ldk, arena_bytes
void pl_c64_plan(int64_t n, int64_t p, int64_t n_pad, int64_t p_pad, int64_t p_total, int masked, int64_t p_valid, int k, int n_oversamples,
                 int n_iter, int krylov_allowed, int64_t* out) {
  const C64Plan c = c64_plan(n, p, n_pad, p_pad, p_total, masked != 0, p_valid, k, n_oversamples, n_iter, krylov_allowed != 0);
  const int64_t o[] = {c.status, c.r, c.l, c.adaptive, c.n_iter, c.auto_count, c.h, c.LP, c.ko, c.Lo, c.transposed, c.small, c.small_pad,
                       c.tall_pad, c.big, c.krylov, c.nbmax, c.ldk, (int64_t)c.arena_bytes};
  std::copy(o, o + 19, out);
}
int64_t pl_c64_mul_scratch_bytes(int64_t n, int64_t p, int64_t n_pad, int64_t p_pad, int L) {
  return (int64_t)c64_mul_scratch_bytes(n, p, n_pad, p_pad, L);
}

int64_t pl_null_repair_bytes(int64_t rows_pad, int Lo) { return (int64_t)null_repair_bytes(rows_pad, Lo); }
int64_t pl_rinv_blocked_bytes(int l) { return (int64_t)rinv_blocked_bytes(l); }
int64_t pl_rsvd_scratch_bytes(int64_t tall_pad, int64_t small_pad, int l, int k) { return (int64_t)rsvd_scratch_bytes(tall_pad, small_pad, l, k); }
// out [9]: status, r, l_req, l, L, Lo, n_iter, transposed, full_width
static void rsvd_plan_out(const RsvdPlan& q, int64_t* out) {
  const int64_t o[] = {q.status, q.r, q.l_req, q.l, q.L, q.Lo, q.n_iter, q.transposed, q.full_width};
  std::copy(o, o + 9, out);
}
void pl_rsvd_plan(int64_t rows, int64_t cols, int k, int n_oversamples, int n_iter, int64_t* out) {
  rsvd_plan_out(rsvd_plan(rows, cols, k, n_oversamples, n_iter), out);
}
// out [15]: the nine of pl_rsvd_plan, then tall, small, tall_pad, small_pad, gram_route, arena_bytes
void pl_cross_plan(int64_t n, int64_t n_pad, int64_t p1, int64_t p1_pad, int64_t p2, int64_t p2_pad, int64_t P1, int64_t P2, int sharded,
                   int want_tsc, int fast1, int fast2, int64_t fast_scratch1, int64_t fast_scratch2, int k, int n_oversamples, int n_iter,
                   int no_gram, int64_t* out) {
  const CrossPlan c = cross_plan(n, n_pad, p1, p1_pad, p2, p2_pad, P1, P2, sharded != 0, want_tsc != 0, fast1 != 0, fast2 != 0,
                                 (size_t)fast_scratch1, (size_t)fast_scratch2, k, n_oversamples, n_iter, no_gram != 0);
  rsvd_plan_out(c, out);
  const int64_t o[] = {c.tall, c.small, c.tall_pad, c.small_pad, c.gram_route, (int64_t)c.arena_bytes};
  std::copy(o, o + 6, out + 9);
}
int pl_fused_fit_eligible(int keep_raw, int prec, int aligned16, int64_t n, int64_t P, int k, int n_oversamples, int64_t omega_rows,
                          int omega_on_device) {
  return fused_fit_eligible(keep_raw, prec, aligned16 != 0, n, P, k, rsvd_plan(n, P, k, n_oversamples, -1), omega_rows, omega_on_device != 0) ? 1 : 0;
}

// ---- eofx_sketch.hpp
void sk_gaussian_f32(uint32_t seed, int64_t rows, int64_t cols, float* out) { eofx_sketch::gaussian_f32(seed, rows, cols, out); }
int64_t sk_candidates(int64_t need) { return eofx_sketch::candidates(need); }

// ---- eofx_hilbert_host.hpp (complex arrays: interleaved (re, im) doubles)
double hh_kappa(int64_t N, int64_t d) { return hilbert_kappa(N, d); }
void hh_fft(std::complex<double>* a, int64_t N) {
  std::vector<std::complex<double>> v(a, a + N);
  host_fft_f64(v);
  std::copy(v.begin(), v.end(), a);
}
int64_t hh_length(int64_t n, int* log2_out) { return hilbert_length(n, log2_out); }
int64_t hh_position_frequency(int L, int64_t pos) { return hfft::position_frequency(L, pos); }
void hh_fused_table(int64_t n, int64_t N, int L, float* out) {      // [2^L]
  const std::vector<float> t = hilbert_fused_table(n, N, L);
  std::copy(t.begin(), t.end(), out);
}
void hh_circular_kernel(int64_t n, int64_t N, int64_t P, float* out) {      // [P + 2]
  const std::vector<float> t = hilbert_circular_kernel(n, N, P);
  std::copy(t.begin(), t.end(), out);
}
void hh_pad_vectors(int64_t n, int64_t N, double decay, double* out) {      // [4][n]
  std::vector<double> u;
  hilbert_pad_vectors(n, N, decay, u);
  std::copy(u.begin(), u.end(), out);
}
void hh_pad_table(int64_t n, int64_t N, double decay, int interleaved, float* out) {      // [4 n + 4]
  const std::vector<float> t = hilbert_pad_table(n, N, decay, interleaved != 0);
  std::copy(t.begin(), t.end(), out);
}
int hh_operator(int64_t n, int padding, double decay, float* out) {      // [n][n]
  std::vector<float> hc;
  if (!build_hilbert_operator_host(n, padding, decay, hc)) return 1;
  std::copy(hc.begin(), hc.end(), out);
  return 0;
}

// ---- eofx_gwplan.hpp
void* gwp_build(const double* xy, int64_t n, int64_t first, int64_t count, int64_t chunk, int sorted, int metric, int kernel, double bw) {
  GwPlan* plan = new GwPlan();
  gw_plan(xy, n, first, count, chunk, sorted != 0, metric, kernel, bw, *plan);
  return plan;
}
void gwp_free(void* h) { delete static_cast<GwPlan*>(h); }
// out: chunks, centre tiles, entries of cols, entries of rowptr, visited, possible, neighbour tiles, centres in all chunks
void gwp_sizes(const void* h, int64_t* out) {
  const GwPlan& p = *static_cast<const GwPlan*>(h);
  int64_t centres = 0;
  for (auto& ch : p.chunks) centres += ch.count;
  const int64_t o[] = {(int64_t)p.chunks.size(), p.ctiles, (int64_t)p.cols.size(), (int64_t)p.rowptr.size(), p.visited, p.possible, p.nb.ntiles, centres};
  std::copy(o, o + 8, out);
}
// nb_perm [n], nb_geo [3 n], rowptr, cols, chunk_info [chunks][5] = {first, count, off_tiles, off_cols, tiles}, c_perm [centres],
// c_geo [3 centres] (the chunks one after the other, as gw_run uploads them)
void gwp_copy(const void* h, int64_t* nb_perm, double* nb_geo, int* rowptr, int* cols, int64_t* chunk_info, int64_t* c_perm, double* c_geo) {
  const GwPlan& p = *static_cast<const GwPlan*>(h);
  std::copy(p.nb.perm.begin(), p.nb.perm.end(), nb_perm);
  std::copy(p.nb.geo.begin(), p.nb.geo.end(), nb_geo);
  std::copy(p.rowptr.begin(), p.rowptr.end(), rowptr);
  std::copy(p.cols.begin(), p.cols.end(), cols);
  for (auto& ch : p.chunks) {
    const int64_t o[] = {ch.first, ch.count, ch.off_tiles, ch.off_cols, ch.c.ntiles};
    chunk_info = std::copy(o, o + 5, chunk_info);
    c_perm = std::copy(ch.c.perm.begin(), ch.c.perm.end(), c_perm);
    c_geo = std::copy(ch.c.geo.begin(), ch.c.geo.end(), c_geo);
  }
}
}

#ifdef PLANS_SELFTEST
namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    std::fprintf(stderr, "plans selftest: FAILED %s\n", what);
  }
}
uint64_t lcg_state = 0x2545F4914F6CDD1Dull;
double lcg() {      // uniform in [-1, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((lcg_state >> 11) & 0xFFFFFFFFull) / 2147483648.0 - 1.0;
}
}  // namespace

int main() {
  // plans
  int widths[64], c[13];
  pl_constants(c);
  for (int L = 32; L <= 544; L += 32) {
    expect(pl_tiles(L, 0, widths) > 0 && pl_tiles(L, 1, widths) > 0, "tiles cover the panel");
    for (int64_t M : {512, 2560, 512 * 1024})
      for (int64_t K : {32, 1056, 40032}) {
        int64_t kps = 0;
        const int S = pl_atb_plan(M, K, L, L >= 96, &kps);
        expect(S * kps >= K && (S - 1) * kps < K && kps % ATB_KG == 0, "atb_plan");
        expect(pl_atb_scratch_bytes(M, K, L) >= 4096, "atb_scratch_bytes");
      }
    int groups[64];
    expect(pl_lag_groups(21, L, groups) >= 1, "lag_groups");
  }
  for (int64_t rows_pad : {256, 512, 256 * 1023, 256 * 1024})
    for (int64_t K : {64, 15 * 64, 16 * 64, 17 * 64, 5056}) {
      int64_t kps = 0;
      const int S = pl_axb_plan(rows_pad, K, &kps);
      expect(S * kps >= K && (S - 1) * kps < K && kps % AXB_KG == 0, "axb_plan");
    }
  expect(pl_gram_parts(130000, 1536) >= 1 && pl_rsvd_auto_iters(3, 100, 200) == 7 && pl_orth_tall_rule(512, 32, EOFX_PREC_F32) == 1, "rules");
  expect(pl_spca_grid(100000, 64) >= 1 && pl_lag_blocks(0) == 1 && pl_tmul_nt_ok(1037, 2560, 1, 512) == 1, "rules");
  expect(pl_matmul_nt_ok(1024, 512, 256) == 1 && pl_gram_fast_ok(512, 1000, 1) == 1 && pl_fit_first_eligible(2, EOFX_PREC_F16X3, 1, 120, 132, 16) == 1, "predicates");
  // the work list of gram_nt_kernel: the splits of every tile cover the stages once, the forced S is normalised
  for (int sym = 0; sym < 2; ++sym)
    for (int nt : {1, 3, 8, 128})
      for (int nst : {2, 26, 2050})
        for (int S : {0, 1, 5, 40}) {
          int head[4];
          expect(pl_gram_plan(nt, nt == 128 ? 7 : nt, sym, nst, S, head, nullptr, 0, nullptr, 0) == 1, "gram_plan sizes");
          std::vector<int> items(5 * (size_t)head[3]), tiles(2 * (size_t)head[2]);
          expect(pl_gram_plan(nt, nt == 128 ? 7 : nt, sym, nst, S, head, items.data(), head[3], tiles.data(), head[2]) == 0, "gram_plan");
          std::vector<int> covered((size_t)head[2], 0);
          for (int b = 0; b < head[3]; ++b) {
            const int* it = &items[5 * (size_t)b];
            if (it[3] <= 0) continue;
            const int tile = it[4] / head[0];
            expect(it[4] >= 0 && tile < head[2] && it[3] % 2 == 0 && it[2] == it[4] % head[0] * head[1] && tiles[2 * (size_t)tile] == it[0] &&
                       tiles[2 * (size_t)tile + 1] == it[1],
                   "gram_plan item");
            if (tile < head[2]) covered[(size_t)tile] += it[3];
          }
          for (int c : covered) expect(c == nst, "gram_plan covers every stage of every tile once");
          expect(S <= 0 || head[0] == (nst + head[1] - 1) / head[1], "gram_plan normalises a forced S");
        }
  {
    int head[4];
    (void)pl_gram_plan(2, 2, 1, 26, 40, head, nullptr, 0, nullptr, 0);
    expect(head[0] == 13 && head[1] == 2, "gram_plan: S = 40 of 26 stages");
    (void)pl_gram_plan(2, 2, 1, 26, 5, head, nullptr, 0, nullptr, 0);
    expect(head[0] == 5 && head[1] == 6, "gram_plan: S = 5 of 26 stages");
  }
  int64_t cs[5];
  int ap[5];
  for (int64_t n : {2, 63, 64, 700, 5000})
    for (int64_t P : {3, 4, 260, 1300, 8200}) {
      pl_colstats_plan(n, P, P, 1, 1, 0, cs);
      expect(cs[1] >= 1 && cs[1] * cs[2] >= n && (cs[1] - 1) * cs[2] < n, "colstats_plan");
      pl_apply_plan(n, P, P - 1, n, 2, 1, 1, 1, ap);
      expect(pl_summary_blocks(P) >= 1 && pl_colstats_scratch(n, P) > 0, "summary_blocks");
    }
  {
    const int p = 300, off[] = {0, 128, 200, 300}, bad[] = {0, 200, 200, 300};
    std::vector<int> view(p), tiles(2 * 16);
    int64_t o3[3];
    expect(pl_viewcov_plan(5000, p, off, 3, 0, view.data(), tiles.data(), 16, o3) > 0, "viewcov_plan");
    expect(pl_viewcov_plan(5000, p, bad, 3, 0, view.data(), tiles.data(), 16, o3) == -VIEWCOV_OFF_ORDER, "viewcov_plan off");
    std::vector<double> w(66, 0.5), wp(2 * 65 + 31);
    int nyG[2];
    expect(pl_lagcov_plan(700, 130, w.data(), 66, wp.data(), nyG) == 66 + 30, "lagcov_plan");
    expect(pl_lowpass_plan(700, 130, w.data(), 40, wp.data(), nyG) == 81 + 30, "lowpass_plan");
  }
  // the complex driver's plan, the hand cases of tests/test_plans_cpu.py: {n, p, p_total, masked, p_valid, k, n_oversamples, n_iter,
  // krylov_allowed} -> {status, l, LP, n_iter, transposed, krylov, nbmax}
  {
    const int64_t cases[][16] = {
        {300, 900, 0, 0, 0, 22, 10, -1, 1, /**/ C64_PLAN_OK, 32, 64, 7, 1, 1, 8},     {300, 900, 0, 0, 0, 23, 10, -1, 1, /**/ C64_PLAN_OK, 33, 128, 7, 1, 1, 8},
        {300, 900, 0, 0, 0, 29, 10, -1, 1, /**/ C64_PLAN_OK, 39, 128, 7, 1, 1, 8},    {300, 900, 0, 0, 0, 30, 10, -1, 1, /**/ C64_PLAN_OK, 40, 128, 4, 1, 1, 5},
        {300, 900, 0, 0, 0, 6, 10, 0, 1, /**/ C64_PLAN_OK, 16, 64, 0, 1, 0, 0},       {300, 900, 0, 0, 0, 6, 10, -2, 1, /**/ C64_PLAN_OK, 16, 64, 20, 1, 1, 21},
        {300, 900, 0, 0, 0, 6, 10, -3, 1, /**/ C64_PLAN_N_ITER, 16, 0, 0, 0, 0, 0},   {300, 900, 0, 0, 0, 38, 10, 7, 1, /**/ C64_PLAN_OK, 48, 128, 7, 1, 1, 8},
        {300, 900, 0, 0, 0, 39, 10, 7, 1, /**/ C64_PLAN_OK, 49, 128, 7, 1, 1, 7},     {300, 900, 0, 0, 0, 54, 10, 7, 1, /**/ C64_PLAN_OK, 64, 128, 7, 1, 1, 6},
        {300, 900, 0, 0, 0, 55, 10, 7, 1, /**/ C64_PLAN_WIDTH, 65, 0, 0, 0, 0, 0},    {20, 900, 0, 0, 0, 21, 10, -1, 1, /**/ C64_PLAN_RANK, 0, 0, 0, 0, 0, 0},
        {300, 900, 0, 1, 301, 6, 10, -1, 1, /**/ C64_PLAN_OK, 16, 64, 7, 1, 1, 8},    {300, 900, 0, 1, 300, 6, 10, -1, 1, /**/ C64_PLAN_MASKED, 16, 0, 0, 0, 0, 0},
        {300, 100, 301, 0, 0, 6, 10, -1, 1, /**/ C64_PLAN_OK, 16, 64, 7, 1, 1, 8},    {300, 100, 300, 0, 0, 6, 10, -1, 1, /**/ C64_PLAN_SHARD_SIDE, 0, 0, 0, 0, 0, 0},
        {900, 300, 0, 0, 0, 6, 10, -1, 1, /**/ C64_PLAN_OK, 16, 64, 7, 0, 1, 8},      {300, 900, 0, 0, 0, 6, 10, -1, 0, /**/ C64_PLAN_OK, 16, 64, 7, 1, 0, 0}};
    for (auto& q : cases) {
      int64_t o[19];
      pl_c64_plan(q[0], q[1], round_up(q[0], ATB_BM), round_up(q[1], ATB_BM), q[2], (int)q[3], q[4], (int)q[5], (int)q[6], (int)q[7], (int)q[8], o);
      expect(o[0] == q[9] && o[2] == q[10] && o[7] == q[11] && o[4] == q[12] && o[10] == q[13] && o[15] == q[14] && o[16] == q[15], "c64_plan hand case");
      expect(o[0] != C64_PLAN_OK || (o[16] * o[2] <= KRYLOV_MAX_ORDER && o[17] == o[16] * o[7] && o[18] > 0), "c64_plan invariants");
    }
    expect(pl_c64_mul_scratch_bytes(300, 900, 512, 1024, 64) > (8 << 20), "c64_mul_scratch_bytes");
  }
  // the real drivers' plans, the hand cases of tests/test_plans_cpu.py: {rows, cols, k, n_oversamples, n_iter} -> {status, r, l, L,
  // n_iter, transposed, full_width}; then the cross plan in both forms and the fused-fit predicate
  {
    const int64_t cases[][12] = {{700, 60, 5, 10, -1, /**/ RSVD_PLAN_OK, 60, 15, 32, 7, 0, 0},   {60, 700, 5, 10, -1, /**/ RSVD_PLAN_OK, 60, 15, 32, 7, 1, 0},
                                 {60, 12, 4, 10, -1, /**/ RSVD_PLAN_OK, 12, 12, 32, 4, 0, 1},    {60, 12, 13, 0, -1, /**/ RSVD_PLAN_RANK, 12, 12, 32, 4, 0, 1},
                                 {900, 400, 250, 10, 3, /**/ RSVD_PLAN_WIDTH, 400, 260, 288, 3, 0, 0}};
    for (auto& q : cases) {
      int64_t o[9];
      pl_rsvd_plan(q[0], q[1], (int)q[2], (int)q[3], (int)q[4], o);
      expect(o[0] == q[5] && o[1] == q[6] && o[3] == q[7] && o[4] == q[8] && o[6] == q[9] && o[7] == q[10] && o[8] == q[11], "rsvd_plan hand case");
    }
    int64_t loc[15], shd[15];
    for (int route = 0; route < 2; ++route) {
      pl_cross_plan(300, 512, 1300, 1536, 900, 1024, 1300, 900, 0, 1, route, route, 5 << 20, 3 << 20, 6, 10, -1, 0, loc);
      pl_cross_plan(300, 512, 1300, 1536, 900, 1024, 1300, 900, 1, 1, route, route, 5 << 20, 3 << 20, 6, 10, -1, 0, shd);
      expect(loc[0] == RSVD_PLAN_OK && loc[13] == route && loc[9] == 1300 && loc[12] == 1024 && shd[14] >= loc[14] && loc[14] > 0, "cross_plan");
    }
    expect(pl_null_repair_bytes(1536, 32) > 1536 * 32 * 4 && pl_rinv_blocked_bytes(100) > 0 && pl_rsvd_scratch_bytes(1536, 512, 16, 6) > (4 << 20),
           "real drivers' sizes");
    expect(pl_fused_fit_eligible(2, EOFX_PREC_F16X3, 1, 120, 132, 6, 10, 120, 0) == 1 && pl_fused_fit_eligible(2, EOFX_PREC_F16X3, 1, 120, 132, 6, 10, 119, 0) == 0,
           "fused_fit_eligible");
  }
  // the sketch generator at eight threads (twice: the second call reuses the pool and the buffers) and at one
  {
    const int64_t rows = 3000, cols = 61;
    std::vector<float> a((size_t)rows * cols), b(a.size()), s((size_t)7 * 3);
    setenv("EOFX_SKETCH_THREADS", "8", 1);
    sk_gaussian_f32(5, rows, cols, a.data());
    sk_gaussian_f32(5, rows, cols, b.data());
    expect(a == b, "sketch: two calls at 8 threads");
    setenv("EOFX_SKETCH_THREADS", "1", 1);
    sk_gaussian_f32(5, rows, cols, b.data());
    expect(a == b, "sketch: 1 thread against 8");
    sk_gaussian_f32(0, 7, 3, s.data());
    sk_gaussian_f32(1, 0, 3, s.data());
    expect(sk_candidates(1) > 1, "sketch candidates");
  }
  // the Hilbert setup: both builders run their threads from n = 512 on
  {
    for (int64_t n : {1, 2, 7, 300, 600}) {
      int L = 0;
      const int64_t P = hh_length(n, &L);
      std::vector<float> t((size_t)P + 2), u((size_t)4 * n + 4), hc((size_t)n * n);
      hh_fused_table(n, 3 * n, L, t.data());
      hh_circular_kernel(n, n, P, t.data());
      hh_pad_table(n, 3 * n, 0.2, 1, u.data());
      hh_pad_table(n, 3 * n, 0.2, 0, u.data());
      expect(hh_operator(n, 1, 0.2, hc.data()) == 0 && hh_operator(n, 0, 0.2, hc.data()) == 0, "hilbert operator");
    }
    std::vector<float> t((size_t)1 << 15);
    hh_fused_table(9000, 27000, 15, t.data());
    std::vector<std::complex<double>> a(1024);
    for (auto& x : a) x = {lcg(), lcg()};
    hh_fft(a.data(), 1024);
    expect(hh_kappa(8, 0) == 0.0 && hh_position_frequency(10, 0) == 0, "hilbert kappa");
  }
  // the GWPCA plan: both metrics, sorted and unsorted
  for (int metric = 0; metric < 2; ++metric)
    for (int64_t n : {1, 16, 17, 700}) {
      std::vector<double> xy(2 * (size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        xy[2 * i] = 180.0 * lcg();
        xy[2 * i + 1] = 90.0 * lcg();
      }
      for (int sorted = 0; sorted < 2; ++sorted) {
        void* h = sorted ? gwp_build(xy.data(), n, 0, n, 32, 1, metric, 0, 40.0) : gwp_build(xy.data(), n, n / 3, n - n / 3, n, 0, metric, 1, 40.0);
        int64_t sz[8];
        gwp_sizes(h, sz);
        std::vector<int64_t> np((size_t)n), info(5 * (size_t)sz[0]), cp((size_t)sz[7]);
        std::vector<double> ng(3 * (size_t)n), cg(3 * (size_t)sz[7]);
        std::vector<int> rp((size_t)sz[3]), cl((size_t)sz[2] + 1);
        gwp_copy(h, np.data(), ng.data(), rp.data(), cl.data(), info.data(), cp.data(), cg.data());
        expect(sz[4] <= sz[5] && sz[3] == sz[1] + sz[0], "gw_plan sizes");
        gwp_free(h);
      }
    }
  if (failures) return 1;
  std::printf("plans selftest: ok\n");
  return 0;
}
#endif
