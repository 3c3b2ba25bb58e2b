// extern "C" wrappers around two GPU-free pieces of the engine, built by the host compiler alone (tests/planes_shim.py):
//   * the layout of the fp16 planes of an in-place X Y pass's panel (eofx_plans.hpp: axb_plane_offset, axb_planes_bytes), and
//   * the sketch generator WITH its memo (eofx_sketch.hpp: gaussian_f32, sketch_memo_drop).
// With -DPLANES_SHIM_MAIN the file is a stand-alone program that drives the memo from eight threads with two alternating keys
// and checks every matrix against a fresh draw -- the program to build with -fsanitize=thread -pthread or
// -fsanitize=address,undefined (tests/test_sketch_memo_cpu.py does both where the toolchain has the runtimes).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "eofx_plans.hpp"
#include "eofx_sketch.hpp"

extern "C" {
int64_t ps_plane_offset(int64_t cb, int64_t K_all, int64_t k, int c, int plane) { return eofx::axb_plane_offset(cb, K_all, k, c, plane); }
int64_t ps_planes_bytes(int64_t K_all, int L) { return (int64_t)eofx::axb_planes_bytes(K_all, L); }
void ps_constants(int* out) {
  out[0] = eofx::AXB_KG;
  out[1] = eofx::AXB_PLANE_BYTES;
  out[2] = eofx::AXB_PAIR_BYTES;
}
void ps_sketch(uint32_t seed, int64_t rows, int64_t cols, float* out) { eofx_sketch::gaussian_f32(seed, rows, cols, out); }
void ps_sketch_draw(uint32_t seed, int64_t rows, int64_t cols, float* out) { eofx_sketch::gaussian_f32_draw(seed, rows, cols, out); }
void ps_sketch_drop() { eofx_sketch::sketch_memo_drop(); }
// 1 when the memo holds exactly this key
int ps_sketch_cached(uint32_t seed, int64_t rows, int64_t cols) {
  eofx_sketch::SketchMemo& mm = eofx_sketch::sketch_memo();
  std::lock_guard<std::mutex> lk(mm.mu);
  return mm.valid && mm.seed == seed && mm.rows == rows && mm.cols == cols ? 1 : 0;
}
int64_t ps_sketch_memo_max_bytes() { return (int64_t)eofx_sketch::SKETCH_MEMO_MAX_BYTES; }
}

#ifdef PLANES_SHIM_MAIN
int main() {
  int bad = 0;
  const uint32_t seeds[2] = {5, 6};
  const int64_t rows[2] = {700, 333}, cols[2] = {60, 61};
  std::vector<float> ref[2];
  for (int i = 0; i < 2; ++i) {
    ref[i].resize((size_t)(rows[i] * cols[i]));
    ps_sketch_draw(seeds[i], rows[i], cols[i], ref[i].data());
  }
  std::vector<int> wrong(8, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      std::vector<float> out;
      for (int it = 0; it < 12; ++it) {
        const int i = (t + it) & 1;
        out.assign(ref[i].size(), -1.f);
        ps_sketch(seeds[i], rows[i], cols[i], out.data());
        if (std::memcmp(out.data(), ref[i].data(), sizeof(float) * out.size()) != 0) ++wrong[t];
        if (t == 3 && it % 4 == 3) ps_sketch_drop();
      }
    });
  for (auto& x : th) x.join();
  for (int t = 0; t < 8; ++t) bad += wrong[t];
  // the layout: every half of a small panel's planes is hit exactly once
  const int64_t K_all = 128;
  const int L = 96;
  std::vector<int> hits((size_t)ps_planes_bytes(K_all, L) / 2, 0);
  for (int64_t col = 0; col < 128; ++col)
    for (int64_t k = 0; k < K_all; ++k)
      for (int plane = 0; plane < 2; ++plane) ++hits[(size_t)ps_plane_offset(col >> 6, K_all, k, (int)(col & 63), plane) / 2];
  for (int h : hits) bad += h != 1;
  ps_sketch_drop();
  std::printf(bad ? "planes_shim: %d FAILED\n" : "planes_shim: ok\n", bad);
  return bad ? 1 : 0;
}
#endif
