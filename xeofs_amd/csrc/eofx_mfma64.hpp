// eofx_mfma64.hpp -- the lane map of v_mfma_f64_16x16x4_f64, stated once.
//
// One instruction multiplies a 16 x 4 tile A by a 4 x 16 tile B and adds the 16 x 16 product to D, all float64, over
// the 64 lanes of a wave.  With (c, k) = (lane % 16, lane / 16), lane (c, k)
//     supplies  A[c][k]   (row c of the tile, k-step k),
//     supplies  B[k][c]   (k-step k, column c),
//     holds     D[k + 4 q][c]  in register q = 0 .. 3 of the accumulator
// (measured on gfx950).  A kernel on the fp64 matrix cores takes its lane coordinates, its products and the walk over
// its results from here and keeps what is its own: which tile of its problem an accumulator stands for, and how its
// operands reach the lanes.  Four kernels still carry index arithmetic of their own: atb_f64_kernel and
// panel_matmul_kernel are software-pipelined by hand, xgram_mfma_kernel and rot_step_wide_kernel measured slower on
// the helpers (docs/EXPERIMENTS.md); a new kernel starts from the helpers.
//
// Most kernels hold a 4 x 4 block of accumulators, acc[x][y], fed per k-step from four A values a[x] and four B values
// b[y].  Two ways of laying such a block over 64 x 64 outputs are in use:
//   blocked       tile (x, y) is the 16 x 16 outputs at (16 x, 16 y):   row = 16 x + k + 4 q,   col = 16 y + c;
//   interleaved   tile (x, y) takes every fourth row and column:        row = 4 (k + 4 q) + x,  col = 4 c + y
//                 (a lane that loads four adjacent floats holds one element of four tiles).
#pragma once
#include <hip/hip_runtime.h>

namespace eofx {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Row stride, in doubles, of a 64-column operand tile in LDS whose rows are the k-steps (lane (c, k) reads row 4 s + k, column
// 16 y + c): rows k and k + 1 lie on disjoint halves of the banks for the 32 lanes of a ds_read_b64 half-wave (k = 0, 1 | 2, 3).
constexpr int MFMA64_TILE_LD = 80;

struct Mfma64Lane {
  int c, k;
};
__device__ __forceinline__ Mfma64Lane mfma64_lane() {
  const int lane = threadIdx.x & 63;
  return {lane & 15, lane >> 4};
}

// the keep predicate of a block whose 16 tiles are all wanted
struct Mfma64All {
  __device__ __forceinline__ bool operator()(int, int) const { return true; }
};

__device__ __forceinline__ void mfma64_zero(f64x4& acc) { acc = f64x4{0.0, 0.0, 0.0, 0.0}; }
template <int N>
__device__ __forceinline__ void mfma64_zero(f64x4 (&acc)[N]) {
#pragma unroll
  for (int y = 0; y < N; ++y) mfma64_zero(acc[y]);
}
template <int M, int N>
__device__ __forceinline__ void mfma64_zero(f64x4 (&acc)[M][N]) {
#pragma unroll
  for (int x = 0; x < M; ++x) mfma64_zero(acc[x]);
}

// one k-step of one tile: D += A B with this lane's a = A[c][k], b = B[k][c]
__device__ __forceinline__ void mfma64_step(f64x4& acc, double a, double b) {
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
}
// one k-step of a 4 x 4 block, tile (x, y) only where keep(x, y)
template <class Keep>
__device__ __forceinline__ void mfma64_step(f64x4 (&acc)[4][4], const double (&a)[4], const double (&b)[4], Keep keep) {
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y)
      if (keep(x, y)) mfma64_step(acc[x][y], a[x], b[y]);
}

// f(row, col, value) for the four results of one tile that this lane holds
template <class F>
__device__ __forceinline__ void mfma64_each(const f64x4& acc, F f) {
  const Mfma64Lane ln = mfma64_lane();
#pragma unroll
  for (int q = 0; q < 4; ++q) f(ln.k + 4 * q, ln.c, acc[q]);
}
// f(x, y, row, col, value) for the results of the tiles with keep(x, y) of a 4 x 4 block, x outermost
template <class Keep, class F>
__device__ __forceinline__ void mfma64_each_blocked(const f64x4 (&acc)[4][4], Keep keep, F f) {
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y)
      if (keep(x, y)) mfma64_each(acc[x][y], [&](int r, int c, double v) { f(x, y, 16 * x + r, 16 * y + c, v); });
}
template <class Keep, class F>
__device__ __forceinline__ void mfma64_each_interleaved(const f64x4 (&acc)[4][4], Keep keep, F f) {
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y)
      if (keep(x, y)) mfma64_each(acc[x][y], [&](int r, int c, double v) { f(x, y, 4 * r + x, 4 * c + y, v); });
}

}  // namespace eofx
