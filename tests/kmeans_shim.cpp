// extern "C" wrappers around the plan of xeofs_amd/csrc/eofx_kmeans.hpp and nothing else: compiled by tests/kmeans_plan.py
// with the host C++ compiler (which does not define __HIPCC__, so the kernel is not seen) and loaded through ctypes.
#include <cstdint>

#include "eofx_kmeans.hpp"

extern "C" {

// KMEANS_KMAX, KMEANS_QMAX, KMEANS_NMAX, KMEANS_RMAX, KMEANS_ITER_MAX, KMEANS_WG, KMEANS_ACC_MAX, KMEANS_RED_BYTES
void km_constants(int32_t* out) {
  const int v[] = {eofx::KMEANS_KMAX, eofx::KMEANS_QMAX, eofx::KMEANS_NMAX, eofx::KMEANS_RMAX,
                   eofx::KMEANS_ITER_MAX, eofx::KMEANS_WG, eofx::KMEANS_ACC_MAX, eofx::KMEANS_RED_BYTES};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// out: grid, threads, qp, groups, rpt, acc_off, c_off, stage_off, cnt_off, lab_off, lds
void km_plan(int64_t n, int q, int k, int64_t R, int64_t* out) {
  const eofx::KmeansPlan pl = eofx::kmeans_plan(n, q, k, R);
  out[0] = pl.grid, out[1] = pl.threads, out[2] = pl.qp, out[3] = pl.groups, out[4] = pl.rpt, out[5] = (int64_t)pl.acc_off;
  out[6] = (int64_t)pl.c_off, out[7] = (int64_t)pl.stage_off, out[8] = (int64_t)pl.cnt_off, out[9] = (int64_t)pl.lab_off;
  out[10] = (int64_t)pl.lds;
}
}
