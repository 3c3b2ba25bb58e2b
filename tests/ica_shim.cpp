// extern "C" wrappers around the plan of xeofs_amd/csrc/eofx_ica.hpp and nothing else: compiled by tests/ica_plan.py with the
// host C++ compiler (which does not define __HIPCC__, so the kernels are not seen) and loaded through ctypes.
#include <cstdint>

#include "eofx_ica.hpp"

extern "C" {

// ICA_QMAX, ICA_NMAX, ICA_RMAX, ICA_ITER_MAX, ICA_WG, ICA_BMAX
void ica_constants(int32_t* out) {
  const int v[] = {eofx::ICA_QMAX, eofx::ICA_NMAX, eofx::ICA_RMAX, eofx::ICA_ITER_MAX, eofx::ICA_WG, eofx::ICA_BMAX};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// out: blocks, rows, qp, qw, slot, lds
void ica_plan(int64_t n, int q, int64_t* out) {
  const eofx::IcaPlan pl = eofx::ica_plan(n, q);
  out[0] = pl.blocks, out[1] = pl.rows, out[2] = pl.qp, out[3] = pl.qw, out[4] = pl.slot, out[5] = (int64_t)pl.lds;
}

// float64 words of scratch for R restarts
int64_t ica_scratch(int64_t n, int q, int64_t R) { return (int64_t)eofx::ica_scratch(n, q, R); }
}
