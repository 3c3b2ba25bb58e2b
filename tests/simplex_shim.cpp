// extern "C" wrappers around the plan of xeofs_amd/csrc/eofx_simplex.hpp and nothing else: compiled by tests/simplex_plan.py
// with the host C++ compiler (which does not define __HIPCC__, so the kernels are not seen) and loaded through ctypes.
#include <cstdint>

#include "eofx_simplex.hpp"

extern "C" {

// SIMPLEX_MMAX, SIMPLEX_KMAX, SIMPLEX_REG_MMAX, SIMPLEX_WG, SIMPLEX_PG_WG
void sx_constants(int32_t* out) {
  const int v[] = {eofx::SIMPLEX_MMAX, eofx::SIMPLEX_KMAX, eofx::SIMPLEX_REG_MMAX, eofx::SIMPLEX_WG, eofx::SIMPLEX_PG_WG};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// out: tier, lanes, epl, threads, rpb, grid, lds
void sx_plan(int64_t r, int64_t m, int64_t* out) {
  const eofx::SimplexPlan pl = eofx::simplex_plan(r, m);
  out[0] = pl.tier, out[1] = pl.lanes, out[2] = pl.epl, out[3] = pl.threads, out[4] = pl.rpb, out[5] = pl.grid, out[6] = (int64_t)pl.lds;
}

int sx_pg_width(int k) { return eofx::simplex_pg_width(k); }
}
