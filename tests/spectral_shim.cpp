// extern "C" wrappers around the plans of xeofs_amd/csrc/eofx_spectral.hpp and nothing else: compiled by
// tests/test_spectraleof_host.py with the host C++ compiler (which does not define __HIPCC__, so the kernels are not seen)
// and loaded through ctypes.
#include <cstdint>

#include "eofx_spectral.hpp"

extern "C" {

// BLOCKXFORM_NFFT_MAX, BLOCKXFORM_NCOEF_MAX, BLOCKXFORM_TS, BLOCKXFORM_TC, BLOCKXFORM_WGS, BLOCKXFORM_GMAX, ROWGRAM_RMAX,
// ROWGRAM_SPAN, ROWGRAM_SMAX, ROWGRAM_NBMAX, SLABMUL_QMAX, SLABMUL_RMAX, SLABMUL_NBMAX, SLABMUL_TP
void sp_constants(int32_t* out) {
  const int v[] = {eofx::BLOCKXFORM_NFFT_MAX, eofx::BLOCKXFORM_NCOEF_MAX, eofx::BLOCKXFORM_TS, eofx::BLOCKXFORM_TC, eofx::BLOCKXFORM_WGS,
                   eofx::BLOCKXFORM_GMAX,     eofx::ROWGRAM_RMAX,         eofx::ROWGRAM_SPAN,  eofx::ROWGRAM_SMAX,  eofx::ROWGRAM_NBMAX,
                   eofx::SLABMUL_QMAX,        eofx::SLABMUL_RMAX,         eofx::SLABMUL_NBMAX, eofx::SLABMUL_TP};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// out: stiles, ctiles, groups
void sp_blockxform_plan(int64_t p, int64_t ncoef, int64_t nblk, int64_t* out) {
  const eofx::BlockxformPlan pl = eofx::blockxform_plan(p, ncoef, nblk);
  out[0] = pl.stiles, out[1] = pl.ctiles, out[2] = pl.groups;
}

// out: rt, spans, splits
void sp_rowgram_plan(int64_t r, int64_t p, int64_t nb, int64_t* out) {
  const eofx::RowgramPlan pl = eofx::rowgram_plan(r, p, nb);
  out[0] = pl.rt, out[1] = pl.spans, out[2] = pl.splits;
}

int64_t sp_first(int64_t count, int parts, int z) { return eofx::spectral_first(count, parts, z); }
int sp_slabmul_qt(int64_t q) { return eofx::slabmul_qt(q); }
}
