"""Builds tests/plans_shim.cpp (extern "C" wrappers around the GPU-free headers eofx_plans.hpp, eofx_sketch.hpp,
eofx_hilbert_host.hpp and eofx_gwplan.hpp) with the host C++ compiler and loads it through ctypes -- once per session, shared by
the CPU tests of the four headers.  `lib()` skips the calling test when there is no compiler."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
I, I64, D, P, U32 = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32

SIGNATURES = {
    "pl_constants": (None, [P]), "pl_atb_wide": (I, [I]), "pl_tiles": (I, [I, I, P]), "pl_atb_plan": (I, [I64, I64, I, I, P]),
    "pl_axb_plan": (I, [I64, I64, P]), "pl_atb_scratch_bytes": (I64, [I64, I64, I]), "pl_gram_parts": (I, [I64, I]),
    "pl_rsvd_auto_iters": (I, [I, I64, I64]), "pl_orth_tall_rule": (I, [I64, I, I]), "pl_spca_grid": (I, [I64, I64]),
    "pl_lag_blocks": (I, [I64]), "pl_lag_groupsize": (I, [I, I]), "pl_lag_groups": (I, [I, I, P]),
    "pl_tmul_nt_ok": (I, [I64, I64, I, I]), "pl_matmul_nt_ok": (I, [I64, I, I]), "pl_gram_fast_ok": (I, [I64, I64, I]),
    "pl_gram_plan": (I, [I, I, I, I, I, P, P, I64, P, I64]), "pl_fit_first_eligible": (I, [I, I, I, I64, I64, I]), "pl_colstats_plan": (None, [I64, I64, I64, I, I, I, P]),
    "pl_colstats_scratch": (I64, [I64, I64]), "pl_summary_blocks": (I, [I64]),
    "pl_apply_plan": (None, [I64, I64, I64, I64, I, I, I, I, P]), "pl_viewcov_plan": (I, [I64, I, P, I, I, P, P, I, P]),
    "pl_lagcov_plan": (I, [I64, I, P, I, P, P]), "pl_lowpass_plan": (I, [I64, I, P, I, P, P]),
    "pl_c64_plan": (None, [I64, I64, I64, I64, I64, I, I64, I, I, I, I, P]), "pl_c64_mul_scratch_bytes": (I64, [I64, I64, I64, I64, I]),
    "pl_null_repair_bytes": (I64, [I64, I]), "pl_rinv_blocked_bytes": (I64, [I]), "pl_rsvd_scratch_bytes": (I64, [I64, I64, I, I]),
    "pl_rsvd_plan": (None, [I64, I64, I, I, I, P]),
    "pl_cross_plan": (None, [I64, I64, I64, I64, I64, I64, I64, I64, I, I, I, I, I64, I64, I, I, I, I, P]),
    "pl_fused_fit_eligible": (I, [I, I, I, I64, I64, I, I, I64, I]),
    "sk_gaussian_f32": (None, [U32, I64, I64, P]), "sk_candidates": (I64, [I64]),
    "hh_kappa": (D, [I64, I64]), "hh_fft": (None, [P, I64]), "hh_length": (I64, [I64, P]), "hh_position_frequency": (I64, [I, I64]),
    "hh_fused_table": (None, [I64, I64, I, P]), "hh_circular_kernel": (None, [I64, I64, I64, P]),
    "hh_pad_vectors": (None, [I64, I64, D, P]), "hh_pad_table": (None, [I64, I64, D, I, P]), "hh_operator": (I, [I64, I, D, P]),
    "gwp_build": (P, [P, I64, I64, I64, I64, I, I, I, D]), "gwp_free": (None, [P]), "gwp_sizes": (None, [P, P]),
    "gwp_copy": (None, [P, P, P, P, P, P, P, P]),
}
CONSTANTS = ("ATB_BM", "ATB_KG", "AXB_BM", "AXB_KG", "LAG_GROUP_COLS", "VIEWCOV_T", "VIEWCOV_WGS", "LAGCOV_PADW", "LOWPASS_PADW", "GW_T",
             "KRYLOV_MAX_ORDER", "C64_IT_MIN", "C64_IT_CAP")


@functools.lru_cache(maxsize=1)
def _load():
    d = tempfile.mkdtemp(prefix="plans_shim")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "plans_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "plans_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    for name, (res, args) in SIGNATURES.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


def lib():
    if not CXX:
        pytest.skip("no host C++ compiler")
    return _load()


def constants(lib):
    out = np.zeros(len(CONSTANTS), np.int32)
    lib.pl_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, out.tolist()))
