"""The launch plan of csrc/eofx_simplex.hpp for the tests: tests/simplex_shim.cpp compiled with the host C++ compiler and loaded
through ctypes.  plan(r, m) -> dict(tier, lanes, epl, threads, rpb, grid, lds); the GPU tests read the tier boundary from it."""

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
CONSTANTS = ("SIMPLEX_MMAX", "SIMPLEX_KMAX", "SIMPLEX_REG_MMAX", "SIMPLEX_WG", "SIMPLEX_PG_WG")
FIELDS = ("tier", "lanes", "epl", "threads", "rpb", "grid", "lds")


@functools.lru_cache(maxsize=1)
def _shim():
    d = tempfile.mkdtemp(prefix="simplex_shim")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "simplex_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "simplex_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for name, (res, args) in {"sx_constants": (None, [P]), "sx_plan": (None, [I64, I64, P]), "sx_pg_width": (I, [I])}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def shim():
    if not CXX:
        pytest.skip("no host C++ compiler")
    return _shim()


def constants() -> dict:
    out = np.zeros(len(CONSTANTS), np.int32)
    shim().sx_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, (int(v) for v in out)))


def plan(r: int, m: int) -> dict:
    out = np.zeros(len(FIELDS), np.int64)
    shim().sx_plan(r, m, out.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in out)))


def tier_boundary() -> int:
    """the longest row of tier 0, found from the plan itself"""
    lo, hi = 1, constants()["SIMPLEX_MMAX"]
    assert plan(1, lo)["tier"] == 0 and plan(1, hi)["tier"] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(1, mid)["tier"] == 0:
            lo = mid
        else:
            hi = mid
    return lo
