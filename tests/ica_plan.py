"""The launch plan of csrc/eofx_ica.hpp for the tests: tests/ica_shim.cpp compiled with the host C++ compiler and loaded through
ctypes.  plan(n, q) -> dict(blocks, rows, qp, qw, slot, lds); scratch(n, q, R) -> float64 words."""

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
CONSTANTS = ("ICA_QMAX", "ICA_NMAX", "ICA_RMAX", "ICA_ITER_MAX", "ICA_WG", "ICA_BMAX")
FIELDS = ("blocks", "rows", "qp", "qw", "slot", "lds")


@functools.lru_cache(maxsize=1)
def _shim():
    d = tempfile.mkdtemp(prefix="ica_shim")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "ica_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "ica_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for name, (res, args) in {"ica_constants": (None, [P]), "ica_plan": (None, [I64, I, P]), "ica_scratch": (I64, [I64, I, I64])}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def shim():
    if not CXX:
        pytest.skip("no host C++ compiler")
    return _shim()


def constants() -> dict:
    out = np.zeros(len(CONSTANTS), np.int32)
    shim().ica_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, (int(v) for v in out)))


def plan(n: int, q: int) -> dict:
    out = np.zeros(len(FIELDS), np.int64)
    shim().ica_plan(n, q, out.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in out)))


def scratch(n: int, q: int, R: int) -> int:
    return int(shim().ica_scratch(n, q, R))
