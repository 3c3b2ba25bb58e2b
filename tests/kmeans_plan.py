"""The launch plan of csrc/eofx_kmeans.hpp for the tests: tests/kmeans_shim.cpp compiled with the host C++ compiler and loaded
through ctypes.  plan(n, q, k, R) -> dict(grid, threads, qp, groups, rpt, the LDS offsets, lds)."""

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
CONSTANTS = ("KMEANS_KMAX", "KMEANS_QMAX", "KMEANS_NMAX", "KMEANS_RMAX", "KMEANS_ITER_MAX", "KMEANS_WG", "KMEANS_ACC_MAX",
             "KMEANS_RED_BYTES")
FIELDS = ("grid", "threads", "qp", "groups", "rpt", "acc_off", "c_off", "stage_off", "cnt_off", "lab_off", "lds")


@functools.lru_cache(maxsize=1)
def _shim():
    d = tempfile.mkdtemp(prefix="kmeans_shim")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "kmeans_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "kmeans_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for name, (res, args) in {"km_constants": (None, [P]), "km_plan": (None, [I64, I, I, I64, P])}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def shim():
    if not CXX:
        pytest.skip("no host C++ compiler")
    return _shim()


def constants() -> dict:
    out = np.zeros(len(CONSTANTS), np.int32)
    shim().km_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, (int(v) for v in out)))


def plan(n: int, q: int, k: int, R: int) -> dict:
    out = np.zeros(len(FIELDS), np.int64)
    shim().km_plan(n, q, k, R, out.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in out)))
