"""Builds tests/planes_shim.cpp (the plane layout of eofx_plans.hpp and the sketch generator with its memo, eofx_sketch.hpp) with the
host C++ compiler: as a shared object loaded through ctypes (`lib()`, once per session) and as its stand-alone program
(`build_program`, optionally under a sanitizer).  `lib()` skips the calling test when there is no compiler."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
I, I64, P, U32 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32

SIGNATURES = {
    "ps_plane_offset": (I64, [I64, I64, I64, I, I]), "ps_planes_bytes": (I64, [I64, I]), "ps_constants": (None, [P]),
    "ps_sketch": (None, [U32, I64, I64, P]), "ps_sketch_draw": (None, [U32, I64, I64, P]), "ps_sketch_drop": (None, []),
    "ps_sketch_cached": (I, [U32, I64, I64]), "ps_sketch_memo_max_bytes": (I64, []),
}


@functools.lru_cache(maxsize=1)
def _tmpdir():
    d = tempfile.mkdtemp(prefix="planes_shim")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _compile(out, extra):
    cmd = [CXX, "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "planes_shim.cpp"), "-o", out] + extra
    return subprocess.run(cmd, capture_output=True, text=True)


@functools.lru_cache(maxsize=1)
def _load():
    so = os.path.join(_tmpdir(), "planes_shim.so")
    r = _compile(so, ["-shared", "-fPIC"])
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


def build_program(name, flags):
    """the stand-alone program (-DPLANES_SHIM_MAIN) with extra compiler flags -> (path, None) or (None, compiler message)"""
    if not CXX:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(_tmpdir(), name)
    r = _compile(exe, ["-DPLANES_SHIM_MAIN", "-g"] + list(flags))
    return (exe, None) if r.returncode == 0 else (None, r.stderr[-2000:])
