"""The memo of the sketch generator (eofx_sketch.hpp: the last matrix drawn from (seed, rows, cols) is kept, one entry for the
process, and a repeated call copies it out): same bits as a fresh draw and as numpy's legacy stream, no confusion between
keys, the drop call, the size cap, concurrent callers -- and the stand-alone program of tests/planes_shim.cpp under the thread
and address sanitizers.  No GPU, no engine library."""
import platform
import shutil
import subprocess
import threading

import numpy as np
import pytest

import planes_shim


@pytest.fixture(scope="module")
def lib():
    return planes_shim.lib()


def sketch(lib, seed, shape, fn="ps_sketch"):
    out = np.full(shape, np.nan, np.float32)
    getattr(lib, fn)(seed, shape[0], shape[1], out.ctypes.data)
    return out


def reference(seed, shape):
    return np.random.RandomState(seed).normal(size=shape).astype(np.float32)


def test_repeated_call_returns_the_same_bits(lib):
    lib.ps_sketch_drop()
    shape = (1001, 61)          # an odd total: the cached second deviate of the polar method
    a = sketch(lib, 77, shape)
    assert lib.ps_sketch_cached(77, *shape) == 1
    b = sketch(lib, 77, shape)
    ref = reference(77, shape)
    assert np.array_equal(a.view(np.uint32), ref.view(np.uint32)) and np.array_equal(b.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(sketch(lib, 77, shape, "ps_sketch_draw"), ref)


@pytest.mark.parametrize("seed, shape", [(78, (1001, 61)), (77, (1000, 61)), (77, (1001, 60)), (77, (61, 1001))])
def test_another_key_is_drawn_afresh(lib, seed, shape):
    """a different seed, row count, column count, and the transposed shape (same total): never the cached matrix"""
    lib.ps_sketch_drop()
    first = sketch(lib, 77, (1001, 61))
    got = sketch(lib, seed, shape)
    assert np.array_equal(got, reference(seed, shape))
    assert lib.ps_sketch_cached(seed, *shape) == 1 and lib.ps_sketch_cached(77, 1001, 61) == 0      # one entry: the last one
    assert np.array_equal(sketch(lib, 77, (1001, 61)), first)


def test_drop_empties_the_cache(lib):
    shape = (300, 20)
    a = sketch(lib, 3, shape)
    assert lib.ps_sketch_cached(3, *shape) == 1
    lib.ps_sketch_drop()
    assert lib.ps_sketch_cached(3, *shape) == 0
    assert np.array_equal(sketch(lib, 3, shape), a) and lib.ps_sketch_cached(3, *shape) == 1
    lib.ps_sketch_drop()
    lib.ps_sketch_drop()        # dropping an empty cache is fine


def test_nothing_above_the_cap_is_kept(lib):
    assert lib.ps_sketch_memo_max_bytes() == 64 << 20
    lib.ps_sketch_drop()
    rows, cols = (64 << 20) // 4 // 64 + 1, 64          # one row more than 64 MiB of float32
    out = np.empty((rows, cols), np.float32)
    lib.ps_sketch(9, rows, cols, out.ctypes.data)
    assert lib.ps_sketch_cached(9, rows, cols) == 0
    assert np.array_equal(out[:50], reference(9, (50, cols)))          # (numpy fills row by row: the leading rows are the smaller draw)
    del out
    small = sketch(lib, 9, (10, 64))
    assert lib.ps_sketch_cached(9, 10, 64) == 1 and np.array_equal(small, reference(9, (10, 64)))
    lib.ps_sketch_drop()


def test_empty_matrix_touches_nothing(lib):
    lib.ps_sketch_drop()
    keep = sketch(lib, 4, (8, 8))
    guard = np.full(4, 7.0, np.float32)
    lib.ps_sketch(1, 0, 4, guard.ctypes.data)
    lib.ps_sketch(1, 4, 0, guard.ctypes.data)
    assert np.all(guard == 7.0) and lib.ps_sketch_cached(4, 8, 8) == 1
    assert np.array_equal(sketch(lib, 4, (8, 8)), keep)


def test_eight_threads_two_alternating_keys(lib):
    keys = [(5, (700, 60)), (6, (333, 61))]
    refs = [reference(s, sh) for s, sh in keys]
    wrong = []

    def run(t):
        for it in range(10):
            i = (t + it) & 1
            got = sketch(lib, *keys[i])          # (ctypes releases the GIL during the call)
            if not np.array_equal(got.view(np.uint32), refs[i].view(np.uint32)):
                wrong.append((t, it))
            if t == 3 and it % 4 == 3:
                lib.ps_sketch_drop()

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not wrong, wrong


@pytest.mark.parametrize("name, flags", [("plain", []), ("tsan", ["-fsanitize=thread"]), ("asan", ["-fsanitize=address,undefined"])])
def test_standalone_program(name, flags):
    """the generator, its memo and the layout function as a program of their own -- the form a sanitizer can check (nothing is
    loaded into Python): eight threads, two alternating keys, drops in between"""
    exe, msg = planes_shim.build_program("planes_shim_" + name, flags)
    if exe is None and flags:
        pytest.skip("the toolchain does not build with " + " ".join(flags) + ": " + msg[-300:])
    assert exe is not None, msg
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if flags and r.returncode != 0 and not r.stdout and ("unexpected memory mapping" in r.stderr or "Shadow memory range interleaves" in r.stderr):
        # the sanitizer's runtime could not lay out its shadow memory under this kernel's address-space randomisation and left
        # before main(): once more with the randomisation off for this one process, where the host allows that
        setarch = shutil.which("setarch")
        if setarch:
            r = subprocess.run([setarch, platform.machine(), "-R", exe], capture_output=True, text=True, timeout=300)
        if r.returncode != 0 and not r.stdout:
            pytest.skip("the sanitizer runtime does not start on this host: " + r.stderr[-200:])
    assert r.returncode == 0 and "planes_shim: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
