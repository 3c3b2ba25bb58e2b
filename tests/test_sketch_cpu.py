"""The Gaussian sketch generator (xeofs_amd/csrc/eofx_sketch.hpp) without the engine library: the header is plain C++, compiled
into tests/plans_shim.cpp with the host compiler and called through ctypes.  Every matrix is compared BIT FOR BIT with numpy's
legacy stream, np.random.RandomState(seed).normal(size=shape).astype(np.float32) -- what scikit-learn draws for randomized_svd."""
import numpy as np
import pytest

import plans_shim


@pytest.fixture(scope="module")
def lib():
    return plans_shim.lib()


def sketch(lib, seed, shape):
    out = np.full(shape, np.nan, np.float32)
    lib.sk_gaussian_f32(seed, shape[0], shape[1], out.ctypes.data)
    return out


def reference(seed, shape):
    return np.random.RandomState(seed).normal(size=shape).astype(np.float32)


def first_round_accepts(lib, seed, total):
    """(pairs the first round of candidates accepts, pairs needed): the polar method on the header's own candidate count, every
    candidate two 53-bit uniforms of the same stream"""
    need = (total + 1) // 2
    u = np.random.RandomState(seed).random_sample(2 * lib.sk_candidates(need))
    a, b = 2.0 * u[0::2] - 1.0, 2.0 * u[1::2] - 1.0
    r = a * a + b * b
    return int(((r < 1.0) & (r != 0.0)).sum()), need


# the cases of tests/test_abi.py::test_sketch_matrix_is_sklearns: odd totals (the cached second deviate), sizes that span
# MT19937 refills, the multi-threaded tail
@pytest.mark.parametrize("seed, shape", [(42, (50, 12)), (0, (7, 3)), (5, (3000, 60)), (2 ** 32 - 1, (1, 1)), (77, (1001, 61))])
def test_sketch_matrix_is_numpys(lib, seed, shape):
    a = sketch(lib, seed, shape)
    assert np.array_equal(a, reference(seed, shape)), (seed, shape)


def test_empty_sketch_writes_nothing(lib):
    guard = np.full(4, 7.0, np.float32)
    lib.sk_gaussian_f32(1, 0, 4, guard.ctypes.data)
    lib.sk_gaussian_f32(1, 4, 0, guard.ctypes.data)
    assert np.all(guard == 7.0)


# found by scanning seeds 0 .. 3999 with first_round_accepts at totals of 6000 and 10000 deviates (the candidate count asks for
# 1 % + 64 more than the expected need, about three standard deviations at these sizes: a handful of seeds per thousand)
@pytest.mark.parametrize("seed, shape", [(218, (100, 60)), (2170, (1, 9999)), (2119, (2500, 4))])
def test_second_round_of_candidates(lib, seed, shape):
    """the first round accepts fewer pairs than the matrix needs: the generator continues the stream from the state behind the
    first round's words, for an even and for an odd total"""
    got, need = first_round_accepts(lib, seed, shape[0] * shape[1])
    assert got < need, "the case no longer forces a second round: scan for another seed"
    assert np.array_equal(sketch(lib, seed, shape), reference(seed, shape))


def test_thread_count_does_not_change_the_matrix(lib, monkeypatch):
    shape = (3000, 61)
    outs = []
    for threads in ("1", "8", "3"):
        monkeypatch.setenv("EOFX_SKETCH_THREADS", threads)
        outs.append(sketch(lib, 5, shape))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and np.array_equal(outs[0], reference(5, shape))
