"""The host setup of the Hilbert stage (xeofs_amd/csrc/eofx_hilbert_host.hpp) without a GPU: plain C++ compiled into
tests/plans_shim.cpp with the host compiler and called through ctypes.  References: numpy's FFT in float64, the closed form of the
filter's frequency response (-i sgn k), and the oracle's Hilbert stage (oracle/eof_oracle.py, the reference's own steps in float64
numpy) for the operator."""
import ctypes

import numpy as np
import pytest

import plans_shim
from oracle import eof_oracle as orc

E32 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return plans_shim.lib()


def kappa(N, d):
    """the impulse response as the header's comment states it, in numpy"""
    d = np.asarray(d, np.int64)
    x = np.pi * d / N
    with np.errstate(divide="ignore", invalid="ignore"):
        if N % 2 == 0:
            out = np.where(d % 2 == 1, (2.0 / N) / np.tan(x), 0.0)
        else:
            out = (1.0 / np.tan(x) - np.where(np.abs(d) % 2 == 1, -1.0, 1.0) / np.sin(x)) / N
    return np.where(d % N == 0, 0.0, out)


def embedded_kernel(n, N, P):
    """lags -(n - 1) .. n - 1 of the kernel of period N on a circle of P points, 1 / P of the unnormalised inverse folded in"""
    c = np.zeros(P)
    d = np.arange(-(n - 1), n)
    c[d % P] = kappa(N, d) / P
    return c


@pytest.mark.parametrize("N", [2, 8, 1024])
def test_host_fft(lib, N):
    rng = np.random.default_rng(N)
    a = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    got = a.copy()
    lib.hh_fft(got.ctypes.data, N)
    ref = np.fft.fft(a)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("N", [2, 8, 300, 3, 9, 301])
def test_kappa_is_the_hilbert_filter(lib, N):
    """the DFT of kappa over one period is -i sgn(k): zero at k = 0 and at the Nyquist frequency; the header's values are the
    closed form's, also at lags outside one period and at negative ones"""
    d = np.arange(-2 * N, 2 * N + 1)
    got = np.array([lib.hh_kappa(N, int(x)) for x in d])
    assert np.abs(got - kappa(N, d)).max() <= 1e-13 * max(np.abs(got).max(), 1.0)
    one = np.array([lib.hh_kappa(N, int(x)) for x in range(N)])
    k = np.arange(N)
    sgn = np.where(k == 0, 0.0, np.where(2 * k < N, 1.0, np.where(2 * k == N, 0.0, -1.0)))
    assert np.abs(np.fft.fft(one) - (-1j * sgn)).max() <= 1e-12 * N


def _frequencies(lib, L, count):
    k = np.array([lib.hh_position_frequency(L, pos) for pos in range(count)])
    assert np.array_equal(np.sort(k), np.arange(count))        # a permutation of the frequencies
    return k


@pytest.mark.parametrize("n, padding", [(300, 1), (512, 0), (513, 1), (1000, 0)])
def test_permuted_filter_table(lib, n, padding):
    """L = 10 and 11: the table, un-permuted with position_frequency, is Im of np.fft.fft of the embedded kernel to float32
    rounding (the spectrum of a real odd sequence is purely imaginary)"""
    L = ctypes.c_int()
    P = lib.hh_length(n, ctypes.addressof(L))
    assert P == 1 << L.value and P >= 2 * n and L.value == (10 if n <= 512 else 11)
    N = 3 * n if padding else n
    table = np.zeros(P, np.float32)
    lib.hh_fused_table(n, N, L.value, table.ctypes.data)
    spec = np.fft.fft(embedded_kernel(n, N, P))
    assert np.abs(spec.real).max() <= 1e-12 * np.abs(spec).max()
    h = spec.imag[_frequencies(lib, L.value, P)]
    assert np.all(np.abs(table - h) <= E32 * np.abs(h) + 1e-12 * np.abs(h).max())
    circ = np.zeros(P + 2, np.float32)
    lib.hh_circular_kernel(n, N, P, circ.ctypes.data)
    assert np.array_equal(circ[:P], embedded_kernel(n, N, P).astype(np.float32)) and not circ[P:].any()


def test_split_merge_filter_tables(lib):
    """L = 15: with M = P / 2 and k the frequency at position pos of the half-length transform, the first table is
    hm = h[k] - h[M - k] and the second hp2 = (h[k] + h[M - k]) / 2, with h[M] = 0 standing in at k = 0"""
    n, L = 9000, 15
    P, M, N = 1 << L, 1 << (L - 1), 3 * n
    lv = ctypes.c_int()
    assert lib.hh_length(n, ctypes.addressof(lv)) == P and lv.value == L
    table = np.zeros(P, np.float32)
    lib.hh_fused_table(n, N, L, table.ctypes.data)
    h = np.fft.fft(embedded_kernel(n, N, P)).imag
    k = _frequencies(lib, L - 1, M)
    hk, hkp = h[k], np.where(k == 0, 0.0, h[(M - k) % P])
    scale = 1e-12 * np.abs(h).max()
    assert np.all(np.abs(table[:M] - (hk - hkp)) <= E32 * np.abs(hk - hkp) + scale)
    assert np.all(np.abs(table[M:] - 0.5 * (hk + hkp)) <= E32 * np.abs(0.5 * (hk + hkp)) + scale)


@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_correction_vector_layouts(lib, n):
    """the float32 tables of the two device routes are the float64 vectors [4][n] rounded: as they are, or interleaved per sample
    and followed by the four means of the ROUNDED values"""
    N = 3 * n
    u = np.zeros((4, n))
    lib.hh_pad_vectors(n, N, 0.2, u.ctypes.data)
    plain, inter = np.zeros(4 * n + 4, np.float32), np.zeros(4 * n + 4, np.float32)
    lib.hh_pad_table(n, N, 0.2, 0, plain.ctypes.data)
    lib.hh_pad_table(n, N, 0.2, 1, inter.ctypes.data)
    u32 = u.astype(np.float32)
    assert np.array_equal(plain[:4 * n].reshape(4, n), u32) and not plain[4 * n:].any()
    assert np.array_equal(inter[:4 * n].reshape(n, 4), u32.T)
    assert np.array_equal(inter[4 * n:], (u32.astype(np.float64).sum(axis=1) / n).astype(np.float32))


@pytest.mark.parametrize("n", [1, 2, 7, 300])
@pytest.mark.parametrize("padding", ["exp", None])
def test_hilbert_operator(lib, n, padding):
    """H x for the n x n operator is the imaginary part of the oracle's Hilbert transform of x, for random and for constant
    series, to 2e-5 of the series' scale: the tolerance of tests/test_gpu_panel_helpers.py::test_hilbert_operator"""
    H = np.full((n, n), np.nan, np.float32)
    assert lib.hh_operator(n, int(padding == "exp"), 0.2, H.ctypes.data) == 0
    H = H.astype(np.float64)
    rng = np.random.default_rng(n)
    x = np.concatenate([rng.standard_normal((n, 5)), np.full((n, 1), 3.5), np.full((n, 1), -250.0)], axis=1)
    ref = orc.hilbert_transform(x, padding=padding, decay_factor=0.2).imag
    scale = np.abs(x).max(0)
    assert np.all(np.abs(H @ x - ref) <= 2e-5 * scale[None, :])
