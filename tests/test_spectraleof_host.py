"""Host-side checks of the spectral EOF model (xeofs_amd.single.SpectralEOF) that need no GPU: the constructor and every
refusal that runs before a context exists, the GPU-free helpers (the coefficient matrix against numpy.fft.rfft of windowed unit
vectors, the block count, the Hermitian assembly from a designed G, the mode weights, the chunk schedule), the launch plans of
csrc/eofx_spectral.hpp (tests/spectral_shim.cpp, compiled with the host C++ compiler) against the documented rule and against
the model's restatement, and the four new symbols in the header, the ctypes table and the built library."""

import atexit
import ctypes
import functools
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import spectral_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
CONSTANTS = ("BLOCKXFORM_NFFT_MAX", "BLOCKXFORM_NCOEF_MAX", "BLOCKXFORM_TS", "BLOCKXFORM_TC", "BLOCKXFORM_WGS", "BLOCKXFORM_GMAX",
             "ROWGRAM_RMAX", "ROWGRAM_SPAN", "ROWGRAM_SMAX", "ROWGRAM_NBMAX", "SLABMUL_QMAX", "SLABMUL_RMAX", "SLABMUL_NBMAX",
             "SLABMUL_TP")


@functools.lru_cache(maxsize=1)
def _shim():
    d = tempfile.mkdtemp(prefix="spectral_shim")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "spectral_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spectral_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for name, (res, args) in {"sp_constants": (None, [P]), "sp_blockxform_plan": (None, [I64, I64, I64, P]),
                              "sp_rowgram_plan": (None, [I64, I64, I64, P]), "sp_first": (I64, [I64, I, I]),
                              "sp_slabmul_qt": (I, [I64])}.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def shim():
    if not CXX:
        pytest.skip("no host C++ compiler")
    return _shim()


def plan(fn, *args):
    out = np.zeros(3, np.int64)
    fn(*args, out.ctypes.data)
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------ the constructor
def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, SpectralEOF

    assert xe.single.SpectralEOF is SpectralEOF and issubclass(SpectralEOF, EOF)
    extra = ["n_fft", "n_overlap", "window", "sampling_interval", "block_detrend", "freq_chunk"]
    mine, eofs = (list(inspect.signature(c.__init__).parameters) for c in (SpectralEOF, EOF))
    assert [a for a in mine if a not in extra] == eofs and all(a in mine for a in extra)
    sig = inspect.signature(SpectralEOF.__init__).parameters
    assert sig["n_modes"].default == 3 and sig["window"].default == "hamming" and sig["sampling_interval"].default == 1.0
    assert sig["block_detrend"].default is False and sig["freq_chunk"].default is None and sig["n_overlap"].default is None
    m = SpectralEOF(n_fft=64, use_coslat=True)
    prm = m.get_params()
    assert prm["n_modes"] == 3 and prm["n_fft"] == 64 and prm["n_overlap"] == 32 and prm["window"] == "hamming"
    assert prm["use_coslat"] is True and prm["freq_chunk"] is None and prm["block_detrend"] is False
    assert SpectralEOF(n_fft=9).get_params()["n_overlap"] == 4
    assert SpectralEOF(n_fft=9, n_overlap=0).get_params()["n_overlap"] == 0
    assert m.attrs["model"] == "Spectral EOF analysis" and m.attrs["n_fft"] == 64
    assert m.ctx is None and not m.preprocessor.masked_ok
    assert SpectralEOF(n_fft=4, window=[1.0, 2.0, 2.0, 1.0]).attrs["window"] == "custom"


@pytest.mark.parametrize("kw,name", [
    (dict(n_fft=1), "n_fft"), (dict(n_fft=0), "n_fft"), (dict(n_fft=2.0), "n_fft"), (dict(), "n_fft"), (dict(n_fft=2 ** 20), "n_fft"),
    (dict(n_fft=8, n_overlap=8), "n_overlap"), (dict(n_fft=8, n_overlap=-1), "n_overlap"), (dict(n_fft=8, n_overlap=1.5), "n_overlap"),
    (dict(n_fft=8, window="kaiser"), "window"), (dict(n_fft=8, window=np.ones(7)), "window"),
    (dict(n_fft=8, window=np.zeros(8)), "window"), (dict(n_fft=8, window=np.ones((8, 1))), "window"),
    (dict(n_fft=8, window=np.full(8, np.nan)), "window"),
    (dict(n_fft=8, n_modes=0), "n_modes"), (dict(n_fft=8, n_modes=-2), "n_modes"), (dict(n_fft=8, n_modes=1.0), "n_modes"),
    (dict(n_fft=8, n_modes=9), "n_modes"),
    (dict(n_fft=8, sampling_interval=0.0), "sampling_interval"), (dict(n_fft=8, sampling_interval=-1.0), "sampling_interval"),
    (dict(n_fft=8, sampling_interval="1"), "sampling_interval"),
    (dict(n_fft=8, freq_chunk=0), "freq_chunk"), (dict(n_fft=8, freq_chunk=1.5), "freq_chunk"),
])
def test_the_constructor_refuses_and_names_the_argument(kw, name):
    from xeofs_amd.single import SpectralEOF

    with pytest.raises(ValueError, match=name):
        SpectralEOF(**kw)


def test_argument_checks_without_a_context():
    import xeofs_amd as xe
    from xeofs_amd.single import SpectralEOF

    m = SpectralEOF(n_fft=4)
    X = np.zeros((6, 4), dtype=np.complex64)
    with pytest.raises(TypeError, match="This method does not support complex data."):
        m.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(6), "x": np.arange(4)}), dim="time")
    assert m.ctx is None
    with pytest.raises(NotImplementedError):
        m.transform(None)
    with pytest.raises(NotImplementedError):
        m.inverse_transform(None)


# ------------------------------------------------------------------------------------------------ the helpers
@pytest.mark.parametrize("n_fft", [2, 5, 16, 33])
@pytest.mark.parametrize("win", ["hamming", "hann", "boxcar", "custom"])
def test_coefficient_matrix_against_rfft_of_windowed_unit_vectors(n_fft, win):
    from xeofs_amd.single.spectral_eof import coefficient_matrix, onesided_factors, window_values

    rng = np.random.default_rng(n_fft)
    window = rng.uniform(0.1, 1.0, n_fft) if win == "custom" else win
    dt = 0.25
    B = coefficient_matrix(n_fft, window, dt, dtype=np.float64)
    w = window_values(window, n_fft)
    np.testing.assert_allclose(w, sr.window(window, n_fft), rtol=0, atol=1e-15)
    F = np.fft.rfft(np.eye(n_fft) * w[None, :], axis=1).T                # F[k, t] = w_t e^{-2 pi i k t / n_fft}
    s = np.sqrt(onesided_factors(n_fft) * dt / np.sum(w * w))
    assert B.shape == (2 * (n_fft // 2 + 1), n_fft)
    np.testing.assert_allclose(B[0::2], s[:, None] * F.real, rtol=0, atol=1e-14 * np.abs(B).max())
    np.testing.assert_allclose(B[1::2], s[:, None] * F.imag, rtol=0, atol=1e-14 * np.abs(B).max())
    assert np.all(B[1] == 0.0)                                            # the imaginary row of k = 0 is exactly zero
    B32 = coefficient_matrix(n_fft, window, dt)
    assert B32.dtype == np.float32 and np.array_equal(B32, B.astype(np.float32))      # rounded once
    # block_detrend: B (I - 1 1^T / n_fft)
    Bd = coefficient_matrix(n_fft, window, dt, block_detrend=True, dtype=np.float64)
    np.testing.assert_allclose(Bd, B @ (np.eye(n_fft) - np.ones((n_fft, n_fft)) / n_fft), rtol=0, atol=1e-14 * np.abs(B).max())
    # the realisations of a field through B are those of the restatement
    X = rng.standard_normal((3 * n_fft, 4))
    Q = sr.realisations(X, n_fft, n_fft // 2, window, dt)
    Xb = sr.blocks(X, n_fft, n_fft // 2)
    mine = np.einsum("ct,btj->cbj", B, Xb)
    np.testing.assert_allclose(mine[0::2] + 1j * mine[1::2], Q, rtol=0, atol=1e-12 * np.abs(Q).max())


def test_onesided_factors_and_frequencies():
    from xeofs_amd.single.spectral_eof import frequency_axis, onesided_factors

    np.testing.assert_array_equal(onesided_factors(8), [1, 2, 2, 2, 1])
    np.testing.assert_array_equal(onesided_factors(7), [1, 2, 2, 2])
    np.testing.assert_array_equal(onesided_factors(2), [1, 1])
    np.testing.assert_allclose(frequency_axis(8, 0.5), np.fft.rfftfreq(8, 0.5), rtol=1e-15)
    np.testing.assert_allclose(frequency_axis(7, 2.0), np.fft.rfftfreq(7, 2.0), rtol=1e-15)


@pytest.mark.parametrize("n,n_fft,ov,want", [(100, 10, 5, 19), (100, 10, 0, 10), (103, 10, 0, 10), (10, 10, 9, 1), (100, 10, 9, 91),
                                             (11, 10, 9, 2), (400, 64, 32, 11), (2000, 256, 128, 14)])
def test_block_count(n, n_fft, ov, want):
    from xeofs_amd.single.spectral_eof import block_count

    assert block_count(n, n_fft, ov) == want == sr.blocks(np.zeros((n, 1)), n_fft, ov).shape[0]
    assert (want - 1) * (n_fft - ov) + n_fft <= n < want * (n_fft - ov) + n_fft


def test_hermitian_assembly_from_a_designed_gram():
    from xeofs_amd.single.spectral_eof import hermitian_from_gram

    rng = np.random.default_rng(1)
    nblk, p = 4, 9
    Q = rng.integers(-3, 4, (2, nblk, p)) + 1j * rng.integers(-3, 4, (2, nblk, p))
    R = np.concatenate([Q.real, Q.imag], axis=1)                           # [2 x 2 nblk x p]
    G = R @ np.transpose(R, (0, 2, 1))
    M = hermitian_from_gram(G, nblk)
    assert M.shape == (2, nblk, nblk) and M.dtype == np.complex128
    np.testing.assert_array_equal(M, sr.snapshot_matrix(Q))               # integers: exact
    np.testing.assert_array_equal(M, np.conj(np.transpose(M, (0, 2, 1))))
    with pytest.raises(ValueError, match="G must be"):
        hermitian_from_gram(G, 3)


def test_mode_weights_give_orthonormal_modes_and_mark_unresolved_ones():
    from xeofs_amd.single.spectral_eof import eig_descending, mode_weights, resolved_modes

    rng = np.random.default_rng(2)
    nblk, p, K = 5, 40, 3
    Q = rng.standard_normal((nblk, p)) + 1j * rng.standard_normal((nblk, p))
    M = np.conj(Q) @ Q.T / nblk
    lam, Th = eig_descending(M)
    assert np.all(np.diff(lam) <= 0)
    W = mode_weights(lam, Th, K)
    assert W.shape == (2 * K, 2 * nblk)
    out = W @ np.concatenate([Q.real, Q.imag], axis=0)
    Phi = (out[:K] + 1j * out[K:]).T
    np.testing.assert_allclose(np.conj(Phi.T) @ Phi, np.eye(K), atol=1e-12)
    np.testing.assert_allclose(Phi, Q.T @ (Th[:, :K] / np.sqrt(lam[:K] * nblk)), atol=1e-12)
    # two independent blocks out of five: modes 3 .. 5 are not resolved
    Q2 = np.concatenate([Q[:2], Q[:1] * 2, Q[1:2] * -1, Q[:1] + Q[1:2]], axis=0)
    lam2, Th2 = eig_descending(np.conj(Q2) @ Q2.T / nblk)
    ok = resolved_modes(lam2, nblk)
    np.testing.assert_array_equal(ok, [True, True, False, False, False])
    W2 = mode_weights(lam2, Th2, 3)
    assert np.all(W2[[2, 5]] == 0.0) and np.all(np.isfinite(W2))
    assert not resolved_modes(np.zeros(4), 4).any()                        # an empty frequency resolves nothing


def test_chunk_schedule_and_auto_chunk():
    from xeofs_amd.single.spectral_eof import auto_chunk, chunk_schedule

    assert chunk_schedule(5, 2) == [(0, 2), (2, 4), (4, 5)]
    assert chunk_schedule(5, 1) == [(k, k + 1) for k in range(5)]
    assert chunk_schedule(5, 5) == chunk_schedule(5, 99) == [(0, 5)]
    assert chunk_schedule(129, 64) == [(0, 64), (64, 128), (128, 129)]
    with pytest.raises(ValueError, match="freq_chunk"):
        chunk_schedule(5, 0)
    per = 4 * (2 * 14 + 6 * 3) * 129600
    assert auto_chunk(129, 14, 129600, 3, 4 * per * 129) == 129           # everything fits: one chunk
    assert auto_chunk(129, 14, 129600, 3, 4 * per * 100) == 64            # whole tiles of 64 frequencies
    assert auto_chunk(129, 14, 129600, 3, 4 * per * 63) == 63
    assert auto_chunk(129, 14, 129600, 3, 0) == 1


# ------------------------------------------------------------------------------------------------ the plans
def test_the_constants_are_those_the_engine_states():
    from xeofs_amd import engine

    lib = shim()
    out = np.zeros(len(CONSTANTS), np.int32)
    lib.sp_constants(out.ctypes.data)
    c = dict(zip(CONSTANTS, out.tolist()))
    assert c["BLOCKXFORM_NFFT_MAX"] == engine.BLOCKXFORM_NFFT_MAX and c["BLOCKXFORM_NCOEF_MAX"] == engine.BLOCKXFORM_NCOEF_MAX
    assert c["ROWGRAM_RMAX"] == engine.ROWGRAM_RMAX >= 512 and c["ROWGRAM_SPAN"] == engine.ROWGRAM_SPAN == 2048
    assert c["SLABMUL_QMAX"] == engine.SLABMUL_QMAX and c["SLABMUL_RMAX"] == c["ROWGRAM_RMAX"]
    assert c["ROWGRAM_NBMAX"] == c["SLABMUL_NBMAX"] == engine.SPECTRAL_NBMAX == c["BLOCKXFORM_GMAX"] == 65535
    assert c["BLOCKXFORM_TS"] == c["BLOCKXFORM_TC"] == 128 and c["BLOCKXFORM_WGS"] == 1024 and c["ROWGRAM_SMAX"] == 16
    assert c["SLABMUL_TP"] == 512
    assert c["SLABMUL_RMAX"] * 16 * 4 <= 65536                             # W[f] transposed fits the LDS of a workgroup


def test_blockxform_plan_against_the_documented_rule():
    from xeofs_amd.single import spectral_eof as se

    lib = shim()
    for p in (1, 127, 128, 129, 257, 129600, 10 ** 6):
        for ncoef in (1, 2, 128, 129, 258, 8192):
            for nblk in (1, 2, 14, 171, 400, 10 ** 5):
                st, ct, g = plan(lib.sp_blockxform_plan, p, ncoef, nblk)
                assert st == -(-p // 128) and ct == -(-ncoef // 128)
                assert g == max(1, min(-(-1024 // (st * ct)), nblk, 65535))
                assert (st, ct, g) == se.blockxform_plan(p, ncoef, nblk)
                # the groups tile the blocks: ascending, none empty, none lost
                firsts = [lib.sp_first(nblk, g, z) for z in range(g + 1)]
                assert firsts[0] == 0 and firsts[-1] == nblk and all(b > a for a, b in zip(firsts, firsts[1:]))
    assert plan(lib.sp_blockxform_plan, 129600, 128, 14) == (1013, 1, 2)
    assert plan(lib.sp_blockxform_plan, 257, 130, 400) == (3, 2, 171)


def test_rowgram_plan_against_the_documented_rule():
    from xeofs_amd.single import spectral_eof as se

    lib = shim()
    for r, pairs in ((1, 1), (28, 1), (128, 1), (129, 3), (256, 3), (257, 6), (384, 6), (385, 10), (512, 10)):
        for p in (1, 2047, 2048, 2049, 16 * 2048, 16 * 2048 + 1, 129600):
            got = [plan(lib.sp_rowgram_plan, r, p, nb) for nb in (1, 3, 129)]
            assert got[0] == got[1] == got[2]                              # the split does not depend on the batch
            rt, spans, splits = got[0]
            assert rt == -(-r // 128) and rt * (rt + 1) // 2 == pairs and spans == -(-p // 2048)
            assert splits == max(1, min(16 // pairs, spans))
            assert got[0] == se.rowgram_plan(r, p, 1)
            firsts = [lib.sp_first(spans, splits, z) for z in range(splits + 1)]
            assert firsts[0] == 0 and firsts[-1] == spans and all(b > a for a, b in zip(firsts, firsts[1:]))
            assert 3 * splits * r * r * 8 <= 3 * (2 ** 21 + 2 ** 19)      # the partials: about 2 MiB a slab at the most
    assert [lib.sp_slabmul_qt(q) for q in (1, 6, 8, 9, 16)] == [8, 8, 8, 16, 16]


# ------------------------------------------------------------------------------------------------ the layers
def test_engine_entries():
    from xeofs_amd import engine

    assert list(inspect.signature(engine.blockxform).parameters) == ["ctx", "T", "B", "hop", "nblk", "out"]
    assert list(inspect.signature(engine.mat_blockxform).parameters) == ["ctx", "mat", "B", "hop", "nblk", "out"]
    assert list(inspect.signature(engine.rowgram).parameters) == ["ctx", "R", "out"]
    assert list(inspect.signature(engine.slabmul).parameters) == ["ctx", "W", "R", "out"]


def test_new_symbols_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    want = {"eofx_blockxform_f32": 12, "eofx_mat_blockxform_f32": 9, "eofx_rowgram_f32": 6, "eofx_slabmul_f32": 8}
    lib = _lib.load()
    for s, nargs in want.items():
        assert s in syms and s in _lib.SIGNATURES and len(_lib.SIGNATURES[s][1]) == nargs and hasattr(lib, s)
    assert lib.eofx_abi_version() == 1
