"""Host-side checks of trend EOF analysis (xeofs_amd.single.TrendEOF) that need no GPU: the constructor, the argument checks
that run before any context exists, the closed-form total variance, and the two new symbols in the header and the ctypes
table."""

import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, TrendEOF

    assert xe.single.TrendEOF is TrendEOF and issubclass(TrendEOF, EOF)
    assert list(inspect.signature(TrendEOF.__init__).parameters) == list(inspect.signature(EOF.__init__).parameters)
    m = TrendEOF(n_modes=3, standardize=True, use_coslat=True, random_state=7, solver="full")
    prm = m.get_params()
    assert prm["n_modes"] == 3 and prm["standardize"] is True and prm["use_coslat"] is True and prm["random_state"] == 7
    assert prm["solver"] == "full" and prm["solver_kwargs"] == {}
    assert m.attrs["model"] == "Trend EOF analysis"
    assert m.ctx is None                                       # nothing touched a device
    assert not m.preprocessor.masked_ok                        # a land mask is compacted, not kept as zero columns


def test_argument_checks_without_a_context():
    import xeofs_amd as xe
    from xeofs_amd.single import TrendEOF

    m = TrendEOF(n_modes=2)
    with pytest.raises(NotImplementedError, match="not an orthogonal expansion"):
        m.inverse_transform(None)
    X = np.zeros((6, 4), dtype=np.complex64)
    with pytest.raises(TypeError, match="complex"):
        m.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(6), "x": np.arange(4)}), dim="time")
    assert m.ctx is None                                       # refused before a context is bound


def test_limits_and_closed_form():
    from xeofs_amd import engine
    from xeofs_amd.single import trend_eof

    assert trend_eof.MAX_SAMPLES == engine.ORDERPOS_NMAX == 16384
    w = np.array([1.0, 0.5, 2.0])
    assert trend_eof.trend_total_variance(10, w) == 10 * 11 / 12.0 * 5.25
    # the variance (ddof = 1) of any permutation of 0 .. n - 1
    for n in (2, 7, 100):
        assert np.isclose(np.var(np.random.default_rng(n).permutation(n), ddof=1), trend_eof.trend_total_variance(n, [1.0]),
                          rtol=1e-13)


def test_want_is_checked_before_anything_else():
    from xeofs_amd import engine

    with pytest.raises(ValueError, match="want"):
        engine.order_positions(None, None, want="ranks")


def test_new_symbols_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    for s in ("eofx_orderpos_f32", "eofx_mat_orderpos_f32"):
        assert s in syms and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["eofx_orderpos_f32"][1]) == 10
    assert len(_lib.SIGNATURES["eofx_mat_orderpos_f32"][1]) == 4
    lib = _lib.load()
    assert hasattr(lib, "eofx_orderpos_f32") and hasattr(lib, "eofx_mat_orderpos_f32")
    assert lib.eofx_abi_version() == 1
