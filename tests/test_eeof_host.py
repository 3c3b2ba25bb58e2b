"""CPU tests of xeofs_amd.single.ExtendedEOF: the constructor mirrors the reference's (xeofs/single/eeof.py:60-114), argument
checks fire before any device work, transform is refused, and the lag entries are part of the C ABI."""

import inspect

import numpy as np
import pytest

from test_abi import header_symbols


def test_constructor_matches_reference():
    from xeofs_amd.single import ExtendedEOF

    ref = [("n_modes", inspect.Parameter.empty), ("tau", inspect.Parameter.empty), ("embedding", inspect.Parameter.empty),
           ("n_pca_modes", None), ("center", True), ("standardize", False), ("use_coslat", False), ("check_nans", True),
           ("sample_name", "sample"), ("feature_name", "feature"), ("compute", True), ("solver", "auto"),
           ("random_state", None), ("solver_kwargs", {}), ("kwargs", inspect.Parameter.empty)]
    params = inspect.signature(ExtendedEOF.__init__).parameters
    got = [(name, p.default) for name, p in params.items() if name != "self"]
    assert got == ref


def test_get_params_and_attrs():
    from xeofs_amd.single import ExtendedEOF

    m = ExtendedEOF(n_modes=5, tau=2, embedding=3, n_pca_modes=7, solver="randomized", random_state=1)
    p = m.get_params()
    assert (p["tau"], p["embedding"], p["n_pca_modes"], p["solver"]) == (2, 3, 7, "randomized")
    assert p["n_modes"] == 5 and p["random_state"] == 1
    assert m.attrs["model"] == "Extended EOF Analysis"
    assert ExtendedEOF(n_modes=2, tau=1, embedding=2).get_params()["n_pca_modes"] is None


@pytest.mark.parametrize("kw", [dict(tau=0, embedding=2), dict(tau=-1, embedding=2), dict(tau=1, embedding=0),
                                dict(tau=1.5, embedding=2), dict(tau=1, embedding=True), dict(tau=1, embedding=2, n_pca_modes=0)])
def test_bad_arguments_raise(kw):
    from xeofs_amd.single import ExtendedEOF

    with pytest.raises(ValueError):
        ExtendedEOF(n_modes=2, **kw)


def test_too_short_series_raises_before_device_work():
    import xeofs_amd as xe

    X = xe.DataArray(np.zeros((10, 3, 4)), dims=("time", "lat", "lon"))
    m = xe.single.ExtendedEOF(n_modes=2, tau=3, embedding=4)        # n' = 10 - 9 = 1
    with pytest.raises(ValueError, match="the data have 10"):
        m.fit(X, "time")
    with pytest.raises(ValueError, match="the data have 3"):
        xe.single.ExtendedEOF(n_modes=2, tau=1, embedding=3).fit(X, "lat")    # n = 3 samples along lat, n' = 1


def test_transform_not_supported():
    import xeofs_amd as xe

    with pytest.raises(NotImplementedError, match="EEOF does currently not support transform"):
        xe.single.ExtendedEOF(n_modes=2, tau=1, embedding=2).transform(None)


def test_lag_entries_in_abi():
    from xeofs_amd import _lib

    names = ("eofx_lag_stats_f64", "eofx_lag_tmul_f32", "eofx_lag_mul_f32", "eofx_lag_embed_f32")
    syms = header_symbols()
    lib = _lib.load()
    for s in names:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)
    assert set(syms) == set(_lib.SIGNATURES)
    assert lib.eofx_abi_version() == 1
