"""CPU tests of xeofs_amd.single.GWPCA: the constructor mirrors the reference's (xeofs/single/gwpca.py:87-126), its
argument checks (tests/models/single/test_gwpca.py), the discovery of the sample coordinates by name, and the new C ABI
entries."""

import inspect

import numpy as np
import pytest

from test_abi import header_symbols


def test_constructor_matches_reference():
    from xeofs_amd.single import GWPCA

    ref = [("n_modes", inspect.Parameter.empty), ("bandwidth", inspect.Parameter.empty), ("metric", "haversine"),
           ("kernel", "bisquare"), ("center", True), ("standardize", False), ("use_coslat", False), ("check_nans", True),
           ("sample_name", "sample"), ("feature_name", "feature")]
    params = inspect.signature(GWPCA.__init__).parameters
    assert [(name, p.default) for name, p in params.items() if name != "self"] == ref


def test_get_params_and_attrs():
    from xeofs_amd.single import GWPCA

    m = GWPCA(n_modes=3, bandwidth=500.0, metric="euclidean", kernel="gaussian", standardize=True)
    p = m.get_params()
    assert (p["n_modes"], p["bandwidth"], p["metric"], p["kernel"], p["standardize"]) == (3, 500.0, "euclidean", "gaussian", True)
    assert m.attrs["model"] == "GWPCA"
    assert (m.bandwidth, m.metric, m.kernel) == (500.0, "euclidean", "gaussian")


@pytest.mark.parametrize("metric, kernel, bandwidth", [("haversine", "invalid_kernel", 5000), ("invalid_metric", "gaussian", 5000),
                                                       ("haversine", "exponential", 0)])
def test_invalid_arguments(metric, kernel, bandwidth):
    from xeofs_amd.single import GWPCA

    with pytest.raises(ValueError):
        GWPCA(n_modes=2, metric=metric, kernel=kernel, bandwidth=bandwidth)


def test_coordinates_two_sample_dims_by_name():
    import xeofs_amd as xe
    from xeofs_amd.single.gwpca import sample_coordinates

    lat, lon = np.array([-10.0, 0.0, 10.0]), np.array([100.0, 110.0])
    X = xe.DataArray(np.zeros((4, 3, 2)), dims=("time", "lat", "lon"), coords={"lat": lat, "lon": lon})
    a = sample_coordinates(X, ("lat", "lon"))           # stacked order lat-major, columns (lon, lat)
    assert a.shape == (6, 2)
    np.testing.assert_array_equal(a[:, 0], np.tile(lon, 3))
    np.testing.assert_array_equal(a[:, 1], np.repeat(lat, 2))
    b = sample_coordinates(X, ("lon", "lat"))           # stacked order lon-major, still (lon, lat)
    np.testing.assert_array_equal(b[:, 0], np.repeat(lon, 3))
    np.testing.assert_array_equal(b[:, 1], np.tile(lat, 2))
    Y = xe.DataArray(np.zeros((4, 3, 2)), dims=("time", "u", "v"))
    c = sample_coordinates(Y, ("u", "v"))               # no name recognised: dims order
    np.testing.assert_array_equal(c[:, 0], np.repeat(np.arange(3.0), 2))


def test_coordinates_one_sample_dim():
    import xeofs_amd as xe
    from xeofs_amd.single.gwpca import sample_coordinates

    x, y = np.arange(5.0), np.arange(5.0) * 2
    X = xe.DataArray(np.zeros((5, 7)), dims=("station", "time"), coords={"x": x, "y": y})
    np.testing.assert_array_equal(sample_coordinates(X, "station"), np.stack([x, y], 1))
    Z = xe.DataArray(np.zeros((5, 7)), dims=("station", "time"), coords={"Latitude": y, "longitude": x})
    np.testing.assert_array_equal(sample_coordinates(Z, ("station",)), np.stack([x, y], 1))
    with pytest.raises(ValueError, match="Cannot find sample coordinates."):
        sample_coordinates(xe.DataArray(np.zeros((5, 7)), dims=("station", "time")), "station")
    with pytest.raises(ValueError, match="Cannot find sample coordinates."):
        xe.single.GWPCA(n_modes=1, bandwidth=1.0).fit(xe.DataArray(np.zeros((5, 7)), dims=("station", "time")), "station")


def test_three_sample_dims_raise():
    import xeofs_amd as xe

    X = xe.DataArray(np.zeros((2, 3, 4, 5)), dims=("a", "lat", "lon", "f"))
    with pytest.raises(ValueError, match="<= 2"):
        xe.single.GWPCA(n_modes=1, bandwidth=100.0).fit(X, ("a", "lat", "lon"))


def test_not_supported():
    from xeofs_amd.single import GWPCA

    m = GWPCA(n_modes=1, bandwidth=1.0)
    for f in (m.scores, m.transform, m.inverse_transform):
        with pytest.raises(NotImplementedError):
            f(None)


def test_gw_entries_in_abi():
    from xeofs_amd import _lib

    syms = header_symbols()
    lib = _lib.load()
    for s in ("eofx_gwpca_f64", "eofx_gw_cov_f64", "eofx_batched_syev_f64"):
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib.__file__), "..", "include", "eofx.h")).read()
    for c in ("EOFX_GW_METRIC_EUCLIDEAN", "EOFX_GW_METRIC_HAVERSINE", "EOFX_GW_KERNEL_BISQUARE", "EOFX_GW_KERNEL_GAUSSIAN",
              "EOFX_GW_KERNEL_EXPONENTIAL"):
        assert c in hdr
    assert set(syms) == set(_lib.SIGNATURES)
