"""xeofs_amd.single.GWPCA -- drop-in for xeofs.single.GWPCA (xeofs/single/gwpca.py:19-230): geographically weighted PCA
[Harris, Brunsdon & Charlton 2011], one local PCA per location (sample) of the preprocessed field, its neighbours weighted
by a kernel of their distance.

The reference loops over every location with a numba prange and measures the distance to ALL locations
(xeofs/utils/optional/numba_utils.py:13-76).  Here the local covariances are accumulated on the device from spatially
tiled locations, pruning only tile pairs whose weights are all exactly 0 in float64, and a batched Jacobi eigensolver
takes their leading eigenpairs (csrc/eofx_gw.hpp, engine.gwpca).

Deliberate deviations from the reference:
  1. coordinates are identified by NAME (x / lon, y / lat lists of xeofs/utils/constants.py), so dim=("lat", "lon") and
     ("lon", "lat") give the same result; the reference feeds its stacked index columns in dims order, latitude as
     longitude for ("lat", "lon");
  2. the components carry the engine's deterministic sign rule (the reference keeps LAPACK's signs);
  3. a location with fewer positive-weight neighbours than n_modes gets 0 for the trailing eigenvalues and an orthonormal
     completion for their components (e_1 .. e_k for a zero local covariance, ratio 0 / 0 = NaN);
  4. largest_locally_weighted_components() maps the argmax to the feature labels of the VALID features;
  5. at most 256 valid features (ValueError): the covariance kernel stages a neighbour tile of 16 x (p + 1) float64 in LDS.
"""

from __future__ import annotations

import datetime

import numpy as np

from .. import __version__, engine, labelled
from ..preprocessing import Preprocessor, _as_tuple

# xeofs/utils/constants.py
VALID_LATITUDE_NAMES = ["latitude", "lats", "lat", "Latitude", "Lats", "Lat", "LATITUDE", "LATS", "LAT"]
VALID_LONGITUDE_NAMES = ["lon", "lons", "longitude", "longitudes"]
VALID_CARTESIAN_X_NAMES = ["x", "x_coord"]
VALID_CARTESIAN_Y_NAMES = ["y", "y_coord"]
VALID_KERNELS = ["bisquare", "gaussian", "exponential"]
VALID_METRICS = ["euclidean", "haversine"]
X_NAMES = VALID_CARTESIAN_X_NAMES + VALID_LONGITUDE_NAMES
Y_NAMES = VALID_CARTESIAN_Y_NAMES + VALID_LATITUDE_NAMES


def _is_x(name) -> bool:
    return isinstance(name, str) and name.lower() in X_NAMES


def _is_y(name) -> bool:
    return isinstance(name, str) and name.lower() in Y_NAMES


def _coords_along(obj, dim):
    """{name: values} of the coordinates that run along `dim` besides `dim` itself: extra coords of the stand-in DataArray,
    non-dimension coordinates or MultiIndex levels of an xarray.DataArray"""
    if labelled.is_xarray(obj):
        return {k: np.asarray(v.values) for k, v in obj.coords.items() if k != dim and tuple(v.dims) == (dim,)}
    _, dims, coords, _, _ = labelled.unpack(obj)
    n = labelled.unpack(obj)[0].shape[dims.index(dim)]
    return {k: np.asarray(v) for k, v in coords.items() if k != dim and k not in dims and np.ndim(v) == 1 and len(v) == n}


def sample_coordinates(X, sample_dims) -> np.ndarray:
    """(x, y) of every sample in the stacked sample order of the Preprocessor (sample dims in the given order,
    C order) -> [n, 2] float64.  x is the longitude for haversine.  gwpca.py:136-165 with coordinates taken by name."""
    sample_dims = _as_tuple(sample_dims)
    obj = labelled.first_array(X)
    vals, dims, coords, _, _ = labelled.unpack(obj)
    if len(sample_dims) == 1:
        d = sample_dims[0]
        along = _coords_along(obj, d)
        xs = [k for k in along if _is_x(k)]
        ys = [k for k in along if _is_y(k)]
        if not xs or not ys:
            raise ValueError("Cannot find sample coordinates.")
        return np.stack([np.asarray(along[xs[0]], dtype=np.float64), np.asarray(along[ys[0]], dtype=np.float64)], axis=1)
    if len(sample_dims) == 2:
        d0, d1 = sample_dims
        swap = (_is_y(d0) or _is_x(d1)) and not (_is_x(d0) or _is_y(d1))
        c0 = np.asarray(coords[d0], dtype=np.float64)
        c1 = np.asarray(coords[d1], dtype=np.float64)
        g0, g1 = np.meshgrid(c0, c1, indexing="ij")
        xy = np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1)
        return np.ascontiguousarray(xy[:, ::-1]) if swap else xy
    raise ValueError(f"GWPCA requires number of sample dimensions to be <= 2, but got {len(sample_dims)}.")


class GWPCA:
    """Drop-in for xeofs.single.GWPCA (xeofs/single/gwpca.py:19-230).  `fit` computes, for every location, the local PCA of
    all locations weighted by `kernel` of their `metric` distance over `bandwidth` (haversine in km, euclidean in data
    units).  Accessors: components() (mode, *dims), explained_variance(), explained_variance_ratio() and
    largest_locally_weighted_components() (mode, *sample_dims); scores / transform / inverse_transform are not supported
    (as in the reference).  The module docstring lists the deliberate deviations."""

    def __init__(self, n_modes: int, bandwidth: float, metric: str = "haversine", kernel: str = "bisquare",
                 center: bool = True, standardize: bool = False, use_coslat: bool = False, check_nans: bool = True,
                 sample_name: str = "sample", feature_name: str = "feature"):
        if kernel not in VALID_KERNELS:
            raise ValueError(f"Invalid kernel: {kernel}. Must be one of {VALID_KERNELS}.")
        if metric not in VALID_METRICS:
            raise ValueError(f"Invalid metric: {metric}. Must be one of {VALID_METRICS}.")
        if bandwidth <= 0:
            raise ValueError(f"Invalid bandwidth: {bandwidth}. Must be > 0.")
        self.n_modes = n_modes
        self.bandwidth, self.metric, self.kernel = bandwidth, metric, kernel
        self.sample_name, self.feature_name = sample_name, feature_name
        self._params = dict(n_modes=n_modes, bandwidth=bandwidth, metric=metric, kernel=kernel, center=center,
                            standardize=standardize, use_coslat=use_coslat, check_nans=check_nans, sample_name=sample_name,
                            feature_name=feature_name)
        self.ctx = None
        # the engine's own compacted feature-contiguous layout: the covariance kernel reads rows of it
        self.preprocessor = Preprocessor(center, standardize, use_coslat, check_nans, in_place=False)
        self.attrs = {"model": "GWPCA", "software": "xeofs_amd", "version": __version__,
                      "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")}
        self.attrs.update({k: (str(v) if isinstance(v, bool) or v is None else v) for k, v in self._params.items()})
        self.data = {}
        self.stats = {}

    def get_params(self):
        return dict(self._params)

    # ------------------------------------------------------------------ fit
    def fit(self, X, dim, weights=None):
        sample_dims = _as_tuple(dim)
        xy = sample_coordinates(X, sample_dims)          # before any device work: the argument errors come first
        if labelled.is_complex(X):
            raise TypeError("GWPCA does not support complex data.")
        self.ctx = self.ctx or engine.default_context()
        self.preprocessor.ctx = self.ctx
        mat = self.preprocessor.fit_transform(X, sample_dims, weights)
        self.sample_dims = self.preprocessor.sample_dims
        xy = xy[self.preprocessor.valid_sample]
        k = int(self.n_modes)
        if not 1 <= k <= mat.p or mat.p > engine.GW_PMAX:
            p = mat.p
            mat.free()
            if p > engine.GW_PMAX:
                raise ValueError(f"GWPCA supports at most {engine.GW_PMAX} valid features, the data have {p}")
            raise ValueError(f"n_modes must be in [1, {p}] (the number of valid features), got {self.n_modes}")
        try:
            V, ev, tv, self.stats = engine.gwpca(self.ctx, mat, xy, k, self.bandwidth, self.metric, self.kernel)
        finally:
            mat.free()
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = ev / tv[:, None]
        self.data = dict(components=V, explained_variance=ev, explained_variance_ratio=ratio, total_variance=tv)
        return self

    # ------------------------------------------------------------------ accessors
    def _sample_out(self, S, name, fill=np.nan):
        """(n_valid, k) per-location values -> (mode, *sample_dims in the input's dims order), fill for dropped locations"""
        pre = self.preprocessor
        f = pre.fields[0]
        vs = pre.valid_sample
        k = S.shape[1]
        full = np.full((vs.size, k), fill, dtype=S.dtype)
        full[vs] = S
        blk = full.T.reshape((k,) + f.sample_shape)
        order = [d for d in f.dims if d in f.sample_dims]
        blk = np.transpose(blk, [0] + [1 + f.sample_dims.index(d) for d in order])
        coords = {d: f.coords[d] for d in order}
        coords["mode"] = np.arange(1, k + 1)
        return labelled.pack(blk, ("mode",) + tuple(order), coords, name, dict(self.attrs), f.like)

    def components(self):
        """local components with dims (mode, *dims of the input): NaN for dropped locations and features"""
        pre = self.preprocessor
        V = self.data["components"]                       # (n_valid, p_valid, k)
        n_valid, _, k = V.shape
        vs, vf = pre.valid_sample, pre.valid_feature
        full = np.full((vs.size, vf.size, k), np.nan, np.float32)
        full[np.ix_(vs, vf)] = V
        outs, off = [], 0
        for f in pre.fields:
            blk = full[:, off:off + f.P].reshape(f.sample_shape + f.feature_shape + (k,))
            off += f.P
            src = f.sample_dims + f.feature_dims
            blk = np.moveaxis(blk, -1, 0)
            blk = np.transpose(blk, [0] + [1 + src.index(d) for d in f.dims])
            coords = {d: f.coords[d] for d in f.dims}
            coords["mode"] = np.arange(1, k + 1)
            outs.append(labelled.pack(blk, ("mode",) + tuple(f.dims), coords, "components", dict(self.attrs), f.like))
        return pre._wrap(outs)

    def explained_variance(self):
        return self._sample_out(self.data["explained_variance"], "explained_variance")

    def explained_variance_ratio(self):
        return self._sample_out(self.data["explained_variance_ratio"], "explained_variance_ratio")

    def largest_locally_weighted_components(self):
        """the label of the feature with the largest |component| per location and mode (gwpca.py:212-218); the labels of
        the valid features, a tuple of coordinates where there are several feature dimensions (the field's name first
        for several input arrays)"""
        pre = self.preprocessor
        idx = np.abs(self.data["components"]).argmax(axis=1)          # (n_valid, k), into the valid features
        if len(pre.fields) == 1 and len(pre.fields[0].feature_dims) == 1:
            # one feature dim: its coordinate values as they are (numbers, strings, datetime64 ...)
            f = pre.fields[0]
            labels = np.asarray(f.coords[f.feature_dims[0]])[pre.valid_feature]
            vals = labels[idx]
            if vals.dtype.kind in "iub":
                vals = vals.astype(np.float64)                         # NaN for the dropped locations
            elif vals.dtype.kind not in "fcmM":
                vals = vals.astype(object)
            return self._sample_out(vals, "largest_locally_weighted_components",
                                    np.array("NaT", vals.dtype) if vals.dtype.kind in "mM" else np.nan)
        labels = []
        for f in pre.fields:
            grids = np.meshgrid(*[np.asarray(f.coords[d]) for d in f.feature_dims], indexing="ij")
            flat = [g.reshape(-1) for g in grids]
            for i in range(f.P):
                lab = tuple(g[i] for g in flat)                      # numpy scalars: datetime64 stays a datetime
                labels.append(((f.name,) + lab) if len(pre.fields) > 1 else (lab[0] if len(lab) == 1 else lab))
        labels = np.array(labels + [None], dtype=object)[:-1][pre.valid_feature]
        vals = labels[idx]
        return self._sample_out(vals, "largest_locally_weighted_components")

    # ------------------------------------------------------------------ not supported (as in the reference)
    def scores(self, *args, **kwargs):
        raise NotImplementedError("GWPCA does not support scores() yet.")

    def transform(self, *args, **kwargs):
        raise NotImplementedError("GWPCA does not support transform() yet.")

    def inverse_transform(self, *args, **kwargs):
        raise NotImplementedError("GWPCA does not support inverse_transform() yet.")
