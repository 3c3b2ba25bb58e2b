"""Python handles over the C ABI (include/eofx.h): context, resident matrix, one plain function per entry point, and
the marshalling those functions share (weights, statistics buffers, layout mode, start matrix, iteration code, output
factors, the collective-error protocol).  numpy arrays are host buffers, torch CUDA tensors are device buffers; the
library detects which.  Bindings and marshalling only: nothing here iterates, and no arithmetic happens in this file
(the one solver written in Python on top of these calls is xeofs_amd/spca.py).
"""

from __future__ import annotations

import contextlib
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import ptr, raise_for


def _f32c(a):
    """float32 C-contiguous host array or a device tensor, unchanged if already so."""
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a, dtype=np.float32)
    if hasattr(a, "data_ptr"):  # torch tensor
        import torch

        if a.dtype != torch.float32 or not a.is_contiguous():
            a = a.to(torch.float32).contiguous()
        return a
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


class Context:
    """One GPU + one HIP stream (eofx_ctx)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        """stream: a hipStream_t handle; None = torch's CURRENT stream on `device` at construction (the default stream
        unless the caller is inside `torch.cuda.stream(...)`), so torch operations issued between engine calls stay ordered
        with the engine's kernels.  `use_stream` re-binds later."""
        self.lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            try:
                import torch

                if torch.cuda.is_available():
                    stream = int(torch.cuda.current_stream(int(device)).cuda_stream)
            except Exception:
                stream = None
        rc = self.lib.eofx_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(h))
        if rc != 0:
            raise _lib.EofxError(
                f"eofx_ctx_create(device={device}) failed ({rc}): no usable MI355X / HIP runtime. "
                "xeofs_amd has no CPU fallback.")
        self.handle = h
        self.device = int(device)
        self.precision = ("f16x3", "f16x3")

    def synchronize(self):
        raise_for(self.lib.eofx_ctx_synchronize(self.handle), self.handle)

    def use_stream(self, stream=None):
        """bind the context to a hipStream_t handle / a torch.cuda.Stream (None: torch's current stream on this device)"""
        if stream is None:
            stream = _torch().cuda.current_stream(self.device)
        handle = int(getattr(stream, "cuda_stream", stream) or 0)
        raise_for(self.lib.eofx_ctx_set_stream(self.handle, C.c_void_p(handle)), self.handle)

    def set_precision(self, power="f16x3", final="f16x3"):
        """Arithmetic of the matrix passes: "f16x3" (scaled split-fp16 MFMA, default), "f32" (exact-f32
        MFMA), "bf16x3", "bf16x6" (split-bf16 MFMA); see include/eofx.h."""
        raise_for(self.lib.eofx_ctx_set_precision(self.handle, _lib.PREC[power], _lib.PREC[final]), self.handle)
        self.precision = (power, final)

    def trim(self):
        """Return cached resident-matrix buffers to the device."""
        raise_for(self.lib.eofx_ctx_trim(self.handle), self.handle)

    def profile(self, enable: bool = True):
        raise_for(self.lib.eofx_ctx_profile(self.handle, int(enable)), self.handle)

    def profile_read(self):
        """-> dict(launches, ms, flops, bytes) of the atb_f32 launches since the last read."""
        n = C.c_int64()
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        raise_for(self.lib.eofx_ctx_profile_read(self.handle, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)),
                  self.handle)
        kl, km = (C.c_int64 * 3)(), (C.c_double * 3)()
        raise_for(self.lib.eofx_ctx_profile_by_kernel(self.handle, kl, km), self.handle)
        by_kernel = {name: dict(launches=int(kl[i]), ms=float(km[i])) for i, name in enumerate(("atb", "axb")) if kl[i]}
        return dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value, by_kernel=by_kernel)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.eofx_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class ResidentMatrix:
    """A preprocessed (sample x feature) matrix resident in HBM (eofx_mat)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self.handle = handle
        n, p, npad, ppad = (C.c_int64() for _ in range(4))
        ctx.lib.eofx_mat_shape(handle, C.byref(n), C.byref(p), C.byref(npad), C.byref(ppad))
        self.n, self.p, self.n_pad, self.p_pad = n.value, p.value, npad.value, ppad.value
        self._keepalive = None     # the device field a raw-mode matrix reads (must outlive it)
        # Masked in-place matrix (layout mode 3, include/eofx.h): all-NaN grid points stay in the matrix as zero columns.
        # `p` is the number of VALID features -- what every caller means by it --, `p_phys` the column count of the
        # engine's matrix; `valid_index` (int64, ascending) maps one onto the other.  The functions of this module
        # compact / scatter the feature axis of the factors, so callers never see the zero columns.
        self.p_phys = self.p
        self.valid_index = None
        mk, pv = C.c_int(), C.c_int64()
        ctx.lib.eofx_mat_masked(handle, C.byref(mk), C.byref(pv))
        self.masked = bool(mk.value)
        if self.masked:
            self.p = pv.value

    def set_valid(self, valid_feature):
        """the boolean mask of valid features of a masked matrix (from the preprocessing statistics)"""
        idx = np.flatnonzero(np.asarray(valid_feature, dtype=bool)).astype(np.int64)
        if idx.size != self.p or (idx.size and idx[-1] >= self.p_phys):
            raise ValueError("valid-feature mask does not match the masked matrix")
        self.valid_index = idx
        self._valid_dev = None

    def _vidx(self, device=None):
        """valid_index as a torch tensor on `device` (cached)"""
        torch = _torch()
        dev = device if device is not None else f"cuda:{self.ctx.device}"
        if getattr(self, "_valid_dev", None) is None or str(self._valid_dev.device) != str(torch.device(dev)):
            self._valid_dev = torch.as_tensor(self.valid_index, device=dev)
        return self._valid_dev

    def compact_rows(self, V):
        """rows of the valid features of a factor with p_phys rows (numpy array or torch tensor)"""
        if not self.masked:
            return V
        if hasattr(V, "data_ptr"):
            return V.index_select(0, self._vidx(V.device)).contiguous()
        return np.ascontiguousarray(V[self.valid_index])

    def scatter_rows(self, V):
        """a factor with p rows -> p_phys rows, zeros at the masked features"""
        if not self.masked:
            return V
        if hasattr(V, "data_ptr"):
            torch = _torch()
            out = torch.zeros((self.p_phys,) + tuple(V.shape[1:]), dtype=V.dtype, device=V.device)
            out.index_copy_(0, self._vidx(V.device), V)
            return out
        out = np.zeros((self.p_phys,) + V.shape[1:], dtype=V.dtype)
        out[self.valid_index] = V
        return out

    @property
    def shape(self):
        return (self.n, self.p)

    def download(self) -> np.ndarray:
        out = np.empty((self.n, self.p_phys), dtype=np.float32)
        raise_for(self.ctx.lib.eofx_mat_download_f32(self.ctx.handle, self.handle, ptr(out)), self.ctx.handle)
        return np.ascontiguousarray(out[:, self.valid_index]) if self.masked else out

    def sumsq(self) -> float:
        out = C.c_double()
        raise_for(self.ctx.lib.eofx_mat_sumsq_f64(self.ctx.handle, self.handle, C.byref(out)), self.ctx.handle)
        return out.value

    def gram(self, side: int = 0, out=None):
        """side 0: X X^T as an [n_pad, n_pad] float32 device tensor; side 1: X^T X [p_pad, p_pad]
        (rows/columns beyond n / p are zero).  out: a contiguous float32 device tensor of that shape to write into."""
        torch = _torch()
        if side and self.masked:
            raise NotImplementedError("feature-space Gram matrix of a masked in-place matrix")
        d = self.p_pad if side else self.n_pad
        if out is None:
            out = torch.empty((d, d), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        elif tuple(out.shape) != (d, d) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 device tensor of shape ({d}, {d})")
        raise_for(self.ctx.lib.eofx_mat_gram_f32(self.ctx.handle, self.handle, int(side), ptr(out)), self.ctx.handle)
        return out

    def sample_gram(self):
        return self.gram(0)

    def cross_gram(self, other: "ResidentMatrix", side: int = 0):
        """side 0: A_self A_other^T [n_pad, n_pad]; side 1: A_self^T A_other [p_pad, p_pad] (float32 device tensor)"""
        torch = _torch()
        d = self.p_pad if side else self.n_pad
        G = torch.empty((d, d), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        raise_for(self.ctx.lib.eofx_mat_cross_gram_f32(self.ctx.handle, self.handle, other.handle, int(side), ptr(G)),
                  self.ctx.handle)
        return G

    def layout(self):
        """-> (has the feature-contiguous layout, reads the raw field instead): see eofx_ctx_set_layout"""
        hx, hr = C.c_int(), C.c_int()
        self.ctx.lib.eofx_mat_layout(self.handle, C.byref(hx), C.byref(hr))
        return bool(hx.value & 1), bool(hr.value)

    def has_sample_layout(self):
        """False for an in-place matrix until an entry point that needs the sample-contiguous layout has built it"""
        hx = C.c_int()
        self.ctx.lib.eofx_mat_layout(self.handle, C.byref(hx), None)
        return bool(hx.value & 2)

    def ensure_sample_layout(self, only_if_room: bool = True) -> bool:
        """Build the sample-contiguous layout ahead of repeated decompositions on this matrix (their X Y passes run
        faster over it than over the raw field).  only_if_room: only when HBM holds one more copy of the field with 8 GB
        to spare.  -> whether the layout exists afterwards (never for a masked in-place matrix)."""
        built = C.c_int()
        raise_for(self.ctx.lib.eofx_mat_ensure_sample_layout(self.ctx.handle, self.handle, int(only_if_room), C.byref(built)),
                  self.ctx.handle)
        return bool(built.value)

    def release_sample_layout(self):
        """Drop the sample-contiguous layout again (a matrix that still holds the raw field and its map, or the other
        layout, rebuilds it on demand); the memory returns to the context's pool."""
        raise_for(self.ctx.lib.eofx_mat_release_sample_layout(self.ctx.handle, self.handle), self.ctx.handle)

    def release_raw(self):
        """Drop the reference to the raw field (raw / in-place mode); missing layouts are built first / on demand."""
        raise_for(self.ctx.lib.eofx_mat_release_raw(self.ctx.handle, self.handle), self.ctx.handle)
        self._keepalive = None

    def free(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.eofx_mat_destroy(self.ctx.handle, self.handle)
        self.handle = None
        self._keepalive = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _host_staging(shape):
    """float32 host array the engine will upload: page-locked when a GPU is present (the upload of the
    sketch then is a plain DMA instead of a staged pageable copy; torch caches the pinned blocks)"""
    try:
        torch = _torch()
        if torch.cuda.is_available():
            return torch.empty(shape, dtype=torch.float32, pin_memory=True).numpy()
    except Exception:
        pass
    return np.empty(shape, dtype=np.float32)


def _host_out(shape, dtype=np.float32):
    """host array the engine will fill: page-locked above a few MB, so that the download of a 1M-row factor (207 MB of
    components at config 4) is one DMA at PCIe speed instead of a staged pageable copy at a fifth of it"""
    dtype = np.dtype(dtype)
    if int(np.prod(shape, dtype=np.int64)) * dtype.itemsize >= (8 << 20):
        try:
            torch = _torch()
            tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.complex64): torch.complex64}.get(dtype)
            if tdt is not None and torch.cuda.is_available():
                return torch.empty(tuple(shape), dtype=tdt, pin_memory=True).numpy()
        except Exception:
            pass
    return np.empty(shape, dtype=dtype)


def sketch_matrix(rows: int, size: int, random_state=None) -> np.ndarray:
    """The Gaussian test matrix exactly as scikit-learn draws it for
    randomized_svd (sklearn/utils/extmath.py `_randomized_range_finder`):
    ``check_random_state(seed).normal(size=(A.shape[1], size))`` cast to float32,
    so a given `random_state` means the same thing as in the reference
    (xeofs/linalg/decomposer.py:141-146)."""
    if random_state is None or random_state is np.random:
        rs = np.random.mtrand._rand
    elif isinstance(random_state, numbers.Integral):
        seed = int(random_state)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("Seed must be between 0 and 2**32 - 1")
        # native generator: the same legacy MT19937 / polar-method stream as RandomState(seed).normal,
        # bit for bit (tests/test_abi.py), ~3x faster than numpy for the 600k draws of a 10000 x 60 sketch
        out = _host_staging((rows, size))
        raise_for(_lib.load().eofx_sketch_gaussian_f32(seed, rows, size, ptr(out)))
        return out
    elif isinstance(random_state, np.random.RandomState):
        rs = random_state
    else:
        raise ValueError(f"{random_state!r} cannot be used to seed a numpy.random.RandomState instance")
    return np.ascontiguousarray(rs.normal(size=(rows, size)).astype(np.float32))


def sketch_cache_drop() -> None:
    """Release the engine's one-entry cache of the last sketch matrix drawn from an integer seed (it only saves the redraw
    when the same (seed, rows, size) is asked for again; the matrix returned is the same either way)."""
    raise_for(_lib.load().eofx_sketch_cache_drop())


class SketchFuture:
    """Draws the sketch matrix on a worker thread so the ~10 ms of legacy-RandomState sampling
    (600k normals at n=10000, l=60) overlap the preprocess kernels of the same fit (the ctypes
    call into the engine releases the GIL).  `.result()` joins."""

    def __init__(self, rows, size, random_state=None):
        import threading

        self.rows, self.size = int(rows), int(size)
        self._out = None
        self._err = None

        def run():
            try:
                self._out = sketch_matrix(rows, size, random_state)
            except Exception as e:  # re-raised in the caller's thread
                self._err = e

        self._t = threading.Thread(target=run, daemon=True)
        self._t.start()

    def result(self):
        self._t.join()
        if self._err is not None:
            raise self._err
        return self._out


class SketchSlice:
    """The leading `rows` rows of a SketchFuture (numpy fills the draw row by row, so they ARE the smaller draw); joined on
    `.result()`, which engine.crosscov_rsvd calls as late as the engine allows."""

    def __init__(self, future, rows):
        self.future, self.rows = future, int(rows)

    def result(self):
        return np.ascontiguousarray(self.future.result()[:self.rows])


def from_dense(ctx: Context, X) -> ResidentMatrix:
    X = _f32c(X)
    n, p = X.shape
    h = C.c_void_p()
    raise_for(ctx.lib.eofx_mat_from_dense_f32(ctx.handle, ptr(X), n, p, p, C.byref(h)), ctx.handle)
    return ResidentMatrix(ctx, h)


# --------------------------------------------------------------------------- #
# marshalling shared by the entry points below                                  #
# --------------------------------------------------------------------------- #
def _layout_mode(keep_raw, in_place, allow_masked):
    return (3 if allow_masked else 2) if in_place else int(bool(keep_raw))


@contextlib.contextmanager
def _layout(ctx: Context, mode: int, sample_raw: bool = False):
    """the layout mode (eofx_ctx_set_layout) and the sample-raw flag (eofx_ctx_set_sample_raw) of the call inside the block;
    both are context state of the engine and go back to 0 however the block ends"""
    ctx.lib.eofx_ctx_set_layout(ctx.handle, int(mode))
    ctx.lib.eofx_ctx_set_sample_raw(ctx.handle, int(bool(sample_raw)))
    try:
        yield
    finally:
        ctx.lib.eofx_ctx_set_layout(ctx.handle, 0)
        ctx.lib.eofx_ctx_set_sample_raw(ctx.handle, 0)


@contextlib.contextmanager
def _collective(ctx: Context):
    """a call that issues collectives through the communicator attached to the context: an exception raised inside a
    callback communicator cannot cross the C frames, so the trampoline (`comm_set_callback`) stores it in `ctx._comm_err` and
    returns an error status.  The slot is cleared on entry and a stored exception is re-raised on exit -- BEFORE the caller
    looks at the status code, which only says that some collective failed."""
    ctx._comm_err = None
    yield
    if getattr(ctx, "_comm_err", None) is not None:
        raise ctx._comm_err


def _weights(feature_weights, P: int, what: str = "stacked feature"):
    """feature weights as a float64 C-contiguous host array with one entry per `what`, or None"""
    if feature_weights is None:
        return None
    w = np.ascontiguousarray(feature_weights, dtype=np.float64)
    if w.shape != (P,):
        raise ValueError(f"feature_weights must have one entry per {what}")
    return w


class _FitStats:
    """The statistics a preprocessing entry point returns: the buffers the engine fills and the scalars it sets by
    reference.  `args`: the seven pointers in the order every such entry takes them."""

    def __init__(self, n: int, P: int, want_stats: bool):
        self.mean = np.empty(P, np.float64) if want_stats else None
        self.std = np.empty(P, np.float64) if want_stats else None
        self.vf = np.empty(P, np.uint8)
        self.vs = np.empty(n, np.uint8)
        self.n, self.p, self.tv = C.c_int64(), C.c_int64(), C.c_double()
        self.args = (ptr(self.mean), ptr(self.std), ptr(self.vf), ptr(self.vs), C.byref(self.n), C.byref(self.p),
                     C.byref(self.tv))

    def as_dict(self, **extra) -> dict:
        """the `stats` dict; `extra` adds keys (`fused`) or replaces what the entry does not report itself"""
        stats = dict(mean=self.mean, std=self.std, valid_feature=self.vf.astype(bool), valid_sample=self.vs.astype(bool),
                     n=self.n.value, p=self.p.value, total_variance=self.tv.value)
        stats.update(extra)
        return stats


def _adopt(ctx: Context, handle, X, keep: bool, valid_feature) -> ResidentMatrix:
    """the matrix an entry point built from the field X.  keep: the matrix reads X where it lies -- a device field is then
    referenced so that it outlives the matrix (a host field was staged and is owned by the engine).  A masked in-place
    matrix learns which of its physical columns are the valid features."""
    mat = ResidentMatrix(ctx, handle)
    if keep and hasattr(X, "data_ptr"):
        mat._keepalive = X
    if mat.masked:
        mat.set_valid(valid_feature)
    return mat


def _sketch(rows: int, width: int, omega, random_state, *, identity_when_full: bool, exact_rows, resolve_first: bool = False):
    """The start matrix [rows, width] of a randomized decomposition as a float32 C-contiguous host array -- the one place
    that knows how it is resolved.  omega: None (drawn from random_state: `sketch_matrix`), an array, or anything with
    `.result()` (SketchFuture, SketchSlice), which is joined here.
    identity_when_full: a sketch at least as wide as the matrix is small (width >= rows) spans everything, so the identity
    [rows, width] replaces an (occasionally ill-conditioned) square Gaussian; `omega` is then neither joined, drawn nor
    checked -- unless resolve_first (the panel-level drivers of xeofs_amd.sharded resolve before they look at the width: a
    draw from a shared RandomState advances it all the same).
    exact_rows: True -- the shape must be (rows, width); False -- further rows may follow (the engine is told the row count
    and reads the leading `rows`); None -- not checked, the caller slices what it needs."""
    full = identity_when_full and width >= rows
    if not full or resolve_first:
        if hasattr(omega, "result"):
            omega = omega.result()
        if omega is None:
            omega = sketch_matrix(rows, width, random_state)
        omega = np.ascontiguousarray(omega, dtype=np.float32)
        if exact_rows is None:
            fits = True
        elif exact_rows:
            fits = omega.shape == (rows, width)
        else:
            fits = omega.ndim == 2 and omega.shape[1] == width and omega.shape[0] >= rows
        if not fits:
            raise ValueError(f"omega must have shape {(rows, width)}")
    return np.eye(rows, width, dtype=np.float32) if full else omega


def _n_iter_code(n_iter, complex_rule: bool = False) -> int:
    """n_iter as the engine takes it: a count, or -1 for "auto" (scikit-learn's count).  complex_rule (the complex
    decompositions): None means "auto" as well, and "converge" is -2 -- until the Ritz values stand still (at most 20)."""
    if n_iter == "auto" or (complex_rule and n_iter is None):
        return -1
    if complex_rule and n_iter == "converge":
        return -2
    return int(n_iter)


def _factors_out(ctx: Context, n: int, rows_v: int, k: int, dtype=np.float32, device_out: bool = False):
    """-> (U [n, k], s [k] float32 host, V [rows_v, k]) for the engine to fill: host arrays, or torch tensors on the context's
    device with device_out (nothing crosses PCIe); dtype float32 or complex64"""
    if device_out:
        torch = _torch()
        tdt = torch.complex64 if np.dtype(dtype) == np.complex64 else torch.float32
        U = torch.empty((n, k), dtype=tdt, device=f"cuda:{ctx.device}")
        V = torch.empty((rows_v, k), dtype=tdt, device=f"cuda:{ctx.device}")
    else:
        U = _host_out((n, k), dtype)
        V = _host_out((rows_v, k), dtype)
    return U, np.empty(k, np.float32), V


class _CrossOut:
    """The outputs of a cross-covariance driver (x, y: the two resident matrices, k modes).  `args`: the seven pointers in
    the order both entries take them; `tsc`: the total squared covariance, NaN unless the engine is handed it."""

    def __init__(self, x: ResidentMatrix, y: ResidentMatrix, k: int):
        self.x, self.y = x, y
        # (at least one row: an empty slice of a sharded field still hands the engine a buffer)
        self.Q1 = np.empty((max(x.p_phys, 1), k), np.float32)
        self.Q2 = np.empty((max(y.p_phys, 1), k), np.float32)
        self.s = np.empty(k, np.float32)
        self.scores1 = np.empty((x.n, k), np.float32)
        self.scores2 = np.empty((x.n, k), np.float32)
        self.norm1 = np.empty(k, np.float32)
        self.norm2 = np.empty(k, np.float32)
        self.tsc = C.c_double(float("nan"))
        self.args = tuple(ptr(a) for a in (self.Q1, self.s, self.Q2, self.scores1, self.scores2, self.norm1, self.norm2))

    def as_dict(self) -> dict:
        """the result dict; Q1 / Q2 hold the rows of the valid features of their matrix"""
        rows = lambda mat, Q: mat.compact_rows(Q if Q.shape[0] == mat.p_phys else Q[:mat.p_phys])
        return dict(Q1=rows(self.x, self.Q1), Q2=rows(self.y, self.Q2), s=self.s, scores1=self.scores1, scores2=self.scores2,
                    norm1=self.norm1, norm2=self.norm2, total_squared_covariance=self.tsc.value)


# --------------------------------------------------------------------------- #
# preprocessing and decomposition entry points                                  #
# --------------------------------------------------------------------------- #

def preprocess(ctx: Context, X, center=True, standardize=False, feature_weights=None,
               check_nans=True, want_stats=True, build=True, keep_raw=False, in_place=False, allow_masked=False,
               for_hilbert=False):
    """Scaler + Sanitizer + total variance on the stacked raw (n, P) field.
    Returns (ResidentMatrix | None, stats dict).  keep_raw: raw mode (include/eofx.h, eofx_ctx_set_layout) -- the
    feature-contiguous layout is not written, the products read the raw field through the Scaler map; in_place:
    NO layout is written, both products stream the field where it lies (the sample-contiguous layout is built on
    demand by the entry points that need it).  Either way a device field must stay unmodified until
    `release_raw()` / `free()` (the matrix holds a reference to it); a host field is staged and owned.
    allow_masked (with in_place): a field whose NaN pattern is a mask of all-NaN grid points stays in place as well -- the
    masked features become zero columns of the engine's matrix (layout mode 3, include/eofx.h) and this module
    compacts / scatters the feature axis of every factor, so `mat.p` and the factors have the valid features only.
    for_hilbert (with in_place): `hilbert(ctx, mat, ...)` is the next call on this matrix -- the statistics pass also writes the
    raw field in the sample-contiguous layout (eofx_ctx_set_sample_raw) and the Hilbert stage saves its transposing copy."""
    X = _f32c(X)
    n, P = X.shape
    w = _weights(feature_weights, P)
    st = _FitStats(n, P, want_stats)
    h = C.c_void_p()
    with _layout(ctx, _layout_mode(keep_raw, in_place, allow_masked), sample_raw=for_hilbert and in_place and build):
        rc = ctx.lib.eofx_preprocess_f32(ctx.handle, ptr(X), n, P, int(center), int(standardize), ptr(w),
                                         int(check_nans), C.byref(h) if build else None, *st.args)
    raise_for(rc, ctx.handle)
    mat = _adopt(ctx, h, X, keep_raw or in_place, st.vf) if build else None
    return mat, st.as_dict()


def fit(ctx: Context, X, k: int, center=True, standardize=False, feature_weights=None, check_nans=True,
        n_oversamples: int = 10, n_iter: int | str = "auto", random_state=None, flip: bool = True, omega=None,
        want_stats=True, device_out: bool = False, in_place: bool = True, allow_masked: bool = False):
    """Scaler + Sanitizer + randomized SVD in one engine call (eofx_fit_f32): with the in-place layout the column
    statistics ride on the first pass of the decomposition, so the field is read 2 n_iter + 2 times, not 2 n_iter + 3.
    Same results as `preprocess(..., in_place=True)` followed by `rsvd(...)` (which is what the engine falls back to by
    itself for NaN fields, other precisions, wide sketches, n >= P).
    -> (ResidentMatrix, stats dict (as `preprocess`, plus `fused`), U[n', k], s[k], V[p', k])"""
    X = _f32c(X)
    n, P = X.shape
    k = int(k)
    w = _weights(feature_weights, P)
    omega = _sketch(min(n, P), k + n_oversamples, omega, random_state, identity_when_full=False, exact_rows=False)
    st = _FitStats(n, P, want_stats)
    fused = C.c_int()
    h = C.c_void_p()
    U, s, V = _factors_out(ctx, n, P, k, np.float32, device_out)
    with _layout(ctx, _layout_mode(False, in_place, allow_masked)):
        rc = ctx.lib.eofx_fit_f32(ctx.handle, ptr(X), n, P, int(center), int(standardize), ptr(w), int(check_nans), k,
                                  int(n_oversamples), _n_iter_code(n_iter), ptr(omega), omega.shape[0], int(flip),
                                  C.byref(h), *st.args, ptr(U), ptr(s), ptr(V), C.byref(fused))
    raise_for(rc, ctx.handle)
    mat = _adopt(ctx, h, X, True, st.vf)
    if mat.n != n or mat.p_phys != P:     # the factors were written densely with the compacted shape
        U = U.reshape(-1)[: mat.n * k].reshape(mat.n, k)
        V = V.reshape(-1)[: mat.p_phys * k].reshape(mat.p_phys, k)
    return mat, st.as_dict(fused=bool(fused.value)), U, s, mat.compact_rows(V)


# ---- communicator of the native feature-sharded fit (include/eofx.h: eofx_fit_sharded_f32) -------------------------------
def comm_unique_id() -> bytes:
    """128 bytes from ncclGetUniqueId (rank 0 draws them and hands them to every rank)"""
    buf = C.create_string_buffer(128)
    raise_for(_lib.load().eofx_comm_unique_id(buf))
    return buf.raw


def comm_init_rccl(ctx: Context, unique_id: bytes, world: int, rank: int):
    """attach an RCCL communicator to the context: its collectives are enqueued on the context's own stream"""
    raise_for(ctx.lib.eofx_ctx_comm_init_rccl(ctx.handle, C.c_char_p(bytes(unique_id)), int(world), int(rank)), ctx.handle)
    ctx._comm_cb = None
    ctx._comm_attached = (int(world), int(rank))


def comm_set_callback(ctx: Context, fn, world: int, rank: int):
    """attach a host callback as the collective: fn(ptr, count, dtype, op, stream) -> 0, all-reducing `count` elements of the
    device buffer in place (dtype 0 f32 / 1 f64 / 2 i32, op 0 sum / 1 max / 2 min), in stream order"""
    def tramp(_user, buf, count, dtype, op, stream):
        try:
            return int(fn(buf, int(count), int(dtype), int(op), stream) or 0)
        except BaseException as e:        # must not propagate through the C frames
            ctx._comm_err = e
            return 1

    cb = _lib.ALLREDUCE_FN(tramp)
    raise_for(ctx.lib.eofx_ctx_comm_set_callback(ctx.handle, cb, None, int(world), int(rank)), ctx.handle)
    ctx._comm_cb = cb      # keep the trampoline alive
    ctx._comm_attached = (int(world), int(rank))


def comm_clear(ctx: Context):
    raise_for(ctx.lib.eofx_ctx_comm_clear(ctx.handle), ctx.handle)
    ctx._comm_cb = None
    ctx._comm_attached = None


def comm_attached(ctx: Context):
    """(world, rank) of the communicator attached to the context, or None"""
    return getattr(ctx, "_comm_attached", None)


def comm_selftest(ctx: Context) -> bool:
    """One round of every collective the sharded fit uses on known values (collective: every rank calls it)."""
    ok = C.c_int()
    raise_for(ctx.lib.eofx_ctx_comm_selftest(ctx.handle, C.byref(ok)), ctx.handle)
    return bool(ok.value)


def comm_probe(ctx: Context, cases, reps: int = 20):
    """eofx_ctx_comm_probe (collective): cases = [(count, "f32" | "f64" | "i32"), ...] -> (ranks the communicator reduces over,
    [mean microseconds of an all-reduce(sum) per case])"""
    codes = {"f32": 0, "f64": 1, "i32": 2}
    counts = np.ascontiguousarray([int(c) for c, _ in cases], dtype=np.int64)
    dtypes = np.ascontiguousarray([codes[d] for _, d in cases], dtype=np.int32)
    seen = np.zeros(1, np.float64)
    us = np.zeros(len(cases), np.float64)
    raise_for(ctx.lib.eofx_ctx_comm_probe(ctx.handle, len(cases), ptr(counts), ptr(dtypes), int(reps), ptr(seen), ptr(us)), ctx.handle)
    return float(seen[0]), [float(x) for x in us]


def comm_stats(ctx: Context):
    """-> dict(calls, bytes, ms) of the collectives of the native sharded fit since the last call (ms: while profiling)"""
    calls, nbytes, ms = C.c_int64(), C.c_int64(), C.c_double()
    raise_for(ctx.lib.eofx_ctx_comm_stats(ctx.handle, C.byref(calls), C.byref(nbytes), C.byref(ms)), ctx.handle)
    return dict(calls=calls.value, bytes=nbytes.value, ms=ms.value)


def fit_sharded(ctx: Context, X, k: int, p_total: int, center=True, standardize=False, feature_weights=None,
                n_oversamples: int = 10, n_iter: int | str = "auto", random_state=None, flip: bool = True, omega=None,
                want_stats=True, device_out: bool = False, allow_masked: bool = False):
    """`fit` on this rank's slice X [n, p_local] of a field with `p_total` features, the ranks joined by the communicator
    attached to the context (eofx_fit_sharded_f32: every collective is issued by the engine on its own stream).
    -> (ResidentMatrix, stats, U[n, k] replicated, s[k], V[p_local, k]) or None when some rank cannot take the fused path
    (the ranks agree on that; nothing has been built -- use the panel-level driver, xeofs_amd.sharded)."""
    X = _f32c(X)
    n, P = X.shape
    k = int(k)
    w = _weights(feature_weights, P, what="stacked feature of the slice")
    omega = _sketch(n, k + n_oversamples, omega, random_state, identity_when_full=False, exact_rows=False)
    st = _FitStats(n, P, want_stats)
    h = C.c_void_p()
    U, s, V = _factors_out(ctx, n, P, k, np.float32, device_out)
    # (on the way out the layout is reset first, then an exception a callback communicator stored is re-raised)
    with _collective(ctx), _layout(ctx, _layout_mode(False, True, allow_masked)):
        rc = ctx.lib.eofx_fit_sharded_f32(ctx.handle, ptr(X), n, P, int(p_total), int(center), int(standardize), ptr(w), k,
                                          int(n_oversamples), _n_iter_code(n_iter), ptr(omega), omega.shape[0], int(flip),
                                          C.byref(h), ptr(st.mean), ptr(st.std), ptr(st.vf), C.byref(st.tv), ptr(U), ptr(s),
                                          ptr(V))
    if rc == 1:       # the ranks' vote for the panel-level driver; only now is any other status an error
        return None
    raise_for(rc, ctx.handle)
    mat = _adopt(ctx, h, X, True, st.vf)
    # the sharded entry drops no sample and reports no counts: every sample is valid, p is the slice's valid features
    return mat, st.as_dict(valid_sample=np.ones(n, bool), n=n, p=mat.p, fused=True), U, s, mat.compact_rows(V)


def fit_first(ctx: Context, X, Zn, l: int, center=True, standardize=False, feature_weights=None, check_nans=True,
              want_stats=True):
    """The statistics-carrying first pass on its own (eofx_fit_first_f32): Yp = X'^T Zn for the device panel Zn
    [n_pad, L] (first l < L columns in use) together with the preprocessing of X (in-place layout).
    -> (ResidentMatrix, stats dict as `preprocess` plus `fused`, Yp [p_pad, L] device tensor or None when samples were
    dropped and the caller has to redo the product with the surviving rows of Z)"""
    torch = _torch()
    X = _f32c(X)
    n, P = X.shape
    w = _weights(feature_weights, P)
    L = Zn.shape[1]
    Yp = torch.empty(((P + 511) // 512 * 512, L), dtype=torch.float32, device=Zn.device)
    st = _FitStats(n, P, want_stats)
    fused = C.c_int()
    h = C.c_void_p()
    with _layout(ctx, 2):
        rc = ctx.lib.eofx_fit_first_f32(ctx.handle, ptr(X), n, P, int(center), int(standardize), ptr(w), int(check_nans),
                                        ptr(Zn), L, int(l), ptr(Yp), C.byref(h), *st.args, C.byref(fused))
    raise_for(rc, ctx.handle)
    mat = _adopt(ctx, h, X, True, st.vf)
    if st.n.value != n:
        Yp = None
    elif mat.p_pad != Yp.shape[0]:
        Yp = Yp[: mat.p_pad].contiguous()
    return mat, st.as_dict(fused=bool(fused.value)), Yp


def fit_info(ctx: Context):
    """-> dict(fused, preprocess_ms, reason) of the last `fit` on this context (include/eofx.h, eofx_ctx_fit_info)"""
    info = (C.c_double * 3)()
    raise_for(ctx.lib.eofx_ctx_fit_info(ctx.handle, info), ctx.handle)
    return dict(fused=bool(info[0]), preprocess_ms=float(info[1]), reason=int(info[2]))


def last_iterations(ctx: Context) -> int:
    """power iterations of the last `rsvd_c64` on this context (its n_iter="auto" iterates until the Ritz values stand still)"""
    out = C.c_int()
    raise_for(ctx.lib.eofx_ctx_last_iterations(ctx.handle, C.byref(out)), ctx.handle)
    return out.value


def apply(ctx: Context, X, mean, std, feature_weights, valid_feature, check_nans=True, in_place=False, allow_masked=False):
    """Preprocessor.transform on new data with fitted state.  in_place: as in `preprocess` -- nothing is written, the
    projection that follows streams the (staged) field through the fitted map."""
    X = _f32c(X)
    n, P = X.shape
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    mean, std, w = f64(mean), f64(std), f64(feature_weights)
    vf = np.ascontiguousarray(valid_feature, dtype=np.uint8)
    vs = np.empty(n, np.uint8)
    n_out = C.c_int64()
    h = C.c_void_p()
    with _layout(ctx, _layout_mode(False, in_place, allow_masked)):
        rc = ctx.lib.eofx_apply_f32(ctx.handle, ptr(X), n, P, ptr(mean), ptr(std), ptr(w), ptr(vf),
                                    int(check_nans), C.byref(h), ptr(vs), C.byref(n_out))
    raise_for(rc, ctx.handle)
    return _adopt(ctx, h, X, in_place, vf), vs.astype(bool)


def rsvd(ctx: Context, mat: ResidentMatrix, k: int, n_oversamples: int = 10, n_iter: int | str = "auto",
         random_state=None, flip: bool = True, omega=None, device_out: bool = False):
    """randomized SVD of the resident matrix -> (U[n,k], s[k], V[p,k]) float32 host arrays
    (or torch device tensors for U and V with `device_out=True`: nothing crosses PCIe)."""
    k = int(k)
    # (a full-width sketch becomes the identity inside the engine, eofx_rsvd_f32: the draw is still made and checked here)
    omega = _sketch(min(mat.n, mat.p), k + n_oversamples, omega, random_state, identity_when_full=False, exact_rows=True)
    if mat.masked and mat.p < mat.n:
        raise NotImplementedError("masked in-place matrix with fewer valid features than samples")   # the engine never builds one
    U, s, V = _factors_out(ctx, mat.n, mat.p_phys, k, np.float32, device_out)
    rc = ctx.lib.eofx_rsvd_f32(ctx.handle, mat.handle, k, int(n_oversamples), _n_iter_code(n_iter), ptr(omega), int(flip),
                               ptr(U), ptr(s), ptr(V))
    raise_for(rc, ctx.handle)
    return U, s, mat.compact_rows(V)


def project(ctx: Context, mat: ResidentMatrix, V) -> np.ndarray:
    V = _f32c(V)
    if V.ndim != 2 or V.shape[0] != mat.p:
        raise ValueError(f"components have {V.shape[0] if V.ndim == 2 else V.shape} features, the matrix has {mat.p} "
                         "(a different NaN pattern in the new data?)")
    k = V.shape[1]
    out = np.empty((mat.n, k), np.float32)
    V = mat.scatter_rows(V)
    raise_for(ctx.lib.eofx_project_f32(ctx.handle, mat.handle, ptr(V), k, ptr(out)), ctx.handle)
    return out


def reconstruct(ctx: Context, S, V) -> np.ndarray:
    S, V = _f32c(S), _f32c(V)
    if S.ndim != 2 or V.ndim != 2 or S.shape[1] != V.shape[1]:
        raise ValueError(f"scores {S.shape} and components {V.shape} do not have the same number of modes")
    n, k = S.shape
    p = V.shape[0]
    out = np.empty((n, p), np.float32)
    raise_for(ctx.lib.eofx_reconstruct_f32(ctx.handle, ptr(S), ptr(V), n, p, k, ptr(out)), ctx.handle)
    return out


def crosscov_rsvd(ctx: Context, x: ResidentMatrix, y: ResidentMatrix, k: int, n_oversamples: int = 10,
                  n_iter: int | str = "auto", random_state=None, flip: bool = True, omega=None,
                  want_tsc: bool = True):
    """Matrix-free rSVD of C = X^T Y/(n-1) -> dict (cpcca.py:168-225 quantities)."""
    k = int(k)
    small = min(x.p, y.p)
    if (x.masked or y.masked) and k > small:
        raise ValueError(f"n_modes must be less than or equal to the rank of the dataset (rank = {small}).")
    # the engine orients C by the VALID feature counts, as the reference does (sklearn transposes when rows < cols; round 6 --
    # before, it used the physical widths and pairs whose two orders disagree had to be compacted)
    small_mat = x if x.p < y.p else y
    if small_mat.masked and k + n_oversamples >= small:
        raise NotImplementedError("a sketch as wide as the rank on a masked in-place matrix (compact the field)")
    if x.n != y.n:
        raise ValueError(f"Both data matrices must have the same number of samples but found {x.n} in the first and "
                         f"{y.n} in the second.")

    def sketch():       # (called by the engine: a SketchFuture is joined as late as possible)
        om = _sketch(small, k + n_oversamples, omega, random_state, identity_when_full=False, exact_rows=True)
        # masked in-place matrices keep their all-NaN grid points as zero columns: the sketch gets zero rows there, the
        # singular vectors come back with zero rows there (compacted in the result)
        return np.ascontiguousarray(small_mat.scatter_rows(om))

    out = _CrossOut(x, y, k)
    # the engine asks for the sketch when it first needs it (eofx_crosscov_rsvd_lazy_f32): with the total squared
    # covariance wanted, the Gram matrices are queued before that and a SketchFuture finishes beside them
    held = {}

    def provide(_user):
        try:
            held["om"] = sketch()
            return held["om"].ctypes.data
        except BaseException as e:      # re-raised below, in the caller's frame
            held["err"] = e
            return None

    cb = _lib.SKETCH_FN(provide)
    rc = ctx.lib.eofx_crosscov_rsvd_lazy_f32(ctx.handle, x.handle, y.handle, k, int(n_oversamples), _n_iter_code(n_iter), cb,
                                             None, int(flip), *out.args, C.byref(out.tsc) if want_tsc else None)
    if "err" in held:
        raise held["err"]
    raise_for(rc, ctx.handle)
    return out.as_dict()


def comm_allreduce_host(ctx: Context, values, op: str = "sum") -> np.ndarray:
    """all-reduce of a small host vector of doubles over the communicator attached to the context
    (eofx_ctx_comm_allreduce_f64): the global facts a sharded model needs between engine calls"""
    buf = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
    with _collective(ctx):
        rc = ctx.lib.eofx_ctx_comm_allreduce_f64(ctx.handle, ptr(buf), buf.size, {"sum": 0, "max": 1, "min": 2}[op])
    raise_for(rc, ctx.handle)
    return buf


def crosscov_rsvd_sharded(ctx: Context, x: ResidentMatrix, y: ResidentMatrix, k: int, p1_total: int, p1_offset: int,
                          p2_total: int, p2_offset: int, n_oversamples: int = 10, n_iter: int | str = "auto",
                          random_state=None, flip: bool = True, omega=None, want_tsc: bool = True):
    """`crosscov_rsvd` with both fields sharded along their feature axes (eofx_crosscov_rsvd_sharded_f32; the communicator is
    the one attached to the context).  x / y: this rank's slices; p*_total / p*_offset: feature counts over all ranks and this
    slice's position on the global VALID-feature axis.  omega: the GLOBAL sketch [min(p1_total, p2_total), k + n_oversamples]
    (one draw, identical on every rank; drawn here from random_state when None).  Q1 / Q2 come back as this rank's rows."""
    k = int(k)
    if x.n != y.n:
        raise ValueError(f"Both data matrices must have the same number of samples but found {x.n} in the first and "
                         f"{y.n} in the second.")
    small = min(int(p1_total), int(p2_total))
    if k > small:
        raise ValueError(f"n_modes must be less than or equal to the rank of the dataset (rank = {small}).")
    l_req = k + int(n_oversamples)
    if l_req > small:
        raise ValueError("sketch wider than rank not supported on the cross path")
    on_x = int(p1_total) < int(p2_total)            # the sketch lives on the narrower field's feature axis
    sm, off = (x, int(p1_offset)) if on_x else (y, int(p2_offset))
    # (this entry takes the rows of the slice, so the identity of a full-width sketch is written here: see eofx_rsvd_f32)
    om = _sketch(small, l_req, omega, random_state, identity_when_full=True, exact_rows=True)
    rows = np.ascontiguousarray(sm.scatter_rows(np.ascontiguousarray(om[off:off + sm.p])), dtype=np.float32)
    if rows.shape[0] == 0:
        rows = np.zeros((1, l_req), np.float32)
    out = _CrossOut(x, y, k)
    with _collective(ctx):
        rc = ctx.lib.eofx_crosscov_rsvd_sharded_f32(ctx.handle, x.handle, y.handle, int(p1_total), int(p1_offset),
                                                    int(p2_total), int(p2_offset), k, int(n_oversamples), _n_iter_code(n_iter),
                                                    ptr(rows), int(flip), *out.args, C.byref(out.tsc) if want_tsc else None)
    raise_for(rc, ctx.handle)
    return out.as_dict()


def host_eigh(A: np.ndarray):
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    w = np.empty(n)
    V = np.empty((n, n))
    raise_for(_lib.load().eofx_host_eigh_f64(ptr(A), n, ptr(w), ptr(V)))
    return w, V


# --------------------------------------------------------------------------- #
# panel-level steps on torch device tensors (used by the feature-sharded path)  #
# --------------------------------------------------------------------------- #
def _torch():
    import torch

    return torch


def panel_width(l: int) -> int:
    return (int(l) + 31) // 32 * 32


def panel_import(ctx: Context, src, rows_pad: int, L: int):
    torch = _torch()
    src = _f32c(src)
    rows, l = src.shape
    P = torch.empty((rows_pad, L), dtype=torch.float32, device=f"cuda:{ctx.device}")
    raise_for(ctx.lib.eofx_panel_import_f32(ctx.handle, ptr(src), rows, l, ptr(P), rows_pad, L), ctx.handle)
    return P


def panel_export(ctx: Context, P, rows: int, k: int, sign=None, device_out: bool = False):
    if device_out:
        torch = _torch()
        out = torch.empty((rows, k), dtype=torch.float32, device=P.device)
    else:
        out = np.empty((rows, k), np.float32)
    sg = None if sign is None else np.ascontiguousarray(sign, dtype=np.float64)
    raise_for(ctx.lib.eofx_panel_export_f32(ctx.handle, ptr(P), rows, P.shape[1], k, ptr(sg), ptr(out)), ctx.handle)
    return out


def panel_tmul(ctx: Context, mat: ResidentMatrix, Zn, out=None, prec="f32"):
    """Yp[p_pad, L] = X^T Zn[n_pad, L]"""
    torch = _torch()
    L = Zn.shape[1]
    if out is None:
        out = torch.empty((mat.p_pad, L), dtype=torch.float32, device=Zn.device)
    raise_for(ctx.lib.eofx_panel_tmul_f32(ctx.handle, mat.handle, ptr(Zn), ptr(out), L, _lib.PREC[prec]), ctx.handle)
    return out


def panel_mul(ctx: Context, mat: ResidentMatrix, Yp, out=None, prec="f32"):
    """Wn[n_pad, L] = X Yp[p_pad, L]"""
    torch = _torch()
    L = Yp.shape[1]
    if out is None:
        out = torch.empty((mat.n_pad, L), dtype=torch.float32, device=Yp.device)
    raise_for(ctx.lib.eofx_panel_mul_f32(ctx.handle, mat.handle, ptr(Yp), ptr(out), L, _lib.PREC[prec]), ctx.handle)
    return out


def plane_stats(ctx: Context):
    """-> dict(produced_tmul, produced_cholqr, consumed, checked, min_slack, max_slack): tall panels the rSVD drivers wrote as the
    fp16 planes of the in-place X Y pass (by the X^T Z kernel / by the Cholesky-QR), passes that took them as written, and -- with EOFX_AXB_CHECK_BOUND=1 -- passes whose panel was measured
    against its bound, with the extremes of bound / maximum (include/eofx.h, eofx_ctx_plane_stats).  Restarts the counters."""
    cnt, sl = (C.c_int64 * 4)(), (C.c_double * 2)()
    raise_for(ctx.lib.eofx_ctx_plane_stats(ctx.handle, cnt, sl), ctx.handle)
    return dict(produced_tmul=int(cnt[0]), produced_cholqr=int(cnt[1]), consumed=int(cnt[2]), checked=int(cnt[3]),
                min_slack=float(sl[0]), max_slack=float(sl[1]))


def axb_plane_bytes(mat: ResidentMatrix, L: int) -> int:
    """bytes of the fp16 planes of a [p_pad x L] panel of `mat` (eofx_plans.hpp, axb_planes_bytes)"""
    return ((L + 63) // 64) * ((mat.p + 63) // 64) * 16384


def axb_planes_probe(ctx: Context, mat: ResidentMatrix, Zn, producer: int, bound: float = 0.0):
    """The plane producers of the in-place X Y pass, laid open (include/eofx.h, eofx_axb_planes_probe_f32) ->
    dict(planes_prod, planes_split (uint16 arrays), w_prod, w_split, w_reg, w_max, y (device tensors), bound)."""
    torch = _torch()
    L = Zn.shape[1]
    nb = axb_plane_bytes(mat, L)
    pp, ps = np.empty(nb // 2, np.uint16), np.empty(nb // 2, np.uint16)
    w = [torch.empty((mat.n_pad, L), dtype=torch.float32, device=Zn.device) for _ in range(4)]
    y = torch.empty((mat.p_pad, L), dtype=torch.float32, device=Zn.device)
    b = C.c_float()
    raise_for(ctx.lib.eofx_axb_planes_probe_f32(ctx.handle, mat.handle, ptr(Zn), L, int(producer), float(bound), ptr(pp), ptr(ps), nb,
                                                ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(y), C.byref(b)), ctx.handle)
    return dict(planes_prod=pp, planes_split=ps, w_prod=w[0], w_split=w[1], w_reg=w[2], w_max=w[3], y=y, bound=float(b.value))


def panel_gram(ctx: Context, P, out=None):
    torch = _torch()
    L = P.shape[1]
    if out is None:
        out = torch.empty((L, L), dtype=torch.float64, device=P.device)
    raise_for(ctx.lib.eofx_panel_gram_f64(ctx.handle, ptr(P), P.shape[0], L, ptr(out)), ctx.handle)
    return out


def panel_cholqr(ctx: Context, P, l: int, G, out=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(P)
    raise_for(ctx.lib.eofx_panel_cholqr_f32(ctx.handle, ptr(P), P.shape[0], P.shape[1], int(l), ptr(G), ptr(out)),
              ctx.handle)
    return out


def panel_rinv(ctx: Context, G, l: int):
    """R^-1 (L x L float64 device tensor) of the Cholesky factor of the leading l x l block of G"""
    torch = _torch()
    out = torch.empty_like(G)
    raise_for(ctx.lib.eofx_panel_rinv_f64(ctx.handle, ptr(G), G.shape[0], int(l), ptr(out)), ctx.handle)
    return out


def panel_matmul(ctx: Context, P, M, out=None):
    torch = _torch()
    Lo = M.shape[1]
    if out is None:
        out = torch.empty((P.shape[0], Lo), dtype=torch.float32, device=P.device)
    raise_for(ctx.lib.eofx_panel_matmul_f32(ctx.handle, ptr(P), P.shape[0], P.shape[1], ptr(M), Lo, ptr(out)),
              ctx.handle)
    return out


def panel_colminmax(ctx: Context, P, rows: int):
    torch = _torch()
    L = P.shape[1]
    mx = torch.empty(L, dtype=torch.float32, device=P.device)
    mn = torch.empty(L, dtype=torch.float32, device=P.device)
    raise_for(ctx.lib.eofx_panel_colminmax_f32(ctx.handle, ptr(P), int(rows), L, ptr(mx), ptr(mn)), ctx.handle)
    return mx, mn


# --------------------------------------------------------------------------- #
# complex / Hilbert path                                                        #
# --------------------------------------------------------------------------- #
def hilbert(ctx: Context, mat: ResidentMatrix, padding="exp", decay_factor: float = 0.2, want_real: bool = False):
    """Analytic signal along the sample axis (xeofs/utils/hilbert_transform.py:40-72).
    Returns (imag ResidentMatrix, real ResidentMatrix | None).  As in the reference only
    padding == "exp" pads; any other value means no padding."""
    if mat.masked and want_real:      # (checked BEFORE the call: its two result matrices would leak)
        raise NotImplementedError("re-centred real part of a masked in-place matrix (preprocess with center=True)")
    hi, hr = C.c_void_p(), C.c_void_p()
    rc = ctx.lib.eofx_hilbert_f32(ctx.handle, mat.handle, int(padding == "exp"), float(decay_factor),
                                  C.byref(hi), C.byref(hr) if want_real else None)
    raise_for(rc, ctx.handle)
    B = ResidentMatrix(ctx, hi)
    # a masked in-place input (all-NaN grid points kept as zero columns): Im is a plain written matrix over the SAME physical
    # columns, zeros at the masked ones; `rsvd_c64(ctx, mat, B, ...)` compacts the feature axis of its factors through `mat`
    return B, (ResidentMatrix(ctx, hr) if want_real else None)


def cmat_mul(ctx: Context, A: ResidentMatrix, B: ResidentMatrix, P, conj_left: bool, final: bool = False, out=None):
    """one pass of Z = A + iB over a [Re | Im] panel: Z^H P (conj_left, P on the sample side) or Z P -- one launch"""
    torch = _torch()
    if out is None:
        out = torch.empty((A.p_pad if conj_left else A.n_pad, P.shape[1]), dtype=torch.float32, device=P.device)
    raise_for(ctx.lib.eofx_cmat_mul_f32(ctx.handle, A.handle, B.handle, int(conj_left), ptr(P), P.shape[1], int(final),
                                        ptr(out)), ctx.handle)
    return out


def hilbert_cmat_mul(ctx: Context, A: ResidentMatrix, P, conj_left: bool, padding="exp", decay_factor: float = 0.2,
                     final: bool = False, out=None):
    """the same pass for Z = (I + i Hc) A, Hc the resident Hilbert operator (eofx_hilbert_cmat_mul_f32): Im is never written"""
    torch = _torch()
    if out is None:
        out = torch.empty((A.p_pad if conj_left else A.n_pad, P.shape[1]), dtype=torch.float32, device=P.device)
    raise_for(ctx.lib.eofx_hilbert_cmat_mul_f32(ctx.handle, A.handle, int(padding == "exp"), float(decay_factor),
                                                int(conj_left), ptr(P), P.shape[1], int(final), ptr(out)), ctx.handle)
    return out


def cpanel_combine(ctx: Context, P1, P2, conj_left: bool, out=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(P1)
    raise_for(ctx.lib.eofx_cpanel_combine_f32(ctx.handle, ptr(P1), ptr(P2), int(conj_left), P1.shape[0],
                                              P1.shape[1], ptr(out)), ctx.handle)
    return out


def panel_colargminmax(ctx: Context, P, rows: int):
    torch = _torch()
    L = P.shape[1]
    amax = torch.empty(L, dtype=torch.int64, device=P.device)
    amin = torch.empty(L, dtype=torch.int64, device=P.device)
    raise_for(ctx.lib.eofx_panel_colargminmax_f32(ctx.handle, ptr(P), int(rows), L, ptr(amax), ptr(amin)), ctx.handle)
    return amax, amin


# --------------------------------------------------------------------------- #
# rotation steps                                                                #
# --------------------------------------------------------------------------- #
def panel_row_normalize(ctx: Context, P, out=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(P)
    raise_for(ctx.lib.eofx_panel_row_normalize_f32(ctx.handle, ptr(P), P.shape[0], P.shape[1], ptr(out)), ctx.handle)
    return out


def panel_rot_step(ctx: Context, X, R, aux, mode: int, power: float = 1.0):
    """one pass over the normalised loadings panel -> L x L float64 (device) ; see include/eofx.h"""
    torch = _torch()
    L = X.shape[1]
    G = torch.empty((L, L), dtype=torch.float64, device=X.device)
    raise_for(ctx.lib.eofx_panel_rot_step_f64(ctx.handle, ptr(X), X.shape[0], L, ptr(R), ptr(aux), int(mode),
                                              float(power), ptr(G)), ctx.handle)
    return G


def cpanel_colabsmax(ctx: Context, P, rows: int):
    """max over the rows of |column| for the L/2 complex columns of a [Re | Im] panel -> float32 device tensor [L/2]"""
    torch = _torch()
    L = P.shape[1]
    out = torch.empty(L // 2, dtype=torch.float32, device=P.device)
    raise_for(ctx.lib.eofx_cpanel_colabsmax_f32(ctx.handle, ptr(P), int(rows), L, ptr(out)), ctx.handle)
    return out


def vec_dot(ctx: Context, a, b) -> float:
    """float64 dot product of two equally sized float32 device tensors (fixed reduction tree)"""
    out = C.c_double()
    raise_for(ctx.lib.eofx_vec_dot_f64(ctx.handle, ptr(a), ptr(b), a.numel(), C.byref(out)), ctx.handle)
    return out.value


def resample(ctx: Context, mat: ResidentMatrix, rows, center: bool = True):
    """Bootstrap member of a resident matrix: rows drawn with replacement, re-centred.
    -> (ResidentMatrix, mean[p] float64, total_variance)"""
    if mat.masked:
        raise NotImplementedError("resampled copy of a masked in-place matrix (the bootstrapper works on the matrix in place)")
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    mean = np.empty(mat.p, np.float64)
    tv = C.c_double()
    h = C.c_void_p()
    raise_for(ctx.lib.eofx_resample_f32(ctx.handle, mat.handle, ptr(rows), rows.size, int(center), C.byref(h), ptr(mean),
                                        C.byref(tv)), ctx.handle)
    return ResidentMatrix(ctx, h), mean, tv.value


def panel_bootstrap(ctx: Context, P, n: int, idx, order, rowptr, transpose: bool, out=None):
    """H P (transpose False) or H^T P (True) of a bootstrap member on a sample-side panel (eofx_panel_bootstrap_f32);
    idx / order / rowptr: int64 device tensors describing the draw"""
    torch = _torch()
    if out is None:
        out = torch.empty_like(P)
    raise_for(ctx.lib.eofx_panel_bootstrap_f32(ctx.handle, ptr(P), int(n), P.shape[0], P.shape[1], ptr(idx), ptr(order),
                                               ptr(rowptr), int(bool(transpose)), ptr(out)), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# delay embedding of Extended EOF analysis (eofx_lag_*, csrc/eofx_lag.hpp)       #
# --------------------------------------------------------------------------- #
def lag_samples(mat: ResidentMatrix, tau: int, embedding: int) -> int:
    """n' = n - (embedding - 1) tau: the rows of the embedded matrix"""
    return mat.n - (int(embedding) - 1) * int(tau)


def lag_stats(ctx: Context, mat: ResidentMatrix, tau: int, embedding: int):
    """-> (window means mu as a float64 device tensor [embedding * p_pad], lag-major with zero padding rows; total variance
    of the centred embedded matrix)"""
    torch = _torch()
    mean = torch.empty(int(embedding) * mat.p_pad, dtype=torch.float64, device=f"cuda:{ctx.device}")
    tv = C.c_double()
    raise_for(ctx.lib.eofx_lag_stats_f64(ctx.handle, mat.handle, int(tau), int(embedding), ptr(mean), C.byref(tv)), ctx.handle)
    return mean, tv.value


def lag_tmul(ctx: Context, mat: ResidentMatrix, tau: int, embedding: int, mean, Zn, out=None, prec="f32"):
    """Ye[embedding * p_pad, L] = X_ext^T Zn - mu (1^T Zn), Zn[n'_pad, L]"""
    torch = _torch()
    L = Zn.shape[1]
    if out is None:
        out = torch.empty((int(embedding) * mat.p_pad, L), dtype=torch.float32, device=Zn.device)
    raise_for(ctx.lib.eofx_lag_tmul_f32(ctx.handle, mat.handle, int(tau), int(embedding), ptr(mean), ptr(Zn), L, ptr(out),
                                        _lib.PREC[prec]), ctx.handle)
    return out


def lag_mul(ctx: Context, mat: ResidentMatrix, tau: int, embedding: int, mean, Ye, out=None, prec="f32"):
    """Wn[n'_pad, L] = X_ext Ye - 1 (mu^T Ye), Ye[embedding * p_pad, L]"""
    torch = _torch()
    L = Ye.shape[1]
    if out is None:
        rows = (lag_samples(mat, tau, embedding) + 511) // 512 * 512
        out = torch.empty((rows, L), dtype=torch.float32, device=Ye.device)
    raise_for(ctx.lib.eofx_lag_mul_f32(ctx.handle, mat.handle, int(tau), int(embedding), ptr(mean), ptr(Ye), L, ptr(out),
                                       _lib.PREC[prec]), ctx.handle)
    return out


def lag_embed(ctx: Context, mat: ResidentMatrix, tau: int, embedding: int, out=None):
    """the embedded matrix X_ext [n', embedding * p] (not centred) as a float32 device tensor"""
    torch = _torch()
    shape = (lag_samples(mat, tau, embedding), int(embedding) * mat.p)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{ctx.device}")
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {shape} tensor")
    raise_for(ctx.lib.eofx_lag_embed_f32(ctx.handle, mat.handle, int(tau), int(embedding), ptr(out)), ctx.handle)
    return out


def panel_rownorm(ctx: Context, P, rows: int) -> np.ndarray:
    out = np.empty(rows, np.float64)
    raise_for(ctx.lib.eofx_panel_rownorm_f64(ctx.handle, ptr(P), rows, P.shape[1], ptr(out)), ctx.handle)
    return out


def feature_norms(ctx: Context, mat: ResidentMatrix) -> np.ndarray:
    """sqrt(sum over samples of x^2) per feature of the resident matrix"""
    out = np.empty(mat.p_phys, np.float64)
    raise_for(ctx.lib.eofx_mat_feature_norms_f64(ctx.handle, mat.handle, ptr(out)), ctx.handle)
    return out[mat.valid_index] if mat.masked else out


def sample_norms(ctx: Context, mat: ResidentMatrix) -> np.ndarray:
    """sqrt(sum over features of x^2) per sample of the resident matrix (no layout is built for an in-place matrix)"""
    out = np.empty(mat.n, np.float64)
    raise_for(ctx.lib.eofx_mat_sample_norms_f64(ctx.handle, mat.handle, ptr(out)), ctx.handle)
    return out


def _c64_arguments(ctx: Context, A: ResidentMatrix, k: int, n_oversamples: int, n_iter, random_state, omega, device_out: bool,
                   p_total=None):
    """the start matrix, the iteration code and the output buffers (omega, it, U, s, V) of the complex decompositions.
    p_total: A is this rank's slice of a field with `p_total` valid features over all ranks (n < p_total: the start matrix
    lives on the replicated sample side -- one draw, identical on every rank)."""
    if p_total is None:
        r, rows_v = min(A.n, A.p), A.p_phys
    else:
        if not A.n < int(p_total):
            raise ValueError("the sharded complex decomposition needs more features over all ranks than samples")
        r, rows_v = A.n, max(A.p_phys, 1)
    if k > r:
        raise ValueError(f"n_modes must be less than or equal to the rank of the dataset (rank = {r}).")
    omega = _sketch(r, k + n_oversamples, omega, random_state, identity_when_full=True, exact_rows=True)
    U, s, V = _factors_out(ctx, A.n, rows_v, k, np.complex64, device_out)
    return omega, _n_iter_code(n_iter, complex_rule=True), U, s, V


def rsvd_c64(ctx: Context, A: ResidentMatrix, B: ResidentMatrix, k: int, n_oversamples: int = 10, n_iter="auto",
             random_state=None, flip: bool = True, omega=None, device_out: bool = False):
    """complex randomized SVD of Z = A + iB (eofx_rsvd_c64) -> (U[n,k] complex64, s[k] float32, V[p,k] complex64);
    device_out: U and V stay on the device as torch complex64 tensors (V is 8 p k bytes: 166 MB at config 5)"""
    k = int(k)
    if B.masked:
        raise NotImplementedError("complex rSVD with a masked imaginary part (only the real part may be a masked in-place matrix)")
    if A.masked and (B.p_phys != A.p_phys or A.p < A.n):
        raise NotImplementedError("masked in-place real part: the imaginary part must cover the same physical columns and n < p")
    omega, it, U, s, V = _c64_arguments(ctx, A, k, n_oversamples, n_iter, random_state, omega, device_out)
    raise_for(ctx.lib.eofx_rsvd_c64(ctx.handle, A.handle, B.handle, k, int(n_oversamples), it, ptr(omega), int(flip),
                                    ptr(U), ptr(s), ptr(V)), ctx.handle)
    return U, s, A.compact_rows(V)       # (masked real part: the rows of the valid features)


def rsvd_sharded_c64(ctx: Context, A: ResidentMatrix, B: ResidentMatrix, k: int, p_total: int, n_oversamples: int = 10,
                     n_iter="auto", random_state=None, flip: bool = True, omega=None, device_out: bool = False):
    """`rsvd_c64` on this rank's slice of the feature axis (eofx_rsvd_sharded_c64; collectives through the communicator
    attached to the context) -> (U[n,k] replicated, s[k], V[p_local,k])"""
    k = int(k)
    if B.masked or (A.masked and B.p_phys != A.p_phys):
        raise NotImplementedError("masked in-place real part: the imaginary part must be a written matrix over the same physical columns")
    omega, it, U, s, V = _c64_arguments(ctx, A, k, n_oversamples, n_iter, random_state, omega, device_out, p_total=p_total)
    with _collective(ctx):
        rc = ctx.lib.eofx_rsvd_sharded_c64(ctx.handle, A.handle, B.handle, int(p_total), k, int(n_oversamples), it, ptr(omega),
                                           int(flip), ptr(U), ptr(s), ptr(V))
    raise_for(rc, ctx.handle)
    return U, s, A.compact_rows(V[:A.p_phys])


def rsvd_hilbert_sharded_c64(ctx: Context, A: ResidentMatrix, k: int, p_total: int, padding="exp", decay_factor: float = 0.2,
                             n_oversamples: int = 10, n_iter="auto", random_state=None, flip: bool = True, omega=None,
                             device_out: bool = False):
    """`rsvd_hilbert_c64` on this rank's slice (eofx_rsvd_hilbert_sharded_c64): the operator route of the analytic signal,
    feature-sharded -- every pass streams the rank's REAL slice once, the Hilbert operator acts on the replicated sample-side
    panel.  Reference: single/eof.py:546-555 -> linalg/decomposer.py:149-160."""
    k = int(k)
    omega, it, U, s, V = _c64_arguments(ctx, A, k, n_oversamples, n_iter, random_state, omega, device_out, p_total=p_total)
    with _collective(ctx):
        rc = ctx.lib.eofx_rsvd_hilbert_sharded_c64(ctx.handle, A.handle, int(p_total), int(padding == "exp"),
                                                   float(decay_factor), k, int(n_oversamples), it, ptr(omega), int(flip), ptr(U),
                                                   ptr(s), ptr(V))
    raise_for(rc, ctx.handle)
    return U, s, A.compact_rows(V[:A.p_phys])


HILBERT_OPERATOR_MAX_SAMPLES = 16384      # eofx_rsvd_hilbert_c64 holds the n x n operator resident (2 GB at the limit)


def rsvd_hilbert_c64(ctx: Context, A: ResidentMatrix, k: int, padding="exp", decay_factor: float = 0.2, n_oversamples: int = 10,
                     n_iter="auto", random_state=None, flip: bool = True, omega=None, device_out: bool = False):
    """complex randomized SVD of the analytic signal Z = A + i H(A) WITHOUT its imaginary part in memory
    (eofx_rsvd_hilbert_c64): the Hilbert stage is one n x n matrix along the samples, applied to the sample-side panels,
    and every product streams the real field once.  Same results as `rsvd_c64(ctx, A, hilbert(ctx, A)[0], ...)`
    (reference single/eof.py:433-447 + decomposer.py:149-160)."""
    k = int(k)
    if A.masked and A.p < A.n:
        raise NotImplementedError("masked in-place matrix with fewer valid features than samples")
    omega, it, U, s, V = _c64_arguments(ctx, A, k, n_oversamples, n_iter, random_state, omega, device_out)
    raise_for(ctx.lib.eofx_rsvd_hilbert_c64(ctx.handle, A.handle, int(padding == "exp"), float(decay_factor), k,
                                            int(n_oversamples), it, ptr(omega), int(flip), ptr(U), ptr(s), ptr(V)), ctx.handle)
    return U, s, A.compact_rows(V)


def hilbert_operator(ctx: Context, n: int, padding="exp", decay_factor: float = 0.2) -> np.ndarray:
    """Hc [n, n] float32 with Im = Hc A for the Hilbert stage along the samples (eofx_hilbert_operator_f32)"""
    out = np.empty((int(n), int(n)), np.float32)
    raise_for(ctx.lib.eofx_hilbert_operator_f32(ctx.handle, int(n), int(padding == "exp"), float(decay_factor), ptr(out)), ctx.handle)
    return out


def hilbert_sumsq(ctx: Context, A: ResidentMatrix, padding="exp", decay_factor: float = 0.2) -> float:
    """sum of squares of the imaginary part `hilbert(ctx, A)` would hold, without writing it (eofx_hilbert_sumsq_f64):
    total variance of the analytic signal = (A.sumsq() + this) / (n - 1)  (reference single/eof.py:93)"""
    out = C.c_double()
    raise_for(ctx.lib.eofx_hilbert_sumsq_f64(ctx.handle, A.handle, int(padding == "exp"), float(decay_factor), C.byref(out)),
              ctx.handle)
    return float(out.value)


# --------------------------------------------------------------------------- #
# geographically weighted PCA (eofx_gwpca_f64 / eofx_gw_cov_f64 / eofx_batched_syev_f64, csrc/eofx_gw.hpp)   #
# --------------------------------------------------------------------------- #
GW_METRICS = {"euclidean": 0, "haversine": 1}
GW_KERNELS = {"bisquare": 0, "gaussian": 1, "exponential": 2}
GW_EIG_PMAX = 64          # the batched Jacobi solver's limit; wider local covariances go to torch.linalg.eigh
GW_PMAX = 256             # the covariance kernel stages a neighbour tile of 16 x (p + 1) float64 in LDS
GW_LIB_CHUNK_BYTES = 256 << 20


def _gw_stats(st) -> dict:
    return dict(tile_pairs_visited=int(st[0]), tile_pairs_total=int(st[1]), chunks=int(st[2]), tiles=int(st[3]),
                ms_tiling=st[4] / 1e3, ms_covariance=st[5] / 1e3, ms_eigen=st[6] / 1e3, chunk=int(st[7]))


def batched_syev(ctx: Context, A, k: int):
    """A [batch, p, p] float64 device tensor (upper triangle read, p <= 64) -> (w [batch, k], V [batch, p, k]) float64 device
    tensors: the k largest eigenpairs, descending, clamped at 0, signed by the reference's deterministic rule"""
    torch = _torch()
    batch, p = A.shape[0], A.shape[1]
    A = A.to(torch.float64).contiguous()
    w = torch.empty((batch, int(k)), dtype=torch.float64, device=A.device)
    V = torch.empty((batch, p, int(k)), dtype=torch.float64, device=A.device)
    raise_for(ctx.lib.eofx_batched_syev_f64(ctx.handle, ptr(A), batch, p, int(k), ptr(w), ptr(V)), ctx.handle)
    return w, V


def gw_cov(ctx: Context, mat: ResidentMatrix, xy: np.ndarray, metric: str, kernel: str, bandwidth: float, first: int,
           count: int):
    """-> (local covariances C_i / W_i [count, p, p], total variances [count]) of locations [first, first + count), float64
    device tensors, and the tiling statistics"""
    torch = _torch()
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    cov = torch.empty((int(count), mat.p, mat.p), dtype=torch.float64, device=f"cuda:{ctx.device}")
    tv = torch.empty(int(count), dtype=torch.float64, device=cov.device)
    st = (C.c_int64 * 8)()
    raise_for(ctx.lib.eofx_gw_cov_f64(ctx.handle, mat.handle, xy.ctypes.data, GW_METRICS[metric], GW_KERNELS[kernel],
                                      float(bandwidth), int(first), int(count), ptr(cov), ptr(tv), st), ctx.handle)
    return cov, tv, _gw_stats(st)


def gwpca(ctx: Context, mat: ResidentMatrix, xy: np.ndarray, k: int, bandwidth: float, metric: str = "haversine",
          kernel: str = "bisquare", chunk: int | None = None):
    """Local PCAs of every location (row) of the resident matrix; xy [n, 2] = (lon, lat) in degrees or (x, y).
    -> (components [n, p, k] float32, explained_variance [n, k], total_variance [n], stats) as host arrays.
    p <= 64: one engine call (eofx_gwpca_f64).  Wider: eofx_gw_cov_f64 per chunk of locations, then the library's batched
    float64 eigensolver (torch.linalg.eigh), the same ordering, clamping and sign rule as the Jacobi kernel.  `chunk`:
    locations per chunk (None: the automatic size, whose buffers stay within 256 MiB)."""
    torch = _torch()
    n, p, k = mat.n, mat.p, int(k)
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.shape != (n, 2):
        raise ValueError(f"xy must have shape ({n}, 2), got {xy.shape}")
    dev = f"cuda:{ctx.device}"
    if p <= GW_EIG_PMAX:
        comps = torch.empty((n, p, k), dtype=torch.float32, device=dev)
        ev = torch.empty((n, k), dtype=torch.float64, device=dev)
        tv = torch.empty(n, dtype=torch.float64, device=dev)
        st = (C.c_int64 * 8)()
        raise_for(ctx.lib.eofx_gwpca_f64(ctx.handle, mat.handle, xy.ctypes.data, GW_METRICS[metric], GW_KERNELS[kernel],
                                         float(bandwidth), k, int(chunk or 0), ptr(comps), ptr(ev), ptr(tv), st), ctx.handle)
        return comps.cpu().numpy(), ev.cpu().numpy(), tv.cpu().numpy(), _gw_stats(st)
    if not 1 <= k <= p:
        raise ValueError(f"n_modes must be in [1, {p}], got {k}")
    comps = np.empty((n, p, k), np.float32)
    ev = np.empty((n, k))
    tv = np.empty(n)
    chunk = int(chunk) if chunk else max(1, GW_LIB_CHUNK_BYTES // (16 * p * p))
    agg = None
    for c0 in range(0, n, chunk):
        cnt = min(chunk, n - c0)
        cov, t, st = gw_cov(ctx, mat, xy, metric, kernel, bandwidth, c0, cnt)
        torch.cuda.synchronize(ctx.device)
        t_eig = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_eig[0].record()
        w, V = torch.linalg.eigh(cov)                                    # ascending
        del cov
        order = torch.sort(w, dim=1, descending=True, stable=True).indices[:, :k]
        w = torch.gather(w, 1, order).clamp_min(0.0)
        V = torch.gather(V, 2, order[:, None, :].expand(cnt, p, k))
        sign = torch.where(V.amax(dim=1).abs() >= V.amin(dim=1).abs(), 1.0, -1.0)
        V = V * sign[:, None, :]
        t_eig[1].record()
        comps[c0:c0 + cnt] = V.to(torch.float32).cpu().numpy()
        ev[c0:c0 + cnt] = w.cpu().numpy()
        tv[c0:c0 + cnt] = t.cpu().numpy()
        st["ms_eigen"] = t_eig[0].elapsed_time(t_eig[1])
        if agg is None:
            agg = dict(st, tile_pairs_total=0, tile_pairs_visited=0, tiles=0, chunks=0, ms_tiling=0.0, ms_covariance=0.0,
                       ms_eigen=0.0, chunk=chunk)
        for key in ("tile_pairs_total", "tile_pairs_visited", "tiles", "ms_tiling", "ms_covariance", "ms_eigen"):
            agg[key] += st[key]
        agg["chunks"] += 1
    return comps, ev, tv, agg


# --------------------------------------------------------------------------- #
# panels of the float64 kernel entries below: staging an input, validating a caller's output      #
# --------------------------------------------------------------------------- #
def device_panel(ctx: Context, A, name: str = "the panel", dtypes=None):
    """A host array or a device tensor -> a device tensor the float64 kernel entries read: two dimensions (ValueError naming
    `name` otherwise), one of `dtypes` (torch.float32 and torch.float64 by default; anything else becomes the first), unit
    column stride and a row stride of at least the columns.  What already is all that is returned as it is."""
    torch = _torch()
    dtypes = dtypes or (torch.float32, torch.float64)
    if not hasattr(A, "data_ptr"):
        A = np.asarray(A)
        host = {torch.float32: np.float32, torch.float64: np.float64}
        keep = [host[d] for d in dtypes if host[d] == A.dtype]
        A = torch.from_numpy(np.ascontiguousarray(A, dtype=keep[0] if keep else host[dtypes[0]]))
    A = A.to(f"cuda:{ctx.device}")
    if A.dim() != 2:
        raise ValueError(f"{name} must be a matrix, got {A.dim()} dimensions")
    if A.dtype not in dtypes:
        A = A.to(dtypes[0])
    if A.stride(1) != 1 or A.stride(0) < A.shape[1]:
        A = A.contiguous()
    return A


def _check_out(out, rows: int, cols: int, dtypes, what: str):
    """a caller's `out`: a device tensor [rows x cols] of one of `dtypes` with unit column stride, whose row stride may
    exceed the columns"""
    if (not hasattr(out, "data_ptr") or tuple(out.shape) != (rows, cols) or out.dtype not in dtypes
            or (rows and (out.stride(1) != 1 or out.stride(0) < cols))):
        raise ValueError(f"out must be a {what} device tensor of shape ({rows}, {cols}) with unit column stride")
    return out


# --------------------------------------------------------------------------- #
# lag-summed covariance of optimal persistence analysis (eofx_lagcov_f64, csrc/eofx_lagcov.hpp)   #
# --------------------------------------------------------------------------- #
LAGCOV_PMAX = 1024        # columns the kernels take
LAGCOV_FUSE_NTAU = 65     # up to here the filtered panel stays in LDS; beyond, it is written once


def _host_f64(a) -> np.ndarray:
    """a small operand of the filter entries (weights, trend), a host array or a tensor, as a contiguous float64 host array"""
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)


def lagcov(ctx: Context, S, w):
    """M [p x p] = sum_tau w[tau] S[:n - tau]^T S[tau:] (float64 device tensor) of a float32 panel S [n x p] -- a host
    array or a device tensor, whose row stride may exceed p -- and the weights w [ntau] of the lags 0 .. ntau - 1
    (opa.py:104-171 as one filter along the samples and one cross-product)"""
    torch = _torch()
    S = device_panel(ctx, S, "S", (torch.float32,))
    n, p = S.shape
    w = _host_f64(w)
    if w.ndim != 1:
        raise ValueError(f"w must be a vector of lag weights, got shape {w.shape}")
    M = torch.empty((p, p), dtype=torch.float64, device=S.device)
    raise_for(ctx.lib.eofx_lagcov_f64(ctx.handle, ptr(S), n, p, S.stride(0), ptr(w), w.size, ptr(M)), ctx.handle)
    return M


# --------------------------------------------------------------------------- #
# low-pass covariance of low-frequency component analysis (eofx_lowpass_cov_f64, csrc/eofx_lowpass.hpp)   #
# --------------------------------------------------------------------------- #
def _lowpass(ctx: Context, S, w, trend, want_r: bool, want_y: bool):
    torch = _torch()
    S = device_panel(ctx, S, "S", (torch.float32,))
    n, p = S.shape
    w = _host_f64(w)
    if w.ndim != 1 or w.size < 1:
        raise ValueError(f"w must be a vector of the h + 1 weights w_0 .. w_h, got shape {w.shape}")
    if trend is not None:
        trend = _host_f64(trend)
        if trend.shape != (2, p):
            raise ValueError(f"trend must have shape (2, {p}): the intercepts, then the slopes, got {trend.shape}")
    R = torch.empty((p, p), dtype=torch.float64, device=S.device) if want_r else None
    Y = torch.empty((n, p), dtype=torch.float64, device=S.device) if want_y else None
    raise_for(ctx.lib.eofx_lowpass_cov_f64(ctx.handle, ptr(S), n, p, S.stride(0), ptr(w), w.size - 1, ptr(trend), ptr(R),
                                           ptr(Y)), ctx.handle)
    return R, Y


def lowpass_cov(ctx: Context, S, w, trend=None, return_filtered: bool = False):
    """R [p x p] = Y^T Y (float64 device tensor, equal to its transpose bit for bit) of the low-passed panel
    Y[t, j] = sum_{k = -h .. h} w[|k|] d(refl(t + k), j) + (a_j + b_j t), d(u, j) = S[u, j] - (a_j + b_j u): S [n x p] a
    float32 panel -- a host array or a device tensor, whose row stride may exceed p --, w [h + 1] the weights of a symmetric
    filter (h <= n - 1), refl the mirror about the first and the last sample, `trend` [2 x p] the intercepts a and slopes b
    of a line removed before the filter and added back after it (None: no trend).  `return_filtered`: -> (R, Y)."""
    R, Y = _lowpass(ctx, S, w, trend, True, return_filtered)
    return (R, Y) if return_filtered else R


def lowpass(ctx: Context, S, w, trend=None):
    """Y [n x p] (float64 device tensor), the low-passed panel of `lowpass_cov`"""
    return _lowpass(ctx, S, w, trend, False, True)[1]


# --------------------------------------------------------------------------- #
# rank-order operator of trend EOF analysis (eofx_orderpos_f32, eofx_mat_orderpos_f32, csrc/eofx_orderpos.hpp)   #
# --------------------------------------------------------------------------- #
ORDERPOS_NMAX = 16384     # samples of a series the kernel sorts in LDS


def _orderpos_scale(scale, p: int):
    """the per-series factors as a float64 host vector or device tensor of p entries, or None"""
    if scale is None:
        return None
    if hasattr(scale, "data_ptr"):
        scale = scale.to(_torch().float64).contiguous()
    else:
        scale = np.ascontiguousarray(scale, dtype=np.float64)
    if tuple(scale.shape) != (p,):
        raise ValueError(f"scale must have one entry per series ({p}), got shape {tuple(scale.shape)}")
    return scale


def order_positions(ctx: Context, T, scale=None, want: str = "z", out=None):
    """The inverse ranks of every row of the SERIES-MAJOR float32 panel T [p x n] -- a host array or a device tensor, whose row
    stride may exceed n: q [p x n] (int32 device tensor), q[j, r] the 0-based time index of the r-th smallest value of
    series j, equal values in ascending time (numpy.argsort(kind="stable"), -0.0 equal to +0.0, NaNs last), and
    z [p x n] (float32 device tensor) = (q - (n - 1) / 2) * scale[j], the float64 product rounded once.  scale: [p] or None
    (ones).  want: "z", "q" or "both" (-> (q, z)).  out: the device tensor to write (a pair for "both"), whose row stride
    may exceed n."""
    torch = _torch()
    if want not in ("z", "q", "both"):
        raise ValueError(f'want must be "z", "q" or "both", got {want!r}')
    T = device_panel(ctx, T, "T", (torch.float32,))
    p, n = T.shape
    scale = _orderpos_scale(scale, p)
    outs = (None, None) if out is None else (tuple(out) if want == "both" else ((out, None) if want == "q" else (None, out)))
    if len(outs) != 2:
        raise ValueError('out must be the pair (q, z) for want="both"')
    q, z = outs
    if want != "z":
        q = (torch.empty((p, n), dtype=torch.int32, device=T.device) if q is None
             else _check_out(q, p, n, (torch.int32,), "int32"))
    if want != "q":
        z = (torch.empty((p, n), dtype=torch.float32, device=T.device) if z is None
             else _check_out(z, p, n, (torch.float32,), "float32"))
    ld = lambda a: n if a is None else a.stride(0)
    if p:       # (an empty tensor has no address to pass: p == 0 is a no-op of the entry as well)
        raise_for(ctx.lib.eofx_orderpos_f32(ctx.handle, ptr(T), p, n, ld(T), ptr(scale), ptr(q), ld(q), ptr(z), ld(z)), ctx.handle)
    return (q, z) if want == "both" else (q if want == "q" else z)


def rank_matrix(ctx: Context, mat: ResidentMatrix, weights=None) -> ResidentMatrix:
    """The resident matrix Z of `mat`: column j of Z = (the inverse ranks of column j of mat - (n - 1) / 2) * weights[j]
    (order_positions along the samples of every feature).  Reads the sample-contiguous layout of `mat` where it lies (built on
    demand; `mat.release_sample_layout()` drops it again) and writes the new matrix directly: no dense intermediate."""
    if mat.masked:
        raise ValueError("rank_matrix does not take a masked in-place matrix: compact it first")
    weights = _orderpos_scale(weights, mat.p)
    h = C.c_void_p()
    raise_for(ctx.lib.eofx_mat_orderpos_f32(ctx.handle, mat.handle, ptr(weights), C.byref(h)), ctx.handle)
    return ResidentMatrix(ctx, h)


# --------------------------------------------------------------------------- #
# quadratic-form operator of empirical orthogonal teleconnections (eofx_colquad_f32, eofx_mat_colquad_f32, csrc/eofx_colquad.hpp) #
# --------------------------------------------------------------------------- #
COLQUAD_NMAX = 16384      # samples the kernel takes: A is 1 GB there


def _colquad_operands(ctx: Context, A, n: int, p: int, out):
    """A [n x n] as a float32 device tensor (strides honoured) and the float64 device vector of p entries to write"""
    torch = _torch()
    A = device_panel(ctx, A, "A", (torch.float32,))
    if tuple(A.shape) != (n, n):
        raise ValueError(f"A must be a square matrix of the {n} samples, got shape {tuple(A.shape)}")
    if out is None:
        out = torch.empty(p, dtype=torch.float64, device=A.device)
    elif (not hasattr(out, "data_ptr") or tuple(out.shape) != (p,) or out.dtype != torch.float64 or not out.is_cuda
          or (p > 1 and out.stride(0) != 1)):
        raise ValueError(f"out must be a contiguous float64 device vector of {p} entries")
    return A, out


def colquad(ctx: Context, T, A, out=None):
    """q[j] = sum_s sum_t T[j, s] A[s, t] T[j, t] for every row of the SERIES-MAJOR float32 panel T [p x n] and any square
    float32 matrix A [n x n] -- host arrays or device tensors, whose row strides may exceed n.  -> a float64 device tensor of p
    entries (`out` when given).  float32 products and fma chains on the matrix cores, float64 from there on; no atomics: two
    calls are equal bit for bit, and q[j] depends on series j alone."""
    torch = _torch()
    T = device_panel(ctx, T, "T", (torch.float32,))
    p, n = T.shape
    A, out = _colquad_operands(ctx, A, n, p, out)
    if p:       # (an empty tensor has no address to pass: p == 0 is a no-op of the entry as well)
        raise_for(ctx.lib.eofx_colquad_f32(ctx.handle, ptr(T), p, n, T.stride(0), ptr(A), A.stride(0), ptr(out)), ctx.handle)
    return out


def mat_colquad(ctx: Context, mat: ResidentMatrix, A, out=None):
    """colquad on the columns of a resident matrix: q[j] = x_j^T A x_j, x_j the n samples of feature j.  Reads the
    sample-contiguous layout of `mat` where it lies (built on demand; `mat.release_sample_layout()` drops it again)."""
    if mat.masked:
        raise ValueError("mat_colquad does not take a masked in-place matrix: compact it first")
    A, out = _colquad_operands(ctx, A, mat.n, mat.p, out)
    if mat.p:
        raise_for(ctx.lib.eofx_mat_colquad_f32(ctx.handle, mat.handle, ptr(A), A.stride(0), ptr(out)), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# pairwise-minimum operator of the teleconnectivity map (eofx_pairmin_f32, eofx_mat_pairmin_f32, csrc/eofx_pairmin.hpp) #
# --------------------------------------------------------------------------- #
def _pairmin_operands(ctx: Context, w, p: int, out):
    """w [p] as a contiguous float32 device vector (a host array or a device tensor of any stride) and the pair of
    contiguous device vectors (float32 rmin, int32 partner) of p entries to write"""
    torch = _torch()
    if not hasattr(w, "data_ptr"):
        w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
    w = w.to(f"cuda:{ctx.device}")
    if tuple(w.shape) != (p,):
        raise ValueError(f"w must have one entry per series ({p}), got shape {tuple(w.shape)}")
    w = w.to(torch.float32).contiguous()
    if out is None:
        return w, (torch.empty(p, dtype=torch.float32, device=w.device), torch.empty(p, dtype=torch.int32, device=w.device))
    ok = isinstance(out, (tuple, list)) and len(out) == 2
    for o, dt in zip(out if ok else (), (torch.float32, torch.int32)):
        ok = ok and (hasattr(o, "data_ptr") and tuple(o.shape) == (p,) and o.dtype == dt and o.is_cuda
                     and not (p > 1 and o.stride(0) != 1))
    if not ok:
        raise ValueError(f"out must be a pair of contiguous device vectors of {p} entries: float32 (rmin), int32 (partner)")
    return w, tuple(out)


def pairmin(ctx: Context, T, w, out=None):
    """rmin[j] = min_i (d[j, i] w[j]) w[i], d[j, i] = sum_t T[j, t] T[i, t], over i != j with w[i] > 0 and a value that is not
    NaN, and partner[j] = the lowest i that attains it, for every row of the SERIES-MAJOR float32 panel T [p x n] -- a host
    array or a device tensor, whose row stride may exceed n -- and the float32 scales w [p].  (NaN, -1) where w[j] > 0 fails
    or no such i exists.  -> (rmin float32, partner int32) device tensors of p entries (`out` when given).  float32 fma chains
    on the matrix cores; the p x p matrix never exists; no atomics: two calls are equal bit for bit."""
    torch = _torch()
    T = device_panel(ctx, T, "T", (torch.float32,))
    p, n = T.shape
    w, out = _pairmin_operands(ctx, w, p, out)
    if p:       # (an empty tensor has no address to pass: p == 0 is a no-op of the entry as well)
        raise_for(ctx.lib.eofx_pairmin_f32(ctx.handle, ptr(T), p, n, T.stride(0), ptr(w), ptr(out[0]), ptr(out[1])), ctx.handle)
    return out


def mat_pairmin(ctx: Context, mat: ResidentMatrix, w, out=None):
    """pairmin on the columns of a resident matrix: series j = the n samples of feature j.  Reads the sample-contiguous
    layout of `mat` where it lies (built on demand; `mat.release_sample_layout()` drops it again)."""
    if mat.masked:
        raise ValueError("mat_pairmin does not take a masked in-place matrix: compact it first")
    w, out = _pairmin_operands(ctx, w, mat.p, out)
    if mat.p:
        raise_for(ctx.lib.eofx_mat_pairmin_f32(ctx.handle, mat.handle, ptr(w), ptr(out[0]), ptr(out[1])), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# the operators of archetypal analysis (eofx_simplex_rows_f32, eofx_simplex_pg_f32, csrc/eofx_simplex.hpp)       #
# --------------------------------------------------------------------------- #
SIMPLEX_MMAX = 16384        # entries of a row of simplex_rows
SIMPLEX_KMAX = 32           # variables of a problem of simplex_pg


def _simplex_out(out, like, what: str):
    """`out` of a simplex operator: None (a new contiguous tensor), or a float32 device tensor of the shape of `like` with unit
    column stride -- `like` itself among them (the operators work in place)"""
    torch = _torch()
    rows, cols = like.shape
    if out is None:
        return torch.empty((rows, cols), dtype=torch.float32, device=like.device)
    return _check_out(out, rows, cols, (torch.float32,), what)


def simplex_rows(ctx: Context, V, G=None, step: float = 0.0, out=None):
    """out[i] = the Euclidean projection of u[i] = fmaf(-step, G[i], V[i]) (u = V without G) onto the probability simplex
    {x >= 0, sum x = 1}, for every row of the float32 matrix V [r x m] -- a host array or a device tensor whose row stride may
    exceed m; G the same shape.  -> a float32 device tensor [r x m] (`out` when given; it may be V).  tau in float64 from
    Michelot's fixed point, the result rounded once; a row with a NaN or an infinity comes back all NaN; no atomics: two calls
    are equal bit for bit (include/eofx.h)."""
    torch = _torch()
    V = device_panel(ctx, V, "V", (torch.float32,))
    r, m = V.shape
    if G is not None:
        G = device_panel(ctx, G, "G", (torch.float32,))
        if tuple(G.shape) != (r, m):
            raise ValueError(f"G must have the shape of V {(r, m)}, got {tuple(G.shape)}")
    out = _simplex_out(out, V, "float32")
    if m < 1:
        raise ValueError(f"rows of at least one entry are required, got m = {m}")
    if r:       # (an empty tensor has no address to pass: r == 0 is a no-op of the entry as well)
        raise_for(ctx.lib.eofx_simplex_rows_f32(ctx.handle, ptr(V), r, m, V.stride(0), ptr(G), G.stride(0) if G is not None else 0,
                                                float(step), ptr(out), out.stride(0)), ctx.handle)
    return out


def simplex_pg(ctx: Context, A, Q, M, inv_L: float, iters: int, out=None):
    """`iters` steps of projected gradient descent on |x_i - a Z|^2 / 2 over the probability simplex, for every row i
    independently, in one launch: a <- P(a - inv_L (a M - Q[i])) from a = A[i], with Q = X Z^T [n x k] and M = Z Z^T [k x k].
    A, Q: float32, host arrays or device tensors whose row stride may exceed k; M: float64, a host array or a device tensor
    (rounded once to float32).  -> a float32 device tensor [n x k] (`out` when given; it may be A).  float32 fmaf chains, the
    projection of simplex_rows; rows are independent; two calls are equal bit for bit (include/eofx.h)."""
    torch = _torch()
    A = device_panel(ctx, A, "A", (torch.float32,))
    Q = device_panel(ctx, Q, "Q", (torch.float32,))
    n, k = A.shape
    if tuple(Q.shape) != (n, k):
        raise ValueError(f"Q must have the shape of A {(n, k)}, got {tuple(Q.shape)}")
    if hasattr(M, "data_ptr"):
        M = M.to(torch.float64).contiguous()
    else:
        M = np.ascontiguousarray(M, dtype=np.float64)
    if tuple(M.shape) != (k, k):
        raise ValueError(f"M must be {(k, k)}, got {tuple(M.shape)}")
    out = _simplex_out(out, A, "float32")
    if k < 1:
        raise ValueError(f"at least one variable is required, got k = {k}")
    if n:
        raise_for(ctx.lib.eofx_simplex_pg_f32(ctx.handle, ptr(A), A.stride(0), ptr(Q), Q.stride(0), ptr(M), float(inv_L), int(iters), n, k,
                                              ptr(out), out.stride(0)), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# the Lloyd solver of weather-regime clustering (eofx_kmeans_lloyd_f32, csrc/eofx_kmeans.hpp)                    #
# --------------------------------------------------------------------------- #
KMEANS_KMAX = 32            # clusters
KMEANS_QMAX = 32            # columns of the score panel
KMEANS_NMAX = 262144        # rows
KMEANS_RMAX = 4096          # restarts of one launch
KMEANS_ITER_MAX = 1000      # updates of one launch
_KMEANS_OUT = (("labels", "int32"), ("centroids", "float32"), ("counts", "int32"), ("inertia", "float64"), ("iters", "int32"),
               ("converged", "int32"), ("mind2", "float32"))


def kmeans_lloyd(ctx: Context, Z, C0, max_iter: int, out=None, want_mind2: bool = False) -> dict:
    """Lloyd's k-means iteration of R independent restarts on the float32 panel Z [n x q] -- a host array or a device tensor whose
    row stride may exceed q -- from the start centroids C0 [R x k x q] (float32, host or device; finite), all restarts and
    all iterations in one launch: assign (float32 fmaf chain of (z - c)^2, the lowest index among equals), stop when no label
    changed (converged = 1) or after `max_iter` <= KMEANS_ITER_MAX updates, otherwise update (float64 sums in a fixed order,
    an empty cluster keeps its centroid).  max_iter = 0 is the assignment alone.  -> a dict of device tensors: labels [R x n]
    int32 (-1 for a row with a NaN or an infinity), centroids [R x k x q] float32, counts [R x k] int32, inertia [R] float64,
    iters [R] int32, converged [R] int32 and, with `want_mind2`, mind2 [R x n] float32 -- all of them belonging to the
    returned centroids.  `out`: a dict holding any of these as contiguous device tensors to write (giving mind2 asks for it).
    Two calls are equal bit for bit; T chained calls with max_iter = 1 equal one call with max_iter = T (include/eofx.h)."""
    torch = _torch()
    Z = device_panel(ctx, Z, "Z", (torch.float32,))
    n, q = Z.shape
    if not hasattr(C0, "data_ptr"):
        C0 = torch.from_numpy(np.ascontiguousarray(C0, dtype=np.float32))
    if C0.dim() != 3 or C0.shape[2] != q:
        raise ValueError(f"C0 must be [R x k x q] with q = {q} columns, got shape {tuple(C0.shape)}")
    C0 = C0.to(device=Z.device, dtype=torch.float32).contiguous()
    R, k = int(C0.shape[0]), int(C0.shape[1])
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)):
        raise ValueError(f"max_iter must be an integer, got {max_iter!r}")
    if C0.numel() and not bool(torch.isfinite(C0).all()):
        raise ValueError("C0 holds a NaN or an infinity")
    shapes = dict(labels=(R, n), centroids=(R, k, q), counts=(R, k), inertia=(R,), iters=(R,), converged=(R,), mind2=(R, n))
    out = dict(out or {})
    if set(out) - set(shapes):
        raise ValueError(f"out holds unknown entries {sorted(set(out) - set(shapes))}")
    res = {}
    for name, dt in _KMEANS_OUT:
        dtype = getattr(torch, dt)
        t = out.get(name)
        if t is None:
            if name == "mind2" and not want_mind2:
                continue
            t = torch.empty(shapes[name], dtype=dtype, device=Z.device)
        elif (not hasattr(t, "data_ptr") or tuple(t.shape) != shapes[name] or t.dtype != dtype or not t.is_contiguous()
              or t.device != Z.device):
            raise ValueError(f"out[{name!r}] must be a contiguous {dt} device tensor of shape {shapes[name]}")
        res[name] = t
    raise_for(ctx.lib.eofx_kmeans_lloyd_f32(ctx.handle, ptr(Z), n, q, Z.stride(0) if n else q, ptr(C0), k, R, int(max_iter),
                                            ptr(res["labels"]), ptr(res["centroids"]), ptr(res["counts"]), ptr(res["inertia"]),
                                            ptr(res["iters"]), ptr(res["converged"]), ptr(res.get("mind2"))), ctx.handle)
    return res


# --------------------------------------------------------------------------- #
# the FastICA solver of independent component analysis (eofx_fastica_f32, csrc/eofx_ica.hpp)                      #
# --------------------------------------------------------------------------- #
ICA_QMAX = 32               # sources
ICA_NMAX = 4194304          # rows
ICA_RMAX = 1024             # restarts of one call
ICA_ITER_MAX = 64           # iterations of one call
ICA_FUNS = ("logcosh", "exp", "cube")
_ICA_OUT = (("W1", "float64"), ("gmean", "float64"), ("lim", "float64"), ("nused", "int64"))


def fastica(ctx: Context, Z, W, status, iters, fun: str = "logcosh", alpha: float = 1.0, tol: float = 1e-4, max_iter: int = 1,
            out=None, want=("W1", "gmean", "lim", "nused")) -> dict:
    """The parallel FastICA iteration of R independent restarts on the WHITE float32 panel Z [n x q] -- a host array or a device
    tensor whose row stride may exceed q.  W [R x q x q] float64, status [R] and iters [R] int32 are contiguous DEVICE tensors
    and are updated in place: every restart with status 0 advances by at most `max_iter` <= ICA_ITER_MAX iterations (project in
    float32, contrast `fun` in float32, float64 moments in a fixed order, symmetric decorrelation in float64), status 1 =
    converged (scikit-learn's lim < tol), 2 = degenerate.  max_iter = 0 is the moment pass alone for every restart.  -> a dict
    of the outputs named in `want` (or given in `out` as contiguous device tensors): W1 [R x q x q], gmean [R x q], lim [R]
    float64 and nused [1] int64, from the last moment pass a restart ran; an output not asked for is not written.  The call
    enqueues its launches and returns.  Two calls are equal bit for bit (include/eofx.h)."""
    torch = _torch()
    Z = device_panel(ctx, Z, "Z", (torch.float32,))
    n, q = Z.shape
    if fun not in ICA_FUNS:
        raise ValueError(f"fun must be one of {ICA_FUNS}, got {fun!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)):
        raise ValueError(f"max_iter must be an integer, got {max_iter!r}")
    if not hasattr(W, "data_ptr") or W.dim() != 3 or W.shape[1] != q or W.shape[2] != q or W.dtype != torch.float64 \
            or not W.is_contiguous() or W.device != Z.device:
        raise ValueError(f"W must be a contiguous float64 device tensor [R x q x q] with q = {q}")
    R = int(W.shape[0])
    for name, t in (("status", status), ("iters", iters)):
        if not hasattr(t, "data_ptr") or tuple(t.shape) != (R,) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != Z.device:
            raise ValueError(f"{name} must be a contiguous int32 device tensor of shape ({R},)")
    shapes = dict(W1=(R, q, q), gmean=(R, q), lim=(R,), nused=(1,))
    out = dict(out or {})
    if set(out) - set(shapes) or set(want) - set(shapes):
        raise ValueError(f"unknown outputs {sorted((set(out) | set(want)) - set(shapes))}")
    res = {}
    for name, dt in _ICA_OUT:
        dtype = getattr(torch, dt)
        t = out.get(name)
        if t is None:
            if name not in want:
                continue
            t = torch.zeros(shapes[name], dtype=dtype, device=Z.device)
        elif (not hasattr(t, "data_ptr") or tuple(t.shape) != shapes[name] or t.dtype != dtype or not t.is_contiguous()
              or t.device != Z.device):
            raise ValueError(f"out[{name!r}] must be a contiguous {dt} device tensor of shape {shapes[name]}")
        res[name] = t
    raise_for(ctx.lib.eofx_fastica_f32(ctx.handle, ptr(Z), n, q, Z.stride(0) if n else q, ptr(W), R, ICA_FUNS.index(fun), float(alpha),
                                       float(tol), int(max_iter), ptr(status), ptr(iters), ptr(res.get("W1")), ptr(res.get("gmean")),
                                       ptr(res.get("lim")), ptr(res.get("nused"))), ctx.handle)
    return res


# --------------------------------------------------------------------------- #
# the operators of spectral EOF analysis (eofx_blockxform_f32, eofx_mat_blockxform_f32, eofx_rowgram_f32, eofx_slabmul_f32, csrc/eofx_spectral.hpp) #
# --------------------------------------------------------------------------- #
BLOCKXFORM_NFFT_MAX = 16384       # samples per block
BLOCKXFORM_NCOEF_MAX = 8192       # rows of the coefficient matrix
ROWGRAM_RMAX = 512                # rows of a slab
ROWGRAM_SPAN = 2048               # features per float32 chain of rowgram
SLABMUL_QMAX = 16                 # rows of W[f]
SPECTRAL_NBMAX = 65535            # slabs per call of rowgram and slabmul


def _blockxform_operands(ctx: Context, B, p: int, hop, nblk, out):
    """B [ncoef x n_fft] as a float32 device tensor (strides honoured), hop and nblk as ints, and the contiguous float32 device
    tensor [ncoef x nblk x p] to write"""
    torch = _torch()
    B = device_panel(ctx, B, "B", (torch.float32,))
    ncoef = B.shape[0]
    hop, nblk = int(hop), int(nblk)
    if ncoef < 1 or B.shape[1] < 1 or nblk < 1:
        raise ValueError(f"B must have at least one row and one column and nblk must be >= 1, got B {tuple(B.shape)}, nblk = {nblk}")
    if out is None:
        out = torch.empty((ncoef, nblk, p), dtype=torch.float32, device=B.device)
    elif (not hasattr(out, "data_ptr") or tuple(out.shape) != (ncoef, nblk, p) or out.dtype != torch.float32 or not out.is_cuda
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 device tensor of shape ({ncoef}, {nblk}, {p})")
    return B, hop, nblk, out


def blockxform(ctx: Context, T, B, hop: int, nblk: int, out=None):
    """Q[c, b, j] = sum_t B[c, t] T[j, b hop + t] for every row of the SERIES-MAJOR float32 panel T [p x n] and the float32
    coefficient matrix B [ncoef x n_fft] -- host arrays or device tensors, whose row strides may exceed their columns: the
    transform along time of nblk blocks of n_fft samples, hop apart.  -> a float32 device tensor [ncoef x nblk x p] (`out`
    when given), j contiguous.  float32 fma chains over t ascending on the matrix cores; the overlapped blocks are never
    materialised; two calls are equal bit for bit, and Q[:, :, j] depends on series j alone."""
    torch = _torch()
    T = device_panel(ctx, T, "T", (torch.float32,))
    p, n = T.shape
    B, hop, nblk, out = _blockxform_operands(ctx, B, p, hop, nblk, out)
    if p:       # (an empty tensor has no address to pass: p == 0 is a no-op of the entry as well)
        raise_for(ctx.lib.eofx_blockxform_f32(ctx.handle, ptr(T), p, n, T.stride(0), ptr(B), B.shape[0], B.shape[1], B.stride(0),
                                              hop, nblk, ptr(out)), ctx.handle)
    return out


def mat_blockxform(ctx: Context, mat: ResidentMatrix, B, hop: int, nblk: int, out=None):
    """blockxform on the columns of a resident matrix: series j = the n samples of feature j.  Reads the sample-contiguous
    layout of `mat` where it lies (built on demand; `mat.release_sample_layout()` drops it again)."""
    if mat.masked:
        raise ValueError("mat_blockxform does not take a masked in-place matrix: compact it first")
    B, hop, nblk, out = _blockxform_operands(ctx, B, mat.p, hop, nblk, out)
    if mat.p:
        raise_for(ctx.lib.eofx_mat_blockxform_f32(ctx.handle, mat.handle, ptr(B), B.shape[0], B.shape[1], B.stride(0), hop, nblk,
                                                  ptr(out)), ctx.handle)
    return out


def _slabs(ctx: Context, R, name: str = "R"):
    """a batch of slabs [nb x r x p] as a contiguous float32 device tensor (a host array or a device tensor of any stride)"""
    torch = _torch()
    if not hasattr(R, "data_ptr"):
        R = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float32))
    R = R.to(f"cuda:{ctx.device}")
    if R.dim() != 3:
        raise ValueError(f"{name} must be a batch of matrices [nb x rows x columns], got {R.dim()} dimensions")
    return R.to(torch.float32).contiguous()


def _check_out3(out, shape, dtype, what: str):
    if (not hasattr(out, "data_ptr") or tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_cuda
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {what} device tensor of shape {tuple(shape)}")
    return out


def rowgram(ctx: Context, R, out=None):
    """G[f] = R[f] R[f]^T (float64 device tensor [nb x r x r], `out` when given) of a batch of float32 slabs R [nb x r x p] --
    a host array or a device tensor.  float32 fma chains on the matrix cores over spans of ROWGRAM_SPAN features, the spans
    added in float64 in a fixed order; no atomics: two calls are equal bit for bit, and G[f] equals its transpose bit for
    bit."""
    torch = _torch()
    R = _slabs(ctx, R)
    nb, r, p = R.shape
    if r < 1 or p < 1:
        raise ValueError(f"R must have at least one row and one column per slab, got shape {tuple(R.shape)}")
    out = (torch.empty((nb, r, r), dtype=torch.float64, device=R.device) if out is None
           else _check_out3(out, (nb, r, r), torch.float64, "float64"))
    if nb:
        raise_for(ctx.lib.eofx_rowgram_f32(ctx.handle, ptr(R), nb, r, p, ptr(out)), ctx.handle)
    return out


def slabmul(ctx: Context, W, R, out=None):
    """out[f] = W[f] R[f] (float32 device tensor [nb x q x p], `out` when given) of the float32 batches W [nb x q x r] and
    R [nb x r x p] -- host arrays or device tensors.  float32 fma chains over the r rows ascending; column j of out[f]
    depends on column j of R[f] alone."""
    torch = _torch()
    R = _slabs(ctx, R)
    W = _slabs(ctx, W, "W")
    nb, r, p = R.shape
    if W.shape[0] != nb or W.shape[2] != r or W.shape[1] < 1 or r < 1:
        raise ValueError(f"W must have shape ({nb}, q >= 1, {r}) to multiply R of shape {tuple(R.shape)}, got {tuple(W.shape)}")
    q = W.shape[1]
    out = (torch.empty((nb, q, p), dtype=torch.float32, device=R.device) if out is None
           else _check_out3(out, (nb, q, p), torch.float32, "float32"))
    if nb and p:
        raise_for(ctx.lib.eofx_slabmul_f32(ctx.handle, ptr(W), ptr(R), nb, q, r, p, ptr(out)), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# PC-space product of principal oscillation pattern analysis (eofx_pcmul_f64, csrc/eofx_pcmul.hpp)   #
# --------------------------------------------------------------------------- #
PCMUL_AMAX = 1024         # inner length the kernel takes (the PCA modes)
PCMUL_BMAX = 2048         # columns of the small matrix


def pcmul(ctx: Context, X, M, out_dtype=None, out=None):
    """Y [rows x b] = X [rows x a] M [a x b], accumulated in float64 on the matrix cores and rounded once to `out_dtype`
    (torch.float64, the default, or torch.float32) -- a device tensor.  X: a float32 or float64 panel, a host array or a
    device tensor whose row stride may exceed a; M: float64, a host array or a device tensor; `out`: a device tensor
    [rows x b] to write, whose row stride may exceed b."""
    torch = _torch()
    X = device_panel(ctx, X, "X")
    rows, a = X.shape
    if hasattr(M, "data_ptr"):
        M = M.to(torch.float64).contiguous()
    else:
        M = np.ascontiguousarray(M, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != a:
        raise ValueError(f"M must be a matrix of {a} rows, got shape {tuple(M.shape)}")
    b = M.shape[1]
    if out is None:
        out_dtype = torch.float64 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
        out = torch.empty((rows, b), dtype=out_dtype, device=X.device)
    else:
        _check_out(out, rows, b, (torch.float32, torch.float64), "float32 or float64")
    code = {torch.float32: 0, torch.float64: 1}      # EOFX_PCMUL_F32 | EOFX_PCMUL_F64
    raise_for(ctx.lib.eofx_pcmul_f64(ctx.handle, ptr(X), code[X.dtype], rows, a, X.stride(0) if rows else a, ptr(M), b, ptr(out),
                                     code[out.dtype], out.stride(0) if rows else b), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# block cross-covariance of multi-view CCA (eofx_viewcov_f64, csrc/eofx_viewcov.hpp)                 #
# --------------------------------------------------------------------------- #
VIEWCOV_PMAX = 4096       # columns the kernel takes (the views side by side)
VIEWCOV_MMAX = 64         # views


def viewcov(ctx: Context, Z, offsets, center=True, keep_diag=False, out=None):
    """C [p x p] (float64 device tensor) of a float32 panel Z [n x p] -- a host array or a device tensor, whose row stride may
    exceed p -- holding m views side by side, view v the columns offsets[v] .. offsets[v + 1] - 1: the covariance (ddof = 1)
    of columns in different views, +0.0 inside a view unless `keep_diag` (multi/cca.py:480-494 without the diagonal blocks
    it subtracts).  `center`: about the float64 column mean, computed on the device; else the raw second moment over
    n - 1.  Only the tiles on or above the diagonal are computed; C equals its transpose bit for bit.  `out`: a float64
    device tensor [p x p] to write, whose row stride may exceed p."""
    torch = _torch()
    Z = device_panel(ctx, Z, "Z", (torch.float32,))
    n, p = Z.shape
    off = np.asarray(offsets).reshape(-1)
    m = off.size - 1
    if n < 2:
        raise ValueError(f"the covariance needs n >= 2 samples, got n = {n}")
    if p > VIEWCOV_PMAX or m > VIEWCOV_MMAX:
        raise ValueError(f"the view covariance kernel takes p <= {VIEWCOV_PMAX} and m <= {VIEWCOV_MMAX}, got p = {p}, m = {m}")
    if m < 1 or off[0] != 0 or off[-1] != p or np.any(np.diff(off) <= 0) or np.any(off != np.floor(off)):
        raise ValueError(f"offsets must be integers strictly increasing from 0 to p = {p}, got {off.tolist()}")
    off = np.ascontiguousarray(off, dtype=np.int32)
    mean = torch.sum(Z, dim=0, dtype=torch.float64).div_(n).contiguous() if center else None
    if out is None:
        out = torch.empty((p, p), dtype=torch.float64, device=Z.device)
    else:
        _check_out(out, p, p, (torch.float64,), "float64")
    raise_for(ctx.lib.eofx_viewcov_f64(ctx.handle, ptr(Z), n, p, Z.stride(0), ptr(mean), ptr(off), m, int(bool(keep_diag)),
                                       ptr(out), out.stride(0)), ctx.handle)
    return out


# --------------------------------------------------------------------------- #
# gap operators of DINEOF (eofx_gapmask_f32 / eofx_lrfill_f32, csrc/eofx_lrfill.hpp)                  #
# --------------------------------------------------------------------------- #
LRFILL_KMAX = 256         # modes the fill takes
LRFILL_LDMAX = 1 << 26    # row stride of the field in entries


def gap_words(p: int) -> int:
    """32-bit words of one row of the gap mask of a field with p columns"""
    return (int(p) + 31) // 32


def _check_bits(bits, n: int, p: int):
    """a gap mask: an int32 device tensor [n x >= gap_words(p)] with unit column stride"""
    torch = _torch()
    if (not hasattr(bits, "data_ptr") or bits.dim() != 2 or bits.dtype != torch.int32 or not bits.is_cuda or bits.shape[0] != n
            or bits.shape[1] < gap_words(p) or (n and p and (bits.stride(1) != 1 or bits.stride(0) < gap_words(p)))):
        raise ValueError(f"bits must be an int32 device tensor of shape ({n}, >= {gap_words(p)}) with unit column stride")
    return bits


def _device_field(X, name: str):
    """a float32 device tensor [n x p] with unit column stride and a row stride of at least p, as it lies"""
    torch = _torch()
    if (not hasattr(X, "data_ptr") or not X.is_cuda or X.dim() != 2 or X.dtype != torch.float32
            or (X.shape[0] and X.shape[1] and (X.stride(1) != 1 or X.stride(0) < X.shape[1]))):
        raise ValueError(f"{name} must be a float32 device tensor of two dimensions with unit column stride")
    return X


def gap_mask(ctx: Context, X, out=None):
    """(bits, count) of a float32 device field X [n x p], whose row stride may exceed p: bit j & 31 of the int32 word
    bits[i, j >> 5] is set iff X[i, j] is NaN, the bits of columns >= p in the last word are 0; count: the set bits, exact.
    One streaming pass.  `out`: an int32 device tensor [n x >= gap_words(p)] to write (words past gap_words(p) are left)."""
    torch = _torch()
    X = _device_field(X, "X")
    n, p = X.shape
    bits = torch.empty((n, gap_words(p)), dtype=torch.int32, device=X.device) if out is None else _check_bits(out, n, p)
    count = C.c_int64()
    raise_for(ctx.lib.eofx_gapmask_f32(ctx.handle, ptr(X), n, p, X.stride(0) if n and p else p, ptr(bits),
                                       bits.stride(0) if n and p else gap_words(p), C.byref(count)), ctx.handle)
    return bits, int(count.value)


def lrfill(ctx: Context, F, bits, A, B):
    """F[i, j] <- sum_m A[i, m] B[j, m] at every entry of the float32 device field F [n x p] whose bit of the gap mask `bits`
    (`gap_mask`) is set, in place and nowhere else; A [n x k] (the scores U diag(s)) and B [p x k] (the components): float32
    panels, host arrays or device tensors whose row stride may exceed k, k <= LRFILL_KMAX.  Float32 products on the matrix
    cores (an fmaf chain per entry).  -> (count, sum (new - old)^2, sum new^2) over the written entries, the sums in float64
    and equal bit for bit between two runs."""
    torch = _torch()
    F = _device_field(F, "F")
    n, p = F.shape
    _check_bits(bits, n, p)
    A = device_panel(ctx, A, "A", (torch.float32,))
    B = device_panel(ctx, B, "B", (torch.float32,))
    k = A.shape[1]
    if A.shape[0] != n or B.shape != (p, k):
        raise ValueError(f"A must be ({n}, k) and B ({p}, k), got {tuple(A.shape)} and {tuple(B.shape)}")
    if k > LRFILL_KMAX:
        raise ValueError(f"the low-rank fill takes k <= {LRFILL_KMAX}, got k = {k}")
    if k < 1:
        raise ValueError("the low-rank fill needs k >= 1 modes")
    if n and p and F.stride(0) > LRFILL_LDMAX:
        raise ValueError(f"the low-rank fill takes a row stride of at most {LRFILL_LDMAX} entries, got {F.stride(0)}")
    sums = np.zeros(3, np.float64)
    live = bool(n and p)
    raise_for(ctx.lib.eofx_lrfill_f32(ctx.handle, ptr(F), n, p, F.stride(0) if live else p, ptr(bits),
                                      bits.stride(0) if live else gap_words(p), ptr(A), A.stride(0) if n else k, ptr(B),
                                      B.stride(0) if p else k, k, ptr(sums)), ctx.handle)
    return int(sums[0]), float(sums[1]), float(sums[2])
