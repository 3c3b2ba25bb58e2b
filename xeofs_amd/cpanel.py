"""The [Re | Im] layout of complex panels and the small algebra every complex model does in it.

A complex panel of m columns is a real float32 panel [rows_pad, 2 half], half >= m: real parts in columns [0, m),
imaginary parts in [half, half + m), zeros elsewhere.  The panel kernels only ever see the real panel; a complex matrix
acting on the right becomes a real one (`embed`), the real Gram matrix of a panel holds the four blocks of the complex
one (`block`), and the reference's +-1 sign rule (utils/xarray_utils.py:273-301, numpy's lexicographic complex max / min:
the real part decides, ties on it are measure-zero) reads two entries per column (`lex_extrema`, `lex_sign`).
`half` is the caller's: which widths a kernel takes is a kernel limit, not layout.
"""

from __future__ import annotations

import numpy as np

from . import engine


def embed(M, half_in, half_out=None):
    """real (2 half_in) x (2 half_out) float64 matrix E with [Pr | Pi] @ E = [Re(P M) | Im(P M)] for a complex M (l x m)"""
    half_out = half_in if half_out is None else half_out
    l, m = M.shape
    E = np.zeros((2 * half_in, 2 * half_out))
    E[:l, :m] = M.real
    E[half_in:half_in + l, :m] = -M.imag
    E[:l, half_out:half_out + m] = M.imag
    E[half_in:half_in + l, half_out:half_out + m] = M.real
    return E


def block(G, m, half, r0=0, c0=0, hermitian=False):
    """complex m x m product P^H Q from the real one G = [Pr | Pi]^T [Qr | Qi], whose top-left corner is at (r0, c0) of G;
    `hermitian` (Q = P): the rounding-level anti-Hermitian part is dropped"""
    rr, ri = G[r0:r0 + m, c0:c0 + m], G[r0:r0 + m, c0 + half:c0 + half + m]
    ir, ii = G[r0 + half:r0 + half + m, c0:c0 + m], G[r0 + half:r0 + half + m, c0 + half:c0 + half + m]
    H = (rr + ii) + 1j * (ri - ir)
    return 0.5 * (H + H.conj().T) if hermitian else H


def unpack(P, rows, m, half, dtype):
    """the first `rows` rows of a panel (numpy array or torch tensor) as a complex [rows, m] host array.  np.complex128:
    the parts widened to float64 and summed (host algebra goes on in double); np.complex64: the float32 parts as they are."""
    if engine._torch().is_tensor(P):
        P = P[:rows].detach()
        P = (P.double() if dtype == np.complex128 else P).cpu().numpy()
    re, im = P[:rows, :m], P[:rows, half:half + m]
    if dtype == np.complex128:
        return re.astype(np.float64) + 1j * im.astype(np.float64)
    out = np.empty((rows, m), np.complex64)
    out.real, out.imag = re, im
    return out


def pack(Z, half, out=None, c0=0):
    """Re / Im of the complex [r, m] host array Z into columns [c0, c0 + m) of both halves of `out` -- a host array or a
    device tensor, of which only these two r x m slices are written -- or of a new zeroed float32 [r, 2 half] host panel"""
    r, m = Z.shape
    if out is None:
        out = np.zeros((r, 2 * half), np.float32)
    for c, part in ((c0, Z.real), (half + c0, Z.imag)):
        out[:r, c:c + m] = part if isinstance(out, np.ndarray) else engine._torch().as_tensor(part, dtype=out.dtype)
    return out


def lex_extrema(P, amax, amin, k, half, conj=False):
    """(re, im) of the lexicographic max and min of the first k complex columns of the panel P (a tensor), given the rows
    of the largest / smallest real part per column (`panel_colargminmax`; index tensors on any device); `conj`: of the
    conjugated panel.  -> (mr, mi, nr, ni), float64 arrays of k values"""
    cols = engine._torch().arange(k, device=P.device)
    out = []
    for ix in (amax, amin):
        ix = ix[:k].to(P.device)
        out += [P[ix, cols].double().cpu().numpy(), P[ix, cols + half].double().cpu().numpy()]
    if conj:
        out[1], out[3] = -out[1], -out[3]
    return tuple(out)


def lex_sign(mr, mi, nr, ni):
    """+1 where |max| >= |min| per column, else -1"""
    return np.where(np.hypot(mr, mi) >= np.hypot(nr, ni), 1.0, -1.0)


def permute_export(ctx, P, rows, idx, w, half):
    """column j of the result = column idx[j] of the panel P times w[j] (one embedded matmul on the device)
    -> [rows, len(idx)] complex64 on the host"""
    k = idx.size
    M = np.zeros((k, k), dtype=complex)
    M[idx, np.arange(k)] = w
    out = engine.panel_matmul(ctx, P, engine._torch().as_tensor(embed(M, half), device=P.device))
    return unpack(out, rows, k, half, np.complex64)
