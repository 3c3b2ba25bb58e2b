"""Sparse PCA by variable projection (eofx_spca_*_f64, csrc/eofx_spca.hpp): the bindings of its four kernel entries and
the solver built on them -- the thin SVD of the (compressed) matrix, the device loop or its fixed-order restatement for
shapes beyond the loop kernels' limits, the robust variant, and the randomized QB compression of a resident matrix.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import ptr, raise_for
from .engine import Context, ResidentMatrix, _torch, device_panel, panel_mul, panel_tmul, panel_width, sketch_matrix

SPCA_KMAX = 64            # the loop kernels' limits (modes, columns of V); wider shapes take the general route
SPCA_LMAX = 128
SPCA_REGULARIZERS = {"l1": 0, "l0": 1}
SPCA_GAMMA = 0.1          # outlier threshold of the robust route (compute_spca's default; the model never sets it)


def _dev64(ctx: Context, a):
    """a float64 C-contiguous device tensor of a numpy array / tensor"""
    return device_panel(ctx, a, "a", (_torch().float64,)).contiguous()


def spca_gram(ctx: Context, X, Y):
    """X^T Y [a x b] (float64 device tensor) of two float64 device tensors of the same rows, summed in a fixed order"""
    torch = _torch()
    rows, a = X.shape
    b = Y.shape[1]
    out = torch.empty((a, b), dtype=torch.float64, device=X.device)
    raise_for(ctx.lib.eofx_spca_gram_f64(ctx.handle, ptr(X), X.stride(0), a, ptr(Y), Y.stride(0) if Y.shape[0] > 1 else 0, b,
                                         rows, ptr(out)), ctx.handle)
    return out


def spca_sum(ctx: Context, X, absolute: bool = False) -> float:
    """sum of the entries (or of their absolute values) of a float64 device tensor in a fixed order"""
    torch = _torch()
    v = (X.abs() if absolute else X).reshape(-1, 1).contiguous()
    one = torch.ones((1, 1), dtype=torch.float64, device=X.device)
    return float(spca_gram(ctx, v, one).item())


def spca_rowmul(ctx: Context, X, M):
    """X [rows x a] M [a x b] -> [rows x b] float64 device tensor (M: host or device)"""
    torch = _torch()
    M = _dev64(ctx, M)
    rows, a = X.shape
    out = torch.empty((rows, M.shape[1]), dtype=torch.float64, device=X.device)
    raise_for(ctx.lib.eofx_spca_rowmul_f64(ctx.handle, ptr(X), X.stride(0), a, ptr(M), M.shape[1], rows, ptr(out),
                                           out.stride(0)), ctx.handle)
    return out


def spca_prox(ctx: Context, X, Y, s: float, regularizer: str, kappa: float, out=None):
    """prox(X + s Y, kappa) elementwise (Y None: prox(X)); soft threshold for "l1", hard threshold for "l0" """
    torch = _torch()
    if out is None:
        out = torch.empty_like(X)
    raise_for(ctx.lib.eofx_spca_prox_f64(ctx.handle, ptr(X), ptr(Y), float(s), X.numel(), SPCA_REGULARIZERS[regularizer],
                                         float(kappa), ptr(out)), ctx.handle)
    return out


def spca_orth(ctx: Context, T):
    """-> (Q, R) with T = Q R, Q [rows x c] orthonormal (float64 device), R [c x c] host, rows >= c.  CholeskyQR2 on the
    fixed-order Gram matrices; a (numerically) rank-deficient T takes the library's Householder QR instead."""
    torch = _torch()
    c = T.shape[1]
    Q, R = T, np.eye(c)
    for _ in range(2):
        G = spca_gram(ctx, Q, Q).cpu().numpy()
        try:
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            L = None
        d = None if L is None else np.abs(np.diag(L))
        if L is None or not np.all(np.isfinite(L)) or d.min() <= 1e-6 * d.max():
            Qh, Rh = torch.linalg.qr(T, mode="reduced")
            return Qh.contiguous(), Rh.cpu().numpy()
        Rs = L.T
        Q = spca_rowmul(ctx, Q, np.linalg.inv(Rs))
        R = Rs @ R
    return Q, R


def spca_svd(ctx: Context, Ct):
    """thin SVD C = U diag(D) V^T of C given as Ct = C^T [p x m] (float64 device) -> (V [p x r] float64 device, D [r] host),
    r = min(m, p), V's columns signed by the engine's rule (positive where |max| >= |min|)"""
    p, m = Ct.shape
    if m <= p:
        Q, R = spca_orth(ctx, Ct)                   # C^T = Q R, R = U_R S W^T  ->  V = Q U_R
        UR, D, _ = np.linalg.svd(R)
        V = spca_rowmul(ctx, Q, UR)
    else:
        _, R = spca_orth(ctx, Ct.T.contiguous())    # C = Q R, R = U_R S W^T  ->  V = W
        _, D, WT = np.linalg.svd(R)
        V = _dev64(ctx, WT.T)
    sign = (V.amax(dim=0).abs() >= V.amin(dim=0).abs()).to(V.dtype) * 2.0 - 1.0
    return (V * sign).contiguous(), np.asarray(D, dtype=np.float64)


def _spca_objective(D2, Qa, P, a2, b2, s1, s2):
    r = (((Qa - P) ** 2).sum(axis=1) + 1.0 - (Qa ** 2).sum(axis=1)) @ D2
    return 0.5 * r + a2 * s1 + 0.5 * b2 * s2


def spca_solve(ctx: Context, Ct, k: int, alpha: float = 1e-3, beta: float = 1e-3, regularizer: str = "l1",
               max_iter: int = 500, tol: float = 1e-6, check: bool = True, robust: bool = False):
    """Variable projection on C given as Ct = C^T [p x m] (float64 device): compute_spca (_sparse_pca.py:383-563).
    -> dict(B [p x k], A [p x k] (float64 device), dtilde [k], objective [n_iter], n_iter, route, ms)
    route "kernel": the device loop (eofx_spca_loop_f64, k <= 64 and r <= 128); "general": the same iteration as fixed-order
    products, the prox kernel and a host SVD of the small M; "robust": the robust variant on C itself."""
    import time

    torch = _torch()
    if regularizer not in SPCA_REGULARIZERS:
        raise ValueError(f'regularizer must be one of ("l1", "l0"), not {regularizer}.')
    if robust and regularizer == "l0":
        raise NotImplementedError("l0 regularization is not supported for robust sparse pca")
    p, m = Ct.shape
    k = int(k)
    if k > p:
        raise ValueError(f"n_components must be less than the number of columns of X ({p})")
    t0 = time.perf_counter()
    V, D = spca_svd(ctx, Ct)
    r = V.shape[1]
    if k > r:
        raise ValueError(f"n_modes ({k}) exceeds the rank bound min(rows, columns) = {r} of the decomposed matrix")
    torch.cuda.synchronize(ctx.device)
    ms_setup = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    if robust:
        out = _spca_robust(ctx, Ct, V, D, k, alpha, beta, max_iter, tol, check)
    elif k <= SPCA_KMAX and r <= SPCA_LMAX:
        B = torch.empty((p, k), dtype=torch.float64, device=V.device)
        Qa = np.empty((r, k))
        dt = np.empty(k)
        obj = np.empty(int(max_iter))
        it = C.c_int()
        raise_for(ctx.lib.eofx_spca_loop_f64(ctx.handle, ptr(V), p, r, ptr(D), k, float(alpha), float(beta),
                                             SPCA_REGULARIZERS[regularizer], int(max_iter), float(tol), int(bool(check)),
                                             ptr(B), ptr(Qa), ptr(dt), ptr(obj), C.byref(it)), ctx.handle)
        out = dict(B=B, A=spca_rowmul(ctx, V, Qa), dtilde=dt, objective=obj[:it.value].copy(), n_iter=it.value, route="kernel")
    else:
        out = _spca_general(ctx, V, D, k, alpha, beta, regularizer, max_iter, tol, check)
    torch.cuda.synchronize(ctx.device)
    out["ms"] = dict(setup=ms_setup, loop=1e3 * (time.perf_counter() - t0))
    return out


def _spca_scaled(D, alpha, beta):
    d0 = float(D[0]) ** 2
    if not d0 > 0.0:
        raise ValueError("the decomposed matrix is zero")
    a2, b2 = alpha * d0, beta * d0
    nu = 1.0 / (d0 + b2)
    return a2, b2, nu, nu * a2


def _spca_general(ctx, V, D, k, alpha, beta, regularizer, max_iter, tol, check):
    """the iteration of the loop kernels for shapes beyond their limits: fixed-order products on the device, the small
    polar factor on the host (LAPACK)"""
    a2, b2, nu, kappa = _spca_scaled(D, alpha, beta)
    D2 = D ** 2
    B = V[:, :k].contiguous()
    P = spca_gram(ctx, V, B).cpu().numpy()
    obj = []
    for it in range(int(max_iter)):
        U, dt, WT = np.linalg.svd(D2[:, None] * P, full_matrices=False)
        Qa = U @ WT
        G = spca_rowmul(ctx, V, D2[:, None] * (Qa - P))
        B = spca_prox(ctx, B, G - b2 * B, nu, regularizer, kappa)
        P = spca_gram(ctx, V, B).cpu().numpy()
        obj.append(_spca_objective(D2, Qa, P, a2, b2, spca_sum(ctx, B, True), spca_sum(ctx, B * B)))
        if check and it > 0 and abs(obj[-2] - obj[-1]) / obj[-1] < tol:
            break
    return dict(B=B, A=spca_rowmul(ctx, V, Qa), dtilde=dt, objective=np.array(obj), n_iter=len(obj), route="general")


def _spca_robust(ctx, Ct, V, D, k, alpha, beta, max_iter, tol, check):
    """robust variant (_sparse_pca.py:497-550) with the outlier matrix S kept as S^T [p x m] on the device; the polar
    factor of the tall Z through its k x k Gram matrix"""
    a2, b2, nu, kappa = _spca_scaled(D, alpha, beta)
    g = SPCA_GAMMA
    B = V[:, :k].contiguous()
    St = None
    obj = []
    for it in range(int(max_iter)):
        XSt = Ct if St is None else Ct - St
        XB = spca_gram(ctx, Ct, B)                               # C B        [m x k]
        Z = spca_rowmul(ctx, XSt, XB)                            # (C - S)^T C B   [p x k]
        w, E = np.linalg.eigh(spca_gram(ctx, Z, Z).cpu().numpy())
        w, E = w[::-1], E[:, ::-1]
        dt = np.sqrt(np.clip(w, 0.0, None))
        inv = np.where(dt > dt[0] * 1e-12, 1.0 / np.where(dt > 0, dt, 1.0), 0.0) if dt[0] > 0 else np.zeros_like(dt)
        A = spca_rowmul(ctx, Z, (E * inv) @ E.T)                 # polar(Z) = Z E S^-1 E^T
        Rt = XSt - spca_rowmul(ctx, A, XB.T)                     # (C - S - C B A^T)^T
        G = spca_rowmul(ctx, Ct, spca_gram(ctx, Rt, A)) - b2 * B  # C^T (R A) - beta B
        B = spca_prox(ctx, B, G, nu, "l1", kappa)
        Rt = Ct - spca_rowmul(ctx, A, spca_gram(ctx, Ct, B).T)
        St = spca_prox(ctx, Rt, None, 0.0, "l1", g)
        Rt = Rt - St
        obj.append(0.5 * spca_sum(ctx, Rt * Rt) + a2 * spca_sum(ctx, B, True) + 0.5 * b2 * spca_sum(ctx, B * B)
                   + g * spca_sum(ctx, St, True))
        if check and it > 0 and abs(obj[-2] - obj[-1]) / obj[-1] < tol:
            break
    return dict(B=B, A=A, dtilde=dt, objective=np.array(obj), n_iter=len(obj), route="robust")


def _spca_ops_resident(ctx: Context, mat: ResidentMatrix, rows=None):
    """(mul, tmul) of the rows `rows` (a range, None = all) of a resident matrix on float64 device tensors through the
    f32 panel products: mul(Z [p x c]) = X_b Z, tmul(Q [n_b x c]) = X_b^T Q"""
    torch = _torch()
    r0, r1 = (0, mat.n) if rows is None else rows

    def mul(Z):
        c = Z.shape[1]
        Yp = torch.zeros((mat.p_pad, panel_width(c)), dtype=torch.float32, device=Z.device)
        Yp[:mat.p, :c] = Z
        return panel_mul(ctx, mat, Yp)[r0:r1, :c].to(torch.float64).contiguous()

    def tmul(Q):
        c = Q.shape[1]
        Zn = torch.zeros((mat.n_pad, panel_width(c)), dtype=torch.float32, device=Q.device)
        Zn[r0:r1, :c] = Q
        return panel_tmul(ctx, mat, Zn)[:mat.p, :c].to(torch.float64).contiguous()

    return mul, tmul


def _spca_orth_cols(ctx, Y):
    """an orthonormal basis of Y's column space as scipy's economic QR gives it: [rows x min(rows, c)]"""
    rows, c = Y.shape
    if rows <= c:
        return _dev64(ctx, np.eye(rows))
    return spca_orth(ctx, Y)[0]


def _spca_qb(ctx, mul, tmul, p, l, n_subspace, omega):
    """_compute_rqb (_sparse_pca.py:170-218) -> K^T = X^T Q [p x min(rows, l)] (float64 device)"""
    Q = _spca_orth_cols(ctx, mul(omega))
    for _ in range(int(n_subspace)):
        Z = _spca_orth_cols(ctx, tmul(Q))
        Q = _spca_orth_cols(ctx, mul(Z))
    return tmul(Q)


def spca_compress(ctx: Context, mat: ResidentMatrix, k: int, oversample: int = 10, n_subspace: int = 1, n_blocks: int = 1,
                  random_state=None):
    """compute_rqb (_sparse_pca.py:221-333) on the resident matrix -> C^T [p x m_c] (float64 device) of the compressed
    matrix C = Q^T X.  The sketch Omega = standard_normal((p, k + oversample)) is engine.sketch_matrix's draw (an integer
    seed re-seeds at every draw, as check_random_state does).  n_blocks > 1: a QB per block of sample rows through the
    full-matrix products on row-sliced / zero-padded panels, then a QB of the stacked block outputs (fixed-order float64
    products)."""
    l = int(k) + int(oversample)
    p = mat.p
    if int(n_blocks) <= 1:
        mul, tmul = _spca_ops_resident(ctx, mat)
        return _spca_qb(ctx, mul, tmul, p, l, n_subspace, _dev64(ctx, sketch_matrix(p, l, random_state)))
    torch = _torch()
    bounds = np.array_split(np.arange(mat.n), int(n_blocks))
    Kt = []
    for b in bounds:
        if b.size == 0:
            continue
        mul, tmul = _spca_ops_resident(ctx, mat, (int(b[0]), int(b[-1]) + 1))
        Kt.append(_spca_qb(ctx, mul, tmul, p, l, n_subspace, _dev64(ctx, sketch_matrix(p, l, random_state))))
    Kt = torch.cat(Kt, dim=1).contiguous()                      # K^T [p x sum of the block ranks]
    mul = lambda Z: spca_gram(ctx, Kt, Z)                        # K Z
    tmul = lambda Q: spca_rowmul(ctx, Kt, Q)                     # K^T Q
    return _spca_qb(ctx, mul, tmul, p, l, n_subspace, _dev64(ctx, sketch_matrix(p, l, random_state)))
