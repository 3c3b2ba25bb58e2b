"""The steps the PC-space models share (OPA, LFCA, POP), as plain functions: a model reduces its field to q PCA modes, solves
a q x q problem on the host and carries the solution back with products of inner length q on the device.  A model calls
them in the order of its docstring equations and keeps what is its own."""

from __future__ import annotations

import numpy as np

from .. import engine


def whitened_modes(C0: np.ndarray, A: np.ndarray, k: int, rank_rows: int | None = None):
    """With C0 = E D E^T (symmetric, q x q) and K = D^-1/2 E^T: the k leading eigenpairs (values, Uo) of
    Tm = 1/2 (K A K^T + its transpose), values descending, Vq = K^T Uo and Wq = C0 Vq -> (values, Uo, Vq, Wq).  Float64 on the
    host (engine.host_eigh).  C0 is singular where its smallest eigenvalue is not positive or -- given `rank_rows` = n -- to
    the accuracy of float32 scores [n x q]: numpy.linalg.matrix_rank's rule on their singular values."""
    d, E = engine.host_eigh(C0)                                                 # descending
    if not d[-1] > 0.0 or (rank_rows and np.sqrt(d[-1]) <= max(rank_rows, d.size) * np.finfo(np.float32).eps * np.sqrt(d[0])):
        raise np.linalg.LinAlgError("the covariance of the PCA scores is singular: fewer independent modes than "
                                    f"n_pca_modes={C0.shape[0]}")
    K = E.T / np.sqrt(d)[:, None]
    Tm = K @ A @ K.T
    values, Uo = engine.host_eigh(0.5 * (Tm + Tm.T))                            # descending
    values, Uo = values[:k].copy(), np.ascontiguousarray(Uo[:, :k])
    Vq = K.T @ Uo                                                               # q x k
    return values, Uo, Vq, C0 @ Vq


def signed_projection(mul, patterns, scores, Vq: np.ndarray, Wq: np.ndarray):
    """filter patterns = patterns Vq, components = patterns Wq [P x k] and scores = scores Vq [n x k] by `mul(X, M)` -> X M, a
    float64 device product in a fixed order; one sign per mode from its component (positive where |max| >= |min|), the same
    on all three -> (those entries of a model's data, rounded once to float32, and the float64 `norms`; the signs [k])"""
    torch = engine._torch()
    k = Vq.shape[1]
    FW = mul(patterns, np.concatenate([Vq, Wq], axis=1))                        # P x 2k
    P = mul(scores, Vq)                                                         # n x k
    W = FW[:, k:]
    sgn = torch.where(W.amax(dim=0).abs() >= W.amin(dim=0).abs(), 1.0, -1.0).to(torch.float64)
    FW = FW * torch.cat([sgn, sgn])
    P = P * sgn
    norms = torch.sqrt((P * P).sum(dim=0)).cpu().numpy()
    host32 = lambda T: T.to(torch.float32).cpu().numpy()
    return dict(components=host32(FW[:, k:]), scores=host32(P), norms=norms, filter_patterns=host32(FW[:, :k])), sgn.cpu().numpy()


def project_modes(model, X, M: np.ndarray, out_dtype=None):
    """`transform`: new data -> the fitted preprocessing of `model` -> PC space (X V, float32) -> the product with the fitted
    M [q x m] (engine.pcmul) -> (Z [n' x m] on the host, fields, vs) for the preprocessor's inverse_transform_scores"""
    mat, fields, vs = model.preprocessor.transform(X)
    try:
        proj = engine.project(model.ctx, mat, model._pca_components)           # n' x q float32
    finally:
        mat.free()
    return engine.pcmul(model.ctx, proj, M, out_dtype).cpu().numpy(), fields, vs


def reconstruct(ctx, Z, C: np.ndarray) -> np.ndarray:
    """`inverse_transform`: Z C^T [n x P] (float64, host) of the float64 device panel Z [n x k'] and the components C [P x k']:
    products of inner length k' on the matrix cores, engine.pcmul over blocks of PCMUL_BMAX features"""
    rec = np.empty((Z.shape[0], C.shape[0]))
    for c0 in range(0, C.shape[0], engine.PCMUL_BMAX):
        Ct = np.ascontiguousarray(C[c0:c0 + engine.PCMUL_BMAX].T, dtype=np.float64)
        rec[:, c0:c0 + Ct.shape[1]] = engine.pcmul(ctx, Z, Ct).cpu().numpy()
    return rec
