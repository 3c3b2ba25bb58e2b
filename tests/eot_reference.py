"""Float64 numpy restatements of empirical orthogonal teleconnections (van den Dool, Saha & Johansson 2000) for the tests of
xeofs_amd.single.EOT.  They share no code with the product.

  textbook(X, K)   the definition as it is written in the paper: the explicit p x p covariance of the residual field, the
                   explained variance of every point from its column, and the explicit deflation of the field by regression.
  gram_form(X, K)  the sample-space form the model uses: the n x n matrix G = X X^T, the projector I - T T^T applied to it as
                   an explicit matrix product, quadratic forms by einsum; the field is never changed.

Both take the centred (preprocessed) field X [n x p] and return the same dictionary:
  base [K] the base points, score [K] the variance-sum the base series explains (sum_i (x_i . r)^2 / |r|^2 on the residual
  field), series [n x K] the residual base series r_k, patterns [p x K] the regression beta_k of the residual field on r_k,
  all_scores [K x p] the score of every point at every step, den [K x p] the squared residual norm of every point.
`base=`: take these base points instead of the argmax (to follow a model's own choices through a near-tie).
"""

import numpy as np

MIN_RESIDUAL = 1e-3


def _pick(score, base, k):
    return int(np.argmax(score)) if base is None else int(base[k])


def _pack(base, score, series, patterns, all_scores, den):
    return dict(base=np.asarray(base, dtype=np.int64), score=np.asarray(score), series=np.stack(series, axis=1),
                patterns=np.stack(patterns, axis=1), all_scores=np.stack(all_scores), den=np.stack(den))


def textbook(X, K, min_residual=MIN_RESIDUAL, base=None):
    X = np.asarray(X, dtype=np.float64)
    c = np.sum(X * X, axis=0)
    Xr = X.copy()
    out = ([], [], [], [], [], [])
    for k in range(K):
        C = Xr.T @ Xr                                          # p x p
        d = np.diag(C).copy()
        ok = (d > min_residual * c) & (c > 0)
        score = np.zeros_like(d)
        score[ok] = np.sum(C[:, ok] ** 2, axis=0) / d[ok]
        b = _pick(score, base, k)
        r = Xr[:, b].copy()
        beta = Xr.T @ r / (r @ r)
        Xr = Xr - np.outer(r, beta)
        for lst, v in zip(out, (b, score[b], r, beta, score, d)):
            lst.append(v)
    return _pack(*out)


def gram_form(X, K, min_residual=MIN_RESIDUAL, base=None):
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    c = np.einsum("ij,ij->j", X, X)
    G = X @ X.T
    T = np.zeros((n, 0))
    out = ([], [], [], [], [], [])
    for k in range(K):
        P = np.eye(n) - T @ T.T
        A = P @ G @ P
        num = np.einsum("sj,st,tj->j", X, A, X)
        W = X.T @ T
        den = c - np.sum(W * W, axis=1)
        ok = (den > min_residual * c) & (c > 0)
        score = np.zeros(p)
        score[ok] = num[ok] / den[ok]
        b = _pick(score, base, k)
        r = P @ (P @ X[:, b])
        rn = np.sqrt(r @ r)
        T = np.concatenate([T, (r / rn)[:, None]], axis=1)
        beta = X.T @ (r / rn) / rn
        for lst, v in zip(out, (b, score[b], r, beta, score, den)):
            lst.append(v)
    return _pack(*out)


def transform(B, patterns, base):
    """the residual base series of a field from its base columns B [n x K]: column k of the field deflated by the series
    0 .. k - 1, each with the fitted pattern's value at base point k"""
    B = np.asarray(B, dtype=np.float64)
    K = B.shape[1]
    R = np.zeros_like(B)
    for k in range(K):
        r = B[:, k].copy()
        for m in range(k):
            r -= R[:, m] * patterns[base[k], m]
        R[:, k] = r
    return R


# ---------------------------------------------------------------------------------------------------- the designed field
DESIGNED_N = 40
DESIGNED_BASE = (5, 19, 26)            # the designated (noise-free) column of each block of twelve
DESIGNED_NORMS = (4.0, 3.0, 2.0)


def designed_field(seed=3):
    """n = 40, three orthogonal centred signals of norm 4, 3, 2; block m of twelve columns carries signal m with gains in
    [0.5, 1); every column but the designated one of its block gets 0.35 N(0, 1) noise.  -> X [40 x 36], float64, centred"""
    rng = np.random.default_rng(seed)
    n = DESIGNED_N
    S = rng.standard_normal((n, 3))
    S -= S.mean(axis=0)
    Q, _ = np.linalg.qr(S)                                     # orthonormal, and centred: the span of centred columns
    gains = 0.5 + 0.5 * rng.random((3, 12))
    noise = 0.35 * rng.standard_normal((n, 36))
    noise[:, list(DESIGNED_BASE)] = 0.0
    X = np.concatenate([np.outer(Q[:, m] * DESIGNED_NORMS[m], gains[m]) for m in range(3)], axis=1) + noise
    return X - X.mean(axis=0)
