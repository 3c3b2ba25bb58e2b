"""Float64 numpy restatement of trend EOF analysis (xeofs_amd/single/trend_eof.py, csrc/eofx_orderpos.hpp), sharing no code with
either: the checker of tests/test_gpu_orderpos.py and tests/test_gpu_trendeof.py, itself checked against brute force and the
closed forms in tests/test_trend_reference_cpu.py.

    order_positions(T)   Q[j, r] = the time index of the r-th smallest value of row j of T [p x n] (series-major, float32),
                         equal values in ascending time: numpy's stable argsort after -0.0 -> +0.0 and every NaN -> one
                         value above +inf (NaNs of any sign or payload sort last, in time order)
    rank_values(Q, s)    Z = np.float32((Q - (n - 1) / 2) * s[:, None]), the product formed in float64
    total_variance(n, w) n (n + 1) / 12 * sum w^2
    regression(X, S)     X^T Sh / (n - 1), Sh = (S - mean) / std(ddof = 1) per column
"""

import numpy as np


def normalised(T):
    """the float64 image the order is taken on: -0.0 -> +0.0; NaN -> one sentinel above +inf"""
    T = np.asarray(T)
    if T.dtype != np.float32:
        raise TypeError("ranks are defined on the float32 values")
    A = T.astype(np.float64) + 0.0          # -0.0 + 0.0 = +0.0
    big = np.float64(np.finfo(np.float64).max)
    inf = np.isposinf(A)
    A = np.where(np.isnan(A), np.inf, np.where(inf, big, A))     # +inf just below the NaNs' common value
    return A


def order_positions(T):
    """Q [p x n] int64 of the series-major panel T [p x n]"""
    return np.argsort(normalised(T), axis=1, kind="stable")


def rank_values(Q, scale=None):
    """Z [p x n] float32 = (Q - (n - 1) / 2) * scale[j], the float64 product rounded once"""
    Q = np.asarray(Q)
    p, n = Q.shape
    s = np.ones(p) if scale is None else np.asarray(scale, dtype=np.float64)
    return np.float32((Q.astype(np.float64) - (n - 1) / 2.0) * s[:, None])


def total_variance(n, w):
    w = np.asarray(w, dtype=np.float64)
    return n * (n + 1) / 12.0 * np.sum(w * w)


def standardized(S):
    S = np.asarray(S, dtype=np.float64)
    return (S - S.mean(axis=0)) / S.std(axis=0, ddof=1)


def regression(X, S):
    """[p x k]: the regression of the columns of X [n x p] on the standardized columns of S [n x k]"""
    X = np.asarray(X, dtype=np.float64)
    return X.T @ standardized(S) / (X.shape[0] - 1.0)


def restate(X, V, w=None):
    """the model's quantities from the preprocessed field X [n x p] (float32) and ITS OWN rank-space patterns V [p x k]"""
    X = np.asarray(X)
    n, p = X.shape
    w = np.ones(p) if w is None else np.asarray(w, dtype=np.float64)
    Q = order_positions(np.ascontiguousarray(X.T))
    Z = rank_values(Q, w).T                                  # [n x p] float32
    sv = np.linalg.svd(Z.astype(np.float64), compute_uv=False)
    S = X.astype(np.float64) @ np.asarray(V, dtype=np.float64)
    return dict(Q=Q, Z=Z, s=sv, total_variance=total_variance(n, w), scores=S, components=regression(X, S))


def brute_positions(row):
    """O(n^2) rank count of one float32 series: rank of sample t = #{u: x_u < x_t} + #{u < t: x_u == x_t}, NaNs above
    everything and equal to each other; Q[rank] = t"""
    x = np.asarray(row)
    n = x.size
    nan = np.isnan(x)
    q = np.empty(n, dtype=np.int64)
    for t in range(n):
        r = 0
        for u in range(n):
            if nan[t]:
                less = not nan[u]
                equal = nan[u]
            else:
                less = (not nan[u]) and x[u] < x[t]
                equal = (not nan[u]) and x[u] == x[t]        # -0.0 == +0.0
            r += 1 if less or (equal and u < t) else 0
        q[r] = t
    return q
