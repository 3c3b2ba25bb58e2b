"""Extended-precision references and designed inputs for the Cholesky-QR chain (panel Gram -> R^-1 -> P R^-1), no GPU.

Arithmetic: numpy's long double where it is wider than float64 (the 64-bit significand of x86: unit roundoff 2^-64); where
it is not, mpmath numbers at 80 bits in object arrays -- the same code, slower.  `to_f64` rounds once to float64.

References
  chol_rinv_ref(G, l, dead)   upper triangular R^-1 of the leading l x l block of G (float64 in) without the `dead` indices,
                              embedded back: zero rows / columns at the dead indices, zero outside l x l
  matmul_ref(P, M)            P M

Designed inputs (built in extended precision, rounded once)
  design_gram(l, seed, ...)   G = (B D)^T (B D): B [4 l x l] with unit columns, D = 10^U(-2, 2) per column -- after
                              unit-diagonal scaling the condition number is below 10.  `near={j: rho}` replaces column j by
                              sqrt(1 - rho) c + sqrt(rho) q with c a unit combination of two EARLIER columns (`parents`, default
                              j - 2 and j - 1) and q the unit part of the original column orthogonal to every other column (and to
                              the q of the other designed columns): the Schur pivot of column j over its original diagonal entry
                              is rho, and no other column moves.  `zero=[...]` zeroes columns (and their Gram rows) outright.
Random triangular factors are not used for this: they are exponentially ill-conditioned and produce dependent columns of
their own.
"""

import functools

import numpy as np

EXTENDED = np.finfo(np.longdouble).eps < 2.0 ** -60

if EXTENDED:
    def _x(a):
        return np.asarray(a, dtype=np.longdouble)

    _sqrt = np.sqrt
else:                                                          # pragma: no cover  (platforms whose long double is float64)
    import mpmath

    mpmath.mp.prec = 80
    _mpf = np.frompyfunc(lambda v: mpmath.mpf(float(v)) if not isinstance(v, mpmath.mpf) else v, 1, 1)
    _sqrt = np.frompyfunc(mpmath.sqrt, 1, 1)

    def _x(a):
        a = np.asarray(a)
        return a if a.dtype == object else np.asarray(_mpf(a), dtype=object)


extended = _x


def to_f64(a):
    """one rounding to float64"""
    return np.asarray(a).astype(np.float64)


def _zeros(shape):
    return _x(np.zeros(shape))


def matmul_ref(P, M):
    return _x(P) @ _x(M)


def _chol_upper(A):
    """R (upper triangular) with A = R^T R, right-looking; A extended, symmetric positive definite"""
    n = A.shape[0]
    A = A.copy()
    R = _zeros((n, n))
    for j in range(n):
        d = A[j, j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        R[j, j:] = A[j, j:] / _sqrt(d)
        if j + 1 < n:
            A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return R


def _upper_inverse(R):
    n = R.shape[0]
    X = _zeros((n, n))
    one = _x(1.0)
    for i in range(n - 1, -1, -1):
        row = -(R[i, i + 1:] @ X[i + 1:, :]) if i + 1 < n else _zeros(n)
        row[i] = row[i] + one
        X[i, :] = row / R[i, i]
        X[i, :i] = 0
    return X


def chol_rinv_ref(G, l, dead=()):
    """-> [L x L] extended: R^-1 of G[:l, :l] (G = R^T R) without the indices in `dead`, embedded as described above"""
    G = np.asarray(G)
    L = G.shape[0]
    keep = np.setdiff1d(np.arange(l), np.asarray(list(dead), dtype=int))
    out = _zeros((L, L))
    if keep.size:
        X = _upper_inverse(_chol_upper(_x(G[np.ix_(keep, keep)])))
        out[np.ix_(keep, keep)] = X
    return out


@functools.lru_cache(maxsize=None)
def _design(l, seed, near, parents, zero):
    rng = np.random.default_rng(seed)
    B = _x(rng.standard_normal((4 * l, l)))
    B = B / _sqrt((B * B).sum(axis=0))
    D = _x(10.0 ** rng.uniform(-2.0, 2.0, size=l))
    near, parents = dict(near), dict(parents)
    if near:
        J = sorted(near)
        X = _upper_inverse(_chol_upper(B.T @ B))
        Q = B @ (X @ X.T[:, J])                       # column t: orthogonal to every column of B but J[t]
        for t in range(len(J)):                       # ... and, after Gram-Schmidt among themselves, to each other
            for _ in range(2):
                for s in range(t):
                    Q[:, t] = Q[:, t] - (Q[:, s] @ Q[:, t]) * Q[:, s]
            Q[:, t] = Q[:, t] / _sqrt(Q[:, t] @ Q[:, t])
        cols = {}
        for t, j in enumerate(J):
            a, b = parents.get(j, (j - 2, j - 1))
            assert 0 <= a < j and 0 <= b < j and a != b and a not in near and b not in near
            wa, wb = _x(np.cos(0.7 + j)), _x(np.sin(0.7 + j))     # (two designed columns with the same parents still differ)
            c = wa * B[:, a] + wb * B[:, b]
            c = c / _sqrt(c @ c)
            rho = _x(near[j])
            cols[j] = _sqrt(1 - rho) * c + _sqrt(rho) * Q[:, t]
        for j, v in cols.items():
            B[:, j] = v
    P = B * D
    for j in zero:
        P[:, j] = 0
    G = to_f64(P.T @ P)
    G.setflags(write=False)
    Dh = to_f64(D)
    Dh.setflags(write=False)
    return G, Dh


def design_gram(l, seed=0, near=None, parents=None, zero=()):
    """-> G [l x l] float64 (read-only, cached), D [l]: see the module docstring"""
    near = tuple(sorted((near or {}).items()))
    parents = tuple(sorted((parents or {}).items()))
    return _design(int(l), int(seed), near, parents, tuple(sorted(zero)))


def embed(G, L, fill=None, seed=0):
    """G [l x l] in the leading block of an L x L float64 matrix; the rest is `fill` or, by default, N(0, 1) junk that a correct
    route never reads"""
    l = G.shape[0]
    out = np.random.default_rng(seed).standard_normal((L, L)) if fill is None else np.full((L, L), float(fill))
    out[:l, :l] = G
    return out


def scaled_error(X, Xref, G):
    """E = max |X - Xref|_ij sqrt(G_ii) / max |Xref_ij| sqrt(G_ii): row i of R^-1 carries 1 / D_i, which the weight removes
    (Cholesky rounding is invariant under the column scaling of the panel)"""
    w = _sqrt(_x(np.diag(np.asarray(G))))[:, None]
    num = np.abs(_x(X) - _x(Xref)) * w
    den = np.abs(_x(Xref)) * w
    return float(num.max() / den.max())


def numpy_rinv(G):
    return np.linalg.inv(np.linalg.cholesky(G).T)


def unit_diagonal_cond(G):
    """2-norm condition number of G scaled to a unit diagonal"""
    d = 1.0 / np.sqrt(np.diag(G))
    return float(np.linalg.cond(G * d[:, None] * d[None, :]))


# The designed dependent sets of tests/test_gpu_orth_chain.py: (name, l, design_gram keywords, expected dependent columns).
# tests/test_orth_reference_cpu.py runs every one of them through the host rule.
DEAD_ONE_WG = [
    ("zero-column", 17, dict(zero=[5]), [5]),
    ("zero-column-0", 17, dict(zero=[0]), [0]),
    ("zero-last-column", 64, dict(zero=[63]), [63]),
    ("two-panels", 33, dict(near={3: 1e-15, 12: 1e-15}), [3, 12]),
    ("pair-same-parents", 33, dict(near={10: 1e-15, 11: 1e-15}, parents={10: (0, 1), 11: (0, 1)}), [10, 11]),
    ("across-16-blocks", 64, dict(near={15: 1e-15, 16: 1e-15, 48: 1e-15}, parents={15: (0, 9), 16: (1, 10), 48: (2, 40)}, zero=[31]),
     [15, 16, 31, 48]),
]

# (name, l, L, keywords, dependent columns or None for "all alive, classification only").
# one to five 64-blocks: 192 merges [1,1,1] -> [2,1] -> [3] (uniform, then not), 320 [1,1,1,1,1] -> [2,2,1] -> [4,1] -> [5]
BLOCKED = [
    ("65", 65, 96, {}, []),
    ("127", 127, 128, {}, []),
    ("128", 128, 128, {}, []),
    ("129", 129, 160, {}, []),
    ("129-wide-output", 129, 256, {}, []),
    ("192", 192, 192, {}, []),
    ("320", 320, 320, {}, []),
    ("192-late-block", 192, 192, dict(near={130: 1e-15}, parents={130: (3, 70)}), [130]),          # d0_ext: the ORIGINAL diagonal
    ("192-block-edges", 192, 192,
     dict(near={64: 1e-15, 127: 1e-15, 128: 1e-15}, parents={64: (1, 40), 127: (2, 90), 128: (5, 100)}), [64, 127, 128]),
    ("129-last-column-zero", 129, 160, dict(zero=[128], near={7: 1e-15}), [7, 128]),
    ("320-every-block", 320, 320,
     dict(near={8: 1e-15, 100: 1e-15, 191: 1e-15, 192: 1e-15, 319: 1e-15},
          parents={100: (3, 70), 191: (64, 130), 192: (0, 129), 319: (63, 256)}), [8, 100, 191, 192, 319]),
    ("192-alive-at-1e-11", 192, 192, dict(near={130: 1e-11}, parents={130: (3, 70)}), None),
]
