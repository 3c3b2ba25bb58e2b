"""A float64 restatement of weather-regime clustering (xeofs_amd.single.KMeans, csrc/eofx_kmeans.hpp) for the tests: one
assignment with every row's relative margin, one Lloyd step, the whole loop with the kernel's stopping rule, the k-means++
seeding and the classifiability index.  Plain numpy, no GPU, nothing of the package.

A row is UNDECIDED when its margin (d_second - d_best) / d_second is at most 2 (q + 3) 2^-24: the float32 fmaf chain of the
kernel carries a relative error of about (q + 2) 2^-24 on either distance, so only such a row may take another label there.

The file also holds the case list of the GPU operator test (CASES) and its generators; test_kmeans_reference_cpu.py asserts
that the float64 reference alone keeps the share of undecided rows of every case within UNDECIDED_SHARE."""

import numpy as np

UNDECIDED_SHARE = 1e-3        # of the rows; a single row is always allowed
STEPS = 4                     # one-step launches the operator test replays per case


def undecided_margin(q: int) -> float:
    return 2.0 * (q + 3) * 2.0 ** -24


def allowed_undecided(n: int) -> int:
    return max(1, int(np.floor(UNDECIDED_SHARE * n)))


# ------------------------------------------------------------------------------------------------ the algorithm
def assign(Z, C):
    """-> (labels [n] int64, mind2 [n], margin [n]) in float64: d_ic = sum_j (z_ij - c_cj)^2, the lowest index among equals;
    a row with a NaN or an infinity gets label -1, mind2 = NaN and margin = 1.  margin = (d_second - d_best) / d_second, 1 for
    k = 1, 0 where d_second = 0."""
    Z, C = np.asarray(Z, np.float64), np.asarray(C, np.float64)
    n, k = Z.shape[0], C.shape[0]
    ok = np.isfinite(Z).all(axis=1)
    Zs = np.where(ok[:, None], Z, 0.0)
    d = ((Zs[:, None, :] - C[None, :, :]) ** 2).sum(axis=2)
    labels = np.argmin(d, axis=1)                       # (argmin: the first of equals)
    best = d[np.arange(n), labels]
    if k > 1:
        d2 = d.copy()
        d2[np.arange(n), labels] = np.inf
        second = d2.min(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(second > 0.0, (second - best) / second, 0.0)
    else:
        margin = np.ones(n)
    return np.where(ok, labels, -1), np.where(ok, best, np.nan), np.where(ok, margin, 1.0)


def update(Z, labels, C):
    """-> (C_new, counts): the float64 mean of the members; a cluster without rows keeps its centroid"""
    Z, C = np.asarray(Z, np.float64), np.array(C, np.float64)
    k = C.shape[0]
    counts = np.bincount(labels[labels >= 0], minlength=k)
    for c in range(k):
        if counts[c]:
            C[c] = Z[labels == c].sum(axis=0) / counts[c]
    return C, counts


def step(Z, C):
    """one launch with max_iter = 1 in float64: assign, update, assign -> dict(labels0, margin0, C, labels, mind2, margin,
    counts, inertia, converged)"""
    labels0, _, margin0 = assign(Z, C)
    C1, _ = update(Z, labels0, C)
    labels, mind2, margin = assign(Z, C1)
    counts = np.bincount(labels[labels >= 0], minlength=C1.shape[0])
    return dict(labels0=labels0, margin0=margin0, C=C1, labels=labels, mind2=mind2, margin=margin, counts=counts,
                inertia=float(np.nansum(mind2)), converged=int(np.array_equal(labels, labels0)))


def lloyd(Z, C0, max_iter: int):
    """the kernel's loop in float64: it = 0; assign; stop when it > 0 and no label changed (converged = 1) or it == max_iter;
    otherwise update, ++it.  -> dict(labels, C, counts, mind2, inertia, iters, converged, min_margin, inertias), min_margin the
    smallest margin met on the way and inertias the inertia of every assignment"""
    C = np.array(C0, np.float64)
    it, prev, min_margin, inertias = 0, None, np.inf, []
    while True:
        labels, mind2, margin = assign(Z, C)
        min_margin = min(min_margin, float(margin.min()))
        inertias.append(float(np.nansum(mind2)))
        if it > 0 and np.array_equal(labels, prev):
            converged = 1
            break
        if it == max_iter:
            converged = 0
            break
        C, _ = update(Z, labels, C)
        prev = labels
        it += 1
    counts = np.bincount(labels[labels >= 0], minlength=C.shape[0])
    return dict(labels=labels, C=C, counts=counts, mind2=mind2, inertia=inertias[-1], iters=it, converged=converged,
                min_margin=min_margin, inertias=inertias)


def kmeanspp_seeds(S, k: int, R: int, random_state=None) -> np.ndarray:
    """plain k-means++ (Arthur & Vassilvitskii 2007) in float64, R restarts from ONE RandomState(random_state) in restart order:
    the first centre randint(n); each further centre by one random_sample() u and a cumulative search: the first i whose
    cumulative D^2 exceeds u times the total (D^2: the squared distance to the nearest centre so far).  Where the total is 0
    the lowest index not yet taken.  -> [R x k] int64 sample indices"""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    rs = np.random.RandomState(random_state)
    out = np.empty((R, k), np.int64)
    for r in range(R):
        first = int(rs.randint(n))
        picks = [first]
        D2 = ((S - S[first]) ** 2).sum(axis=1)
        for _ in range(1, k):
            u = rs.random_sample()
            cum = np.cumsum(D2)
            if cum[-1] > 0.0:
                i = min(int(np.searchsorted(cum, u * cum[-1], side="right")), n - 1)
            else:
                i = min(set(range(n)) - set(picks))
            picks.append(i)
            D2 = np.minimum(D2, ((S - S[i]) ** 2).sum(axis=1))
        out[r] = picks
    return out


def classifiability(C) -> float:
    """C [R x k x q]: the mean over all ordered pairs of distinct restarts P, Q of min_i max_j cos(p_i, q_j) (Michelangeli et al.
    1995, eq. 6-7), a vector of norm 0 having cosine 0 with everything; NaN for R < 2"""
    C = np.asarray(C, np.float64)
    R = C.shape[0]
    if R < 2:
        return float("nan")
    nrm = np.linalg.norm(C, axis=2, keepdims=True)
    U = np.divide(C, nrm, out=np.zeros_like(C), where=nrm > 0)
    total = 0.0
    for a in range(R):
        for b in range(R):
            if a != b:
                total += (U[a] @ U[b].T).max(axis=1).min()
    return total / (R * (R - 1))


# ------------------------------------------------------------------------------------------------ the cases of the operator test
# (n, q, k, R, kind): every n of {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 4099}, q of {1, 2, 3, 4, 5, 16, 31, 32},
# k of {1, 2, 3, 31, 32, n} and R of {1, 2, 3, 300}
CASES = [
    (1, 1, 1, 1, "blobs"), (2, 2, 2, 2, "blobs"), (3, 4, 3, 1, "decades"), (63, 3, 3, 3, "blobs"), (64, 4, 31, 1, "decades"),
    (65, 5, 32, 2, "blobs"), (255, 16, 2, 3, "dups"), (256, 31, 3, 1, "blobs"), (257, 32, 32, 2, "blobs"), (511, 1, 3, 300, "blobs"),
    (513, 2, 31, 1, "dups"), (1025, 5, 3, 2, "decades"), (1025, 32, 1, 1, "blobs"), (4099, 16, 32, 3, "blobs"),
]


def case_id(case) -> str:
    n, q, k, R, kind = case
    return f"n{n}-q{q}-k{k}-R{R}-{kind}"


def case_seed(case) -> int:
    n, q, k, R, _ = case
    return 1000003 * n + 1009 * q + 31 * k + R


def make_case(case):
    """-> (Z [n x q] float32, C0 [R x k x q] float32: distinct rows of Z per restart)"""
    n, q, k, R, kind = case
    rs = np.random.RandomState(case_seed(case))
    if kind == "blobs":                     # min(k, 5) Gaussian blobs, four noise standard deviations apart
        nb = max(1, min(k, 5))
        Z = 4.0 * rs.standard_normal((nb, q))[rs.randint(nb, size=n)] + rs.standard_normal((n, q))
        pool = n
    elif kind == "decades":                 # ten decades of spread between the columns
        Z = rs.standard_normal((n, q)) * 10.0 ** np.linspace(-5.0, 5.0, q)
        pool = n
    elif kind == "dups":                    # the second half repeats the first row by row
        half = (n + 1) // 2
        Z = rs.standard_normal((half, q)) * 3.0
        Z = np.concatenate([Z, Z[: n - half]])
        pool = half                         # (seeds from the first half: distinct values)
    else:
        raise ValueError(kind)
    Z = Z.astype(np.float32)
    C0 = np.stack([Z[rs.choice(pool, size=k, replace=False)] for _ in range(R)])
    return Z, C0


# ------------------------------------------------------------------------------------------------ the planted field of the model test
PLANTED_SIZES = (240, 180, 120, 60)


def planted_field(n=600, p=2048, sizes=PLANTED_SIZES, sep=10.0, noise=0.05, seed=0):
    """-> (X [n x p] float64, labels [n] in 0 .. 3 by descending size): four blobs of unit standard deviation in a three-dimensional
    subspace of the features, their centres the corners of a regular tetrahedron of edge `sep` (ten noise standard deviations
    apart), plus white noise of standard deviation `noise` on every feature; the rows are shuffled"""
    rs = np.random.RandomState(seed)
    assert sum(sizes) == n
    basis = np.linalg.qr(rs.standard_normal((p, 3)))[0].T                     # 3 x p, orthonormal rows
    corners = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * sep / (2.0 * np.sqrt(2.0))
    labels = np.repeat(np.arange(len(sizes)), sizes)[rs.permutation(n)]
    X = (corners[labels] + rs.standard_normal((n, 3))) @ basis + noise * rs.standard_normal((n, p))
    return X, labels
