"""The float64 host algebra the SVD drivers run between their GPU passes (xeofs_amd/csrc/eofx_hostla.hpp and the
general-purpose solvers of eofx_hosteig.hpp) against numpy, without a GPU: the headers are plain C++, so
tests/hostla_shim.cpp (extern "C" wrappers and nothing else) is compiled here with the host C++ compiler and loaded through
ctypes.  Inputs from numpy.random.default_rng(seed); the reference is numpy in float64."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
c_int, c_double, c_void_p = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
NULLCOL_OK, NULLCOL_BAD, NULLCOL_DEPENDENT = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("hostla")
    so = str(d / "hostla_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           os.path.join(ROOT, "tests", "hostla_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    P, I, D = c_void_p, c_int, c_double
    for name, args in {
        "hl_chol_rinv_d": [P, I, I, P, D, P, P, P, D], "hl_chol_rinv_z": [P, I, I, P, D, P, P, P, D],
        "hl_chol_rinv_padded": [P, I, I, P, D], "hl_heigh": [P, I, P, P], "hl_hermitian_from_real": [P, I, I, P],
        "hl_embed_right": [P, I, I, I, I, I, P, P], "hl_null_column_transform": [P, I, I, I, I, P, P],
        "hl_zheigh_top_embedded": [P, P, I, I, P, P, P], "hl_peaked_spectrum": [P, I], "hl_product_norms": [P, P, I, I, I, P],
        "hl_ritz_block": [P, P, I, I, P], "hl_eigh": [P, I, P, P], "hl_zmatmul": [P, P, I, P],
        "hl_ritz_history": [P, P, I, I, I, I, I, I, P, P],
        "hl_null_repair_c": [P, ctypes.c_int64, I, I, I, I], "hl_ritz": [P, I, I, I, I, I, P, P, P, P, P, P, P, P],
    }.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = c_double if name == "hl_ritz_history" else c_int
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _gauss(rng, shape, cplx):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)


def _chol_rinv(lib, H, tol=1e-13, want_r=False, dref=None, tolref=0.0):
    """-> T, R (or None), n_live of hostla::chol_rinv on the square matrix H (float64 or complex128)"""
    l = H.shape[0]
    H = np.ascontiguousarray(H)
    T = np.full_like(H, 7.0)
    R = np.full_like(H, 7.0) if want_r else None
    live = c_int(-1)
    fn = lib.hl_chol_rinv_z if H.dtype == np.complex128 else lib.hl_chol_rinv_d
    fn(H.ctypes.data, l, l, T.ctypes.data, tol, _ptr(R), ctypes.addressof(live), _ptr(dref), tolref)
    return T, R, live.value


def _gram(rng, l, cplx):
    P = _gauss(rng, (4 * l, l), cplx) * (1.0 + 9.0 * rng.random(l))
    return P, P.conj().T @ P


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("l", [1, 2, 7, 64, 100])
def test_cholesky_inverse(lib, l, cplx):
    """T = R^-1 for H = P^H P = R^H R against inv(cholesky(H)^H) to 1e-9 max|T| (about 50 x l eps cond(H) at cond <= 1e3);
    strictly upper triangular; dead columns (a sum of two earlier ones, a zero one) are zero columns of T, counted by n_live,
    and drop out of the factorisation: the live block is numpy's on H without them and Rout reproduces H there."""
    rng = np.random.default_rng(100 * l + cplx)
    P, H = _gram(rng, l, cplx)
    assert np.linalg.cond(H) <= 1e3
    T, R, live = _chol_rinv(lib, H, want_r=True)
    Tn = np.linalg.inv(np.linalg.cholesky(H).conj().T)
    assert live == l
    assert np.abs(T - Tn).max() <= 1e-9 * np.abs(T).max()
    assert not np.tril(T, -1).any()
    assert np.abs(R.conj().T @ R - H).max() <= 1e-9 * np.abs(H).max()
    if l < 7:
        return
    dep, zero = 5, 3
    P[:, dep] = P[:, 0] + P[:, 2]
    P[:, zero] = 0.0
    H = P.conj().T @ P
    T, R, live = _chol_rinv(lib, H, want_r=True)
    keep = np.setdiff1d(np.arange(l), [dep, zero])
    Hk = H[np.ix_(keep, keep)]
    assert np.linalg.cond(Hk) <= 1e3
    assert live == l - 2
    assert not T[:, dep].any() and not T[:, zero].any() and not np.tril(T, -1).any()
    Tn = np.linalg.inv(np.linalg.cholesky(Hk).conj().T)
    assert np.abs(T[np.ix_(keep, keep)] - Tn).max() <= 1e-9 * np.abs(T).max()
    Rk = R[np.ix_(keep, keep)]
    assert np.abs(Rk.conj().T @ Rk - Hk).max() <= 1e-9 * np.abs(H).max()


@pytest.mark.parametrize("l", [1, 2, 7, 64, 100])
def test_cholesky_inverse_padded_layout(lib, l):
    """hostla::chol_rinv_padded, the host route of launch_rinv: the leading l x l block of an L x L matrix in, R^-1 out with rows
    and columns >= l exactly zero -- and the same numbers as the square form."""
    rng = np.random.default_rng(l)
    L = (l + 31) // 32 * 32
    _, H = _gram(rng, l, False)
    G = rng.standard_normal((L, L))           # (whatever lies outside the block is not read)
    G[:l, :l] = H
    R = np.full((L, L), 7.0)
    lib.hl_chol_rinv_padded(G.ctypes.data, L, l, R.ctypes.data, 1e-13)
    assert not R[l:].any() and not R[:, l:].any() and not np.tril(R, -1).any()
    assert np.array_equal(R[:l, :l], _chol_rinv(lib, H)[0])


@pytest.mark.parametrize("cplx", [False, True])
def test_cholesky_inverse_reference_diagonal_rule(lib, cplx):
    """dref / tolref: a column whose pivot is below tolref x dref[j] but above tol x its original diagonal entry dies -- only
    when dref is passed."""
    l, j = 7, 4
    rng = np.random.default_rng(5 + cplx)
    P, _ = _gram(rng, l, cplx)
    Q, _ = np.linalg.qr(P)
    Q[:, j] = Q[:, 0] + 1e-3 * Q[:, j]        # pivot 1e-6 of the squared length: far above 1e-13, below 1e-4
    H = Q.conj().T @ Q
    T, _, live = _chol_rinv(lib, H)
    assert live == l and T[j, j] != 0
    dref = np.ascontiguousarray(np.diag(H).real)
    T, _, live = _chol_rinv(lib, H, dref=dref, tolref=1e-4)
    assert live == l - 1 and not T[:, j].any() and all(T[i, i] != 0 for i in range(l) if i != j)
    T, _, live = _chol_rinv(lib, H, dref=dref, tolref=1e-8)
    assert live == l


@pytest.mark.parametrize("case", ["random", "equal5"])
@pytest.mark.parametrize("l", [1, 2, 7, 64])
def test_hermitian_eigensolver_through_the_real_embedding(lib, l, case):
    """hosteig::heigh (real symmetric embedding, every eigenvalue twice, Gram-Schmidt inside clusters) against numpy, at the
    tolerances of test_host_hermitian_top_eigensolver: values to 1e-12 of the norm, orthonormality to 1e-11, residual to
    1e-10 max|w| -- on a random Hermitian matrix and on one with five exactly equal leading eigenvalues."""
    rng = np.random.default_rng(10 * l + (case == "equal5"))
    A = _gauss(rng, (l, l), True)
    A = A + A.conj().T
    if case == "equal5":
        Q, _ = np.linalg.qr(A)
        lam = np.concatenate([np.full(5, 9.0), np.linspace(8, -3, max(l - 5, 0))])[:l]
        A = (Q * lam) @ Q.conj().T
        A = 0.5 * (A + A.conj().T)
    A = np.ascontiguousarray(A)
    w, V = np.zeros(l), np.zeros((l, l), complex)
    assert lib.hl_heigh(A.ctypes.data, l, w.ctypes.data, V.ctypes.data) == 0
    we = np.linalg.eigvalsh(A)[::-1]
    scale = np.abs(we).max()
    assert np.abs(w - we).max() <= 1e-12 * scale
    assert np.abs(V.conj().T @ V - np.eye(l)).max() <= 1e-11
    assert np.abs(A @ V - V * w).max() <= 1e-10 * np.abs(w).max()


@pytest.mark.parametrize("h,l", [(32, 7), (32, 32), (64, 40)])
def test_re_im_panel_helpers(lib, h, l):
    """A complex panel P of h columns as the real panel [Pr | Pi]: hermitian_from_real of its real Gram matrix is P^H P on the
    leading l x l block (1e-13 relative) and exactly Hermitian; embed_right(M) is the real matrix E with
    [Pr | Pi] E = [Re(P M) | Im(P M)], here with fewer columns than rows and another output width."""
    rng = np.random.default_rng(h + l)
    P = _gauss(rng, (50, h), True)
    Pri = np.ascontiguousarray(np.hstack([P.real, P.imag]))
    G = np.ascontiguousarray(Pri.T @ Pri)
    H = np.zeros((l, l), complex)
    assert lib.hl_hermitian_from_real(G.ctypes.data, 2 * h, l, H.ctypes.data) == 1
    He = (P.conj().T @ P)[:l, :l]
    assert np.abs(H - He).max() <= 1e-13 * np.abs(He).max()
    assert np.array_equal(H, H.conj().T)
    mcols, Lo, ko = 5, 32, 16
    M = np.ascontiguousarray(_gauss(rng, (l, mcols), True))
    E = np.full((2 * h, Lo), 7.0)
    lib.hl_embed_right(M.ctypes.data, mcols, l, mcols, 2 * h, Lo, E.ctypes.data, None)
    PM = P[:, :l] @ M
    want = np.zeros((50, Lo))
    want[:, :mcols], want[:, ko:ko + mcols] = PM.real, PM.imag
    assert np.abs(Pri @ E - want).max() <= 1e-13 * np.abs(PM).max()
    # the leading 3 columns of a matrix with row stride mcols, scaled column by column (the final stage's Uh[:, :k] / s)
    cs = np.array([2.0, 0.0, -0.5])
    lib.hl_embed_right(M.ctypes.data, mcols, l, 3, 2 * h, Lo, E.ctypes.data, cs.ctypes.data)
    want[:] = 0.0
    want[:, :3], want[:, ko:ko + 3] = (PM[:, :3] * cs).real, (PM[:, :3] * cs).imag
    assert np.abs(Pri @ E - want).max() <= 1e-13 * np.abs(PM).max()
    G[0, 1] = np.inf
    assert lib.hl_hermitian_from_real(G.ctypes.data, 2 * h, l, H.ctypes.data) == 0
    # |W_j|^2 = |V_j|^2 + |K^H W_j|^2 from the diagonal of a Hermitian matrix and two cross-Gram blocks
    C2 = np.ascontiguousarray(rng.standard_normal((2, 2 * h, 2 * h)))
    blocks = [(c[:l, :l] + c[h:h + l, h:h + l]) + 1j * (c[:l, h:h + l] - c[h:h + l, :l]) for c in C2]
    dref = np.zeros(l)
    Hc = np.ascontiguousarray(He)
    lib.hl_product_norms(Hc.ctypes.data, C2.ctypes.data, 2, 2 * h, l, dref.ctypes.data)
    want_d = np.diag(He).real + sum((np.abs(b) ** 2).sum(axis=0) for b in blocks)
    assert np.abs(dref - want_d).max() <= 1e-13 * want_d.max()


def _null_panel(rng, first, rows=40, Lo=32):
    P = rng.standard_normal((rows, Lo))
    P[:, :first] = np.linalg.qr(P[:, :first])[0] if first else P[:, :0]
    return P


def _null_transform(lib, P, first, k, stop_at_bad=1):
    Lo = P.shape[1]
    G = np.ascontiguousarray(P.T @ P)
    M = np.full((Lo, Lo), 7.0)
    flag = np.full(Lo, -1, np.int32)
    rc = lib.hl_null_column_transform(G.ctypes.data, Lo, first, k, stop_at_bad, M.ctypes.data, flag.ctypes.data)
    return rc, M, flag


@pytest.mark.parametrize("first", [0, 2, 4])
def test_null_column_transform(lib, first):
    """One round of fix_null_columns' block Gram-Schmidt as a right factor hM: columns 0 .. k-1 of P hM are orthonormal
    (1e-12), the columns before `first` pass through an exact identity; a zero column and a column inside the span of the
    earlier ones are reported through the flags, with hM left unwritten.
    The pivot floor (1e-6) is relative to what a column keeps AFTER the orthonormal columns before `first`, so the rule sees a
    dependency only where a column of [first, k) takes part in it: the dependent case needs first < k - 1.  (A last column
    wholly inside the span of the kept ones is not reported -- measured at first = 4, column 4 = column 0 + column 1: status
    NULLCOL_OK; the driver's second round absorbs it.  That is the driver's rule as it stands and it is kept bit for bit.)"""
    k = 5
    rng = np.random.default_rng(first)
    P = _null_panel(rng, first)
    rc, M, flag = _null_transform(lib, P, first, k)
    assert rc == NULLCOL_OK and not flag.any()
    Q = (P @ M)[:, :k]
    assert np.abs(Q.T @ Q - np.eye(k)).max() <= 1e-12
    assert np.array_equal(M[:, :first], np.eye(32)[:, :first])      # (with the rows: the leading block is the identity)
    only_last = [int(j == k - 1) for j in range(32)]
    Pz = P.copy()
    Pz[:, k - 1] = 0.0
    rc, M, flag = _null_transform(lib, Pz, first, k)
    assert rc == NULLCOL_BAD and flag.tolist() == only_last and np.all(M == 7.0)
    rc, M, flag = _null_transform(lib, Pz, first, k, stop_at_bad=0)      # (after a successful round the factorisation decides)
    assert rc == NULLCOL_DEPENDENT and flag.tolist() == only_last and np.all(M == 7.0)
    if first == k - 1:
        return
    Pd = P.copy()
    Pd[:, k - 1] = 2.0 * Pd[:, 0] - Pd[:, k - 2]
    rc, M, flag = _null_transform(lib, Pd, first, k)
    assert rc == NULLCOL_DEPENDENT and flag.tolist() == only_last and np.all(M == 7.0)


def test_complex_null_column_repair(lib):
    """The complex driver's repair of the float32 small-side factor [Re | Im]: columns first_null .. k-1 (one zero, one inside
    the span of the others) come back orthonormal to 1e-5, the project's null-mode tolerance; the columns before keep their
    bits."""
    small, k, first_null, ko, Lo = 9, 6, 3, 16, 32
    rng = np.random.default_rng(9)
    Z = _gauss(rng, (small, k), True)
    Z[:, :first_null] = np.linalg.qr(Z[:, :first_null])[0]
    Z[:, 3] = 0.0
    Z[:, 4] = Z[:, 0] - 2j * Z[:, 1]
    hp = np.zeros((small, Lo), np.float32)
    hp[:, :k], hp[:, ko:ko + k] = Z.real, Z.imag
    before = hp.copy()
    lib.hl_null_repair_c(hp.ctypes.data, small, Lo, ko, first_null, k)
    out = hp[:, :k].astype(np.float64) + 1j * hp[:, ko:ko + k].astype(np.float64)
    keep = list(range(first_null)) + list(range(ko, ko + first_null))
    assert np.array_equal(hp[:, keep], before[:, keep])
    assert np.abs(out.conj().T @ out - np.eye(k)).max() <= 1e-5


@pytest.fixture(scope="module")
def krylov():
    """A Hermitian M of order 40, three orthonormal blocks K of l = 4 columns, W = M K as [Re | Im] panels of LP = 64 columns,
    and the real cross-Gram K^T W -- as the device forms it."""
    n, l, nb, LP = 40, 4, 3, 64
    rng = np.random.default_rng(40)
    M = _gauss(rng, (n, n), True)
    M = M + M.conj().T
    K = np.linalg.qr(_gauss(rng, (n, nb * l), True))[0]

    def panel(Z):          # n x (nb LP): block b = [Re | 0 | Im | 0]
        out = np.zeros((n, nb * LP))
        for b in range(nb):
            out[:, b * LP:b * LP + l] = Z[:, b * l:(b + 1) * l].real
            out[:, b * LP + LP // 2:b * LP + LP // 2 + l] = Z[:, b * l:(b + 1) * l].imag
        return out
    return dict(M=M, K=K, l=l, nb=nb, LP=LP, panel=panel, rng=rng)


def _ritz(lib, kr, W, nrow, nWr, nbr, rf=None, hqq=None, X=None):
    l, LP = kr["l"], kr["LP"]
    hCf = np.ascontiguousarray(kr["panel"](kr["K"])[:, :nrow * LP].T @ kr["panel"](W)[:, :nWr * LP])
    Rf = np.zeros((nWr, l, l), complex)
    has = np.zeros(nWr, np.int32)
    for b, r in (rf or {}).items():
        Rf[b], has[b] = r, 1
    m = nbr * l
    Hr, Hi, res = np.zeros((m, m)), np.zeros((m, m)), np.zeros(l)
    Xr = Xi = None
    if X is not None:
        Xr, Xi = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    lib.hl_ritz(hCf.ctypes.data, nrow, nWr, nbr, LP, l, Rf.ctypes.data, has.ctypes.data, _ptr(hqq), Hr.ctypes.data, Hi.ctypes.data,
                _ptr(Xr), _ptr(Xi), res.ctypes.data if X is not None else None)
    return Hr + 1j * Hi, res


def test_rayleigh_ritz_assembly_and_residual(lib, krylov):
    """ritz_assemble: H = K^H M K (1e-12 |M|, exactly Hermitian) from the real cross-Gram of the [Re | Im] panels -- with one block
    given through a non-identity Rf (M Z_b = W_b Rf[b]), with the last diagonal block replaced, and with the newest block not
    yet multiplied (its row and column come from the other reading, its diagonal block from Hqq).  ritz_residual: the norm of
    block row nbr of (K^H M K) y, the coupling of the Ritz vectors to the block outside."""
    kr = krylov
    M, K, l, nb, rng = kr["M"], kr["K"], kr["l"], kr["nb"], kr["rng"]
    He = K.conj().T @ M @ K
    tol = 1e-12 * np.linalg.norm(M, 2)
    W = M @ K
    H, _ = _ritz(lib, kr, W, nb, nb, nb)
    assert np.abs(H - He).max() <= tol and np.array_equal(H, H.conj().T)
    # block 1 stored as W_1 Rf^-1
    Rf = np.triu(_gauss(rng, (l, l), True)) + 3.0 * np.eye(l)
    W2 = W.copy()
    W2[:, l:2 * l] = W[:, l:2 * l] @ np.linalg.inv(Rf)
    H, _ = _ritz(lib, kr, W2, nb, nb, nb, rf={1: Rf})
    assert np.abs(H - He).max() <= tol and np.array_equal(H, H.conj().T)
    # the last diagonal block replaced
    Hqq = np.ascontiguousarray(_gauss(rng, (l, l), True))
    H, _ = _ritz(lib, kr, W, nb, nb, nb, hqq=Hqq)
    want = He.copy()
    want[-l:, -l:] = 0.5 * (Hqq + Hqq.conj().T)
    assert np.abs(H - want).max() <= tol and np.array_equal(H, H.conj().T)
    # the newest block not yet multiplied (nWr < nbr): its diagonal block is P^H P of its tall panel
    Hqq = np.ascontiguousarray(He[-l:, -l:])
    H, _ = _ritz(lib, kr, W, nb, nb - 1, nb, hqq=Hqq)
    assert np.abs(H - He).max() <= tol and np.array_equal(H, H.conj().T)
    # the coupling residual: Ritz pairs over the first two blocks, block row 2
    nbr = nb - 1
    H2, _ = _ritz(lib, kr, W, nbr, nbr, nbr)
    X = np.ascontiguousarray(np.linalg.eigh(H2)[1][:, ::-1][:, :l])
    H2b, res = _ritz(lib, kr, W, nbr + 1, nbr, nbr, X=X)
    assert np.array_equal(H2, H2b)
    want = np.linalg.norm((He @ np.vstack([X, np.zeros((l, l))]))[nbr * l:], axis=0)
    assert np.abs(res - want).max() <= 1e-12
    Xr, Xi = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    for b in range(nbr):        # ritz_block: block b of the split Ritz vectors as one complex l x l matrix
        yb = np.zeros((l, l), complex)
        lib.hl_ritz_block(Xr.ctypes.data, Xi.ctypes.data, b, l, yb.ctypes.data)
        assert np.array_equal(yb, X[b * l:(b + 1) * l])
    # the general-purpose route to the same leading pairs (the driver's fall-back), and the peaked-spectrum rule on their values
    m, Hr, Hi = nbr * l, np.ascontiguousarray(H2.real), np.ascontiguousarray(H2.imag)
    w, Xr, Xi = np.zeros(l), np.zeros((m, l)), np.zeros((m, l))
    assert lib.hl_zheigh_top_embedded(Hr.ctypes.data, Hi.ctypes.data, m, l, w.ctypes.data, Xr.ctypes.data, Xi.ctypes.data) == 0
    we, Xe = np.linalg.eigvalsh(H2)[::-1][:l], Xr + 1j * Xi
    assert np.abs(w - we).max() <= 1e-12 * np.abs(we).max() and np.abs(H2 @ Xe - Xe * w).max() <= 1e-10 * np.abs(we).max()
    for spec, want_peaked in (([900.0, 1.0], 0), ([901.0, 1.0], 1), ([5.0, 0.0], 1), ([5.0, -1.0], 1), ([3.0], 0)):
        spec = np.array(spec)
        assert lib.hl_peaked_spectrum(spec.ctypes.data, len(spec)) == want_peaked


@pytest.mark.parametrize("n", [1, 2, 7, 60])
def test_symmetric_eigensolver_and_small_product(lib, n):
    """hosteig::eigh (tred2 / tql2, the body of eofx_host_eigh_f64) against numpy at the tolerances of the Hermitian solvers: values
    descending to 1e-12 of the norm, orthonormal columns to 1e-11, residual to 1e-10 max|w|; and hostla::zmatmul against numpy's
    product, with an exactly zero entry in the left factor (the loop skips those)."""
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n))
    A = np.ascontiguousarray(A + A.T)
    w, V = np.zeros(n), np.zeros((n, n))
    assert lib.hl_eigh(A.ctypes.data, n, w.ctypes.data, V.ctypes.data) == 0
    we = np.linalg.eigvalsh(A)[::-1]
    assert np.abs(w - we).max() <= 1e-12 * np.abs(we).max()
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-11 and np.abs(A @ V - V * w).max() <= 1e-10 * np.abs(w).max()
    X, Y, Z = (np.ascontiguousarray(_gauss(rng, (n, n), True)) for _ in range(3))
    X[0, 0] = 0.0
    lib.hl_zmatmul(X.ctypes.data, Y.ctypes.data, n, Z.ctypes.data)
    assert np.abs(Z - X @ Y).max() <= 1e-13 * max(np.abs(X @ Y).max(), 1e-300) * n


def test_ritz_history_stopping_rule(lib):
    """hostla::RitzHistory on Ritz values that approach 1 geometrically (not a transcription of the rule: what it must answer).  The
    first check is due three products before scikit-learn's count and can only ask for another; values that gain two digits per
    check stop once two rises are known and the second is small; values that gain 10 % per check get "no further checks" (next check
    past the limit, the factor recorded) at the first check that has two estimates, and not before."""
    def run(rate, checks):
        wv = np.ascontiguousarray((1.0 - 0.5 * rate ** np.arange(checks))[:, None])
        products = np.arange(4, 4 + 3 * checks, 3, dtype=np.int32)
        stop, nxt = np.zeros(checks, np.int32), np.zeros(checks, np.int32)
        factor = lib.hl_ritz_history(wv.ctypes.data, products.ctypes.data, checks, 1, 1, 7, 2, 20, stop.ctypes.data, nxt.ctypes.data)
        return stop.tolist(), nxt.tolist(), factor

    assert run(0.5, 1) == ([0], [7], 0.0)
    stop, nxt, factor = run(0.01, 4)
    assert stop == [0, 0, 0, 1] and nxt[:3] == [7, 10, 13] and factor == 0.0
    stop, nxt, factor = run(0.9, 3)
    assert stop == [0, 0, 0] and nxt == [7, 10, 21] and factor > 0.0
