"""tests/orth_reference.py (the extended-precision reference and the designed inputs of tests/test_gpu_orth_chain.py) checked
without a GPU: the reference against numpy.linalg on well-conditioned Gram matrices, the designed near-dependent columns
through hostla::chol_rinv_padded (tests/hostla_shim.cpp, built as in test_hostla_cpu.py) -- the host twin of the device
rule "pivot <= 1e-13 x original diagonal" --, and the zero fill of the whole L x L output for l <= 64 < L, the behaviour the
device route has to match.

Tolerances: numpy's float64 Cholesky + inverse against the reference, in the row-scaled metric of
orth_reference.scaled_error, within the first-order bound 4 l 2^-53 kappa_2 (unit-diagonal scaling; measured 1.1e-16 ..
2.8e-16 for l = 1 .. 320); the float64 product against the reference within its own bound L 2^-53 |P| |M|.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import orth_reference as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
TOL = 1e-13


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("orthref")
    so = str(d / "hostla_shim.so")
    cmd = [CXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "xeofs_amd", "csrc"),
           os.path.join(ROOT, "tests", "hostla_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    lib.hl_chol_rinv_padded.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double]
    lib.hl_chol_rinv_padded.restype = None
    return lib


def _host_rinv(lib, G, L, fill=np.nan):
    l = G.shape[0]
    Gp = np.ascontiguousarray(oref.embed(G, L, fill=np.nan))       # (outside the block: never read)
    R = np.full((L, L), fill)
    lib.hl_chol_rinv_padded(Gp.ctypes.data, L, l, R.ctypes.data, TOL)
    return R


def _dead_of(R, l):
    return [j for j in range(l) if R[j, j] == 0.0]


@pytest.mark.parametrize("l", [1, 2, 9, 17, 33, 64, 129, 320])
def test_reference_against_numpy(l):
    """well-conditioned designed Gram matrices: upper triangular, R^-T R^-1 = G^-1 through numpy, and numpy's own factor within
    the first-order bound of the reference"""
    G, D = oref.design_gram(l, seed=l)
    kappa = oref.unit_diagonal_cond(G)
    assert kappa <= 10.0, kappa
    X = oref.chol_rinv_ref(G, l)
    Xh = oref.to_f64(X)
    assert not np.tril(Xh, -1).any() and (np.diag(Xh) > 0).all()
    E = oref.scaled_error(oref.numpy_rinv(G), X, G)
    print(f"l={l} kappa={kappa:.2f} E_numpy={E:.3e}")
    assert E <= 4 * l * 2.0 ** -53 * kappa
    # X^T G X = I: the residual of the rounded reference is float64 rounding of a matrix with |entries| <= 1
    S = Xh.T @ G @ Xh
    assert np.abs(S - np.eye(l)).max() <= 8 * l * 2.0 ** -53 * kappa


def test_reference_drops_dead_indices():
    """dead indices come back as zero rows and columns; the rest is the factor of the matrix without them"""
    l, L, dead = 17, 32, [0, 7, 16]
    G, _ = oref.design_gram(l, seed=3)
    X = oref.to_f64(oref.chol_rinv_ref(oref.embed(G, L), l, dead))
    keep = np.setdiff1d(np.arange(l), dead)
    assert not X[dead].any() and not X[:, dead].any() and not X[l:].any() and not X[:, l:].any()
    Xk = oref.to_f64(oref.chol_rinv_ref(G[np.ix_(keep, keep)], keep.size))
    assert np.array_equal(X[np.ix_(keep, keep)], Xk)
    assert oref.scaled_error(oref.numpy_rinv(G[np.ix_(keep, keep)]), Xk, G[np.ix_(keep, keep)]) <= 4 * l * 2.0 ** -53 * 10


def test_matmul_reference():
    rng = np.random.default_rng(0)
    P = (rng.standard_normal((37, 96)) * 10.0 ** rng.uniform(-3, 3, 96)).astype(np.float32)
    M = rng.standard_normal((96, 33))
    ref = oref.matmul_ref(P, M)
    got = P.astype(np.float64) @ M
    bound = 96 * 2.0 ** -53 * (np.abs(P.astype(np.float64)) @ np.abs(M))
    assert (np.abs(oref.to_f64(ref - got)) <= bound).all()
    one = oref.matmul_ref(np.float32([[3.0]]), np.float64([[1.0 / 3.0]]))     # the products keep more than 53 bits
    assert one[0, 0] != 1 and oref.to_f64(one)[0, 0] == 1.0


@pytest.mark.parametrize("l,j", [(l, j) for l in (9, 17, 33, 64) for j in sorted({2, 7, 8, 15, 16, l - 1}) if j < l])
def test_designed_distance_from_dependence(lib, l, j):
    """column j at rho = 1e-15 is dependent for the host rule and at rho = 1e-11 it is not; no other column is affected; the
    live block is the reference's within the first-order bound"""
    L = (l + 31) // 32 * 32
    G, _ = oref.design_gram(l, seed=l, near={j: 1e-15})
    R = _host_rinv(lib, G, L)
    assert _dead_of(R, l) == [j]
    assert not R[j].any() and not R[:, j].any() and not np.tril(R, -1).any() and np.isfinite(R).all()
    keep = np.setdiff1d(np.arange(l), [j])
    Xref = oref.chol_rinv_ref(oref.embed(G, L), l, [j])
    Gk = G[np.ix_(keep, keep)]
    assert oref.scaled_error(R[:l, :l], Xref[:l, :l], G) <= 4 * l * 2.0 ** -53 * oref.unit_diagonal_cond(Gk)
    G, _ = oref.design_gram(l, seed=l, near={j: 1e-11})
    R = _host_rinv(lib, G, L)
    assert _dead_of(R, l) == [] and np.isfinite(R).all()


DESIGNED = [(c, l, kw, dead or []) for c, l, kw, dead in oref.DEAD_ONE_WG] + \
           [(c, l, kw, dead or []) for c, l, _, kw, dead in oref.BLOCKED if kw]


@pytest.mark.parametrize("case,l,kw,dead", DESIGNED, ids=[c[0] for c in DESIGNED])
def test_designed_cases_of_the_device_tests(lib, case, l, kw, dead):
    L = (l + 31) // 32 * 32
    G, _ = oref.design_gram(l, seed=l, **kw)
    R = _host_rinv(lib, G, L)
    assert _dead_of(R, l) == dead, case
    assert not R[dead].any() and not R[:, dead].any()


@pytest.mark.parametrize("l,L", [(9, 96), (9, 128), (64, 96), (64, 128), (1, 96)])
def test_host_route_zero_fills_the_whole_output(lib, l, L):
    """hostla::chol_rinv_padded writes all L x L entries for l <= 64 < L (the output arrives full of NaN): zero outside l x l"""
    G, _ = oref.design_gram(l, seed=l)
    R = _host_rinv(lib, G, L, fill=np.nan)
    assert np.isfinite(R).all()
    assert not R[l:].any() and not R[:, l:].any() and not np.tril(R, -1).any()
    assert oref.scaled_error(R, oref.chol_rinv_ref(oref.embed(G, L), l), oref.embed(G, L, fill=1.0)) <= 4 * l * 2.0 ** -53 * 10
