"""Host-side checks of independent component analysis (xeofs_amd.single.ICA) that need no GPU: the constructor and every refusal,
the GPU-free helpers (the starts against a hand draw from RandomState and against the restatement, gamma, the pick and the order
with their ties), the launch plan of csrc/eofx_ica.hpp (tests/ica_shim.cpp, compiled with the host C++ compiler) against the
documented rule at the limits, and the new symbol in the header, the ctypes table and the built library."""

import inspect
import os
import re

import numpy as np
import pytest

import ica_plan as ip
import ica_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the constructor
def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, ICA

    assert xe.single.ICA is ICA and issubclass(ICA, EOF)
    names = list(inspect.signature(ICA.__init__).parameters)[1:]
    assert names == ["n_modes", "fun", "alpha", "tol", "max_iter", "n_init", "w_init", "center", "standardize", "use_coslat", "check_nans",
                     "sample_name", "feature_name", "solver", "random_state", "solver_kwargs"]
    prm = ICA().get_params()
    assert (prm["n_modes"], prm["fun"], prm["alpha"], prm["tol"], prm["max_iter"], prm["n_init"], prm["w_init"], prm["center"],
            prm["standardize"], prm["use_coslat"], prm["check_nans"], prm["random_state"]) == (2, "logcosh", 1.0, 1e-4, 200, 1, None, True,
                                                                                               False, False, True, None)
    W = np.arange(27.0).reshape(3, 3, 3)
    m = ICA(n_modes=3, fun="exp", alpha=2, tol=1e-6, max_iter=7, n_init=3, w_init=W, random_state=4, standardize=True)
    prm = m.get_params()
    assert (prm["n_modes"], prm["fun"], prm["alpha"], prm["tol"], prm["max_iter"], prm["n_init"]) == (3, "exp", 2.0, 1e-6, 7, 3)
    assert np.array_equal(prm["w_init"], W) and prm["random_state"] == 4 and m.attrs["model"] == "ICA"
    assert ICA(n_modes=32, n_init=1024).n_modes == 32
    assert ICA(n_modes=2, w_init=np.eye(2)).get_params()["w_init"].shape == (1, 2, 2)


@pytest.mark.parametrize("kw, exc, word", [
    (dict(n_modes=0), ValueError, "n_modes"), (dict(n_modes=-1), ValueError, "n_modes"), (dict(n_modes=2.5), ValueError, "n_modes"),
    (dict(n_modes=True), ValueError, "n_modes"), (dict(n_modes=33), NotImplementedError, "32"),
    (dict(fun="tanh"), ValueError, "fun"), (dict(fun=None), ValueError, "fun"),
    (dict(alpha=0.99), ValueError, "alpha"), (dict(alpha=2.01), ValueError, "alpha"), (dict(alpha="1"), ValueError, "alpha"),
    (dict(alpha=float("nan")), ValueError, "alpha"), (dict(alpha=True), ValueError, "alpha"),
    (dict(tol=0.0), ValueError, "tol"), (dict(tol=-1e-4), ValueError, "tol"), (dict(tol=1.5), ValueError, "tol"),
    (dict(tol=float("nan")), ValueError, "tol"),
    (dict(max_iter=0), ValueError, "max_iter"), (dict(max_iter=1.5), ValueError, "max_iter"),
    (dict(n_init=0), ValueError, "n_init"), (dict(n_init=1025), NotImplementedError, "1024"),
    (dict(center=False), ValueError, "center"),
    (dict(n_modes=3, w_init=np.eye(2)), ValueError, "w_init"), (dict(n_modes=2, w_init=np.zeros((2, 2, 2))), ValueError, "n_init"),
    (dict(n_modes=2, w_init=np.full((2, 2), np.nan)), ValueError, "NaN"), (dict(n_modes=2, w_init=np.zeros(4)), ValueError, "w_init"),
])
def test_the_constructor_refuses_and_names_the_argument(kw, exc, word):
    from xeofs_amd.single import ICA

    with pytest.raises(exc, match=word):
        ICA(**kw)


def test_svd_only_accessors_and_limits():
    from xeofs_amd.single import ICA, ica

    with pytest.raises(NotImplementedError, match="singular"):
        ICA().singular_values()
    assert (ica.Q_MAX, ica.N_MAX, ica.R_MAX, ica.CALL_ITERS, ica.FUNS) == (32, 4194304, 1024, 64, ("logcosh", "exp", "cube"))


# ------------------------------------------------------------------------------------------------ the helpers
@pytest.mark.parametrize("q, R, seed", [(1, 1, 0), (4, 1, 3), (6, 5, 1), (32, 3, 7)])
def test_the_starts_against_a_hand_draw(q, R, seed):
    from xeofs_amd.single.ica import ica_starts

    got = ica_starts(q, R, seed)
    rs = np.random.RandomState(seed)
    for r in range(R):
        G = rs.normal(size=(q, q))                      # (with R = 1: scikit-learn's own w_init draw)
        U, _, Vt = np.linalg.svd(G)
        c2 = np.linalg.cond(G) ** 2                     # (the eigh route squares the condition of the draw)
        assert np.abs(got[r] - U @ Vt).max() <= 8 * q * 2.0 ** -52 * c2
        assert np.abs(got[r] @ got[r].T - np.eye(q)).max() <= 8 * q * 2.0 ** -52 * c2
        assert np.abs(got[r] - kr.starts(q, R, seed)[r]).max() <= 8 * q * 2.0 ** -52 * c2
    assert got.shape == (R, q, q) and got.flags["C_CONTIGUOUS"]
    # w_init replaces the draw and is decorrelated too
    Wi = np.random.RandomState(seed + 1).normal(size=(R, q, q))
    got = ica_starts(q, R, seed, Wi)
    assert np.abs(got - np.stack([kr.polar(W) for W in Wi])).max() <= 8 * q * 2.0 ** -52 * max(np.linalg.cond(W) for W in Wi) ** 2
    with pytest.raises(np.linalg.LinAlgError):
        ica_starts(2, 1, 0, np.zeros((1, 2, 2)))


def test_pick_and_order_with_their_ties():
    from xeofs_amd.single import ica

    assert ica.best_restart([1.0, 3.0, 2.0, 3.0], [1, 1, 1, 1]) == 1 and ica.best_restart([5.0], [0]) == 0
    assert ica.best_restart([2.0, 2.0, 2.0], [1, 0, 1]) == 0
    assert ica.best_restart([9.0, 4.0, 4.0], [2, 1, 0]) == 1                  # a degenerate restart never wins
    assert ica.best_restart([np.nan, 4.0], [2, 0]) == 1                       # ... whatever its contrast
    with pytest.raises(np.linalg.LinAlgError, match="degenerate"):
        ica.best_restart([1.0, 2.0], [2, 2])
    for bad in (([], []), ([1.0, np.nan], [1, 1]), ([[1.0, 2.0]], [[1, 1]]), ([1.0, 2.0], [1])):
        with pytest.raises(ValueError):
            ica.best_restart(*bad)
    assert ica.mode_order([5.0, 9.0, 5.0, 0.0, 9.0]).tolist() == [1, 4, 0, 2, 3]
    assert ica.mode_order([0.0, 0.0, 0.0]).tolist() == [0, 1, 2] and ica.mode_order([7.0]).tolist() == [0]
    g = np.array([[0.3, 0.4], [0.75, 0.75]])
    assert np.allclose(ica.restart_contrast(g, "cube"), [(0.45 ** 2 + 0.35 ** 2), 0.0])
    assert ica.restart_contrast(g, "exp").shape == (2,)


# ------------------------------------------------------------------------------------------------ the plan
def test_the_constants_are_those_the_engine_states():
    from xeofs_amd import engine

    c = ip.constants()
    assert c == dict(ICA_QMAX=32, ICA_NMAX=4194304, ICA_RMAX=1024, ICA_ITER_MAX=64, ICA_WG=256, ICA_BMAX=512)
    assert (engine.ICA_QMAX, engine.ICA_NMAX, engine.ICA_RMAX, engine.ICA_ITER_MAX) == (32, 4194304, 1024, 64)


def test_ica_plan_against_the_documented_rule_at_the_limits():
    BMAX, NMAX = 512, 4194304
    for n in (1, 255, 256, 257, 10000, 256 * BMAX - 1, 256 * BMAX, 256 * BMAX + 1, 350000, NMAX - 1, NMAX):
        for q in (1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 31, 32):
            pl = ip.plan(n, q)
            rows = 256 * max(1, -(-n // (256 * BMAX)))
            assert pl["rows"] == rows and pl["blocks"] == -(-n // rows) and 1 <= pl["blocks"] <= BMAX
            assert pl["blocks"] * pl["rows"] >= n > (pl["blocks"] - 1) * pl["rows"]
            qp = max(4, 1 << (q - 1).bit_length())
            assert pl["qp"] == qp and pl["qw"] == max(qp, 16) and pl["slot"] == q * q + 2 * q + 1
            t = pl["qw"] // 16
            stage, red = 4 * 2 * 64 * (pl["qw"] + 1) * 4, 4 * (t * t + 2 * t) * 256 * 8
            assert pl["lds"] == q * qp * 4 + max(stage, red) and pl["lds"] <= 160 * 1024 - 64
            # the scratch, and B independent of R
            for R in (1, 2, 50, 1024):
                assert ip.scratch(n, q, R) == R * pl["blocks"] * pl["slot"]
    assert ip.plan(256 * BMAX, 4)["rows"] == 256 and ip.plan(256 * BMAX + 1, 4)["rows"] == 512 and ip.plan(NMAX, 32)["rows"] == 8192
    assert ip.plan(1, 1)["blocks"] == 1 and ip.plan(NMAX, 32)["blocks"] == BMAX


# ------------------------------------------------------------------------------------------------ the symbol
def test_engine_entry():
    from xeofs_amd import engine

    assert list(inspect.signature(engine.fastica).parameters) == ["ctx", "Z", "W", "status", "iters", "fun", "alpha", "tol", "max_iter",
                                                                  "out", "want"]
    assert engine.ICA_FUNS == ("logcosh", "exp", "cube")


def test_new_symbol_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    lib = _lib.load()
    s = "eofx_fastica_f32"
    assert s in syms and s in _lib.SIGNATURES and len(_lib.SIGNATURES[s][1]) == 17 and hasattr(lib, s)
    assert lib.eofx_abi_version() == 1
    mk = open(os.path.join(ROOT, "xeofs_amd", "csrc", "Makefile")).read()
    assert "eofx_ica.hpp" in mk
