"""Host-side checks of empirical orthogonal teleconnections (xeofs_amd.single.EOT) that need no GPU: the constructor, the
argument checks that run before any context exists, the four GPU-free helpers against the float64 restatement of
tests/eot_reference.py, and the two new symbols in the header, the ctypes table and the built library."""

import inspect
import os
import re

import numpy as np
import pytest

import eot_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, EOT

    assert xe.single.EOT is EOT and issubclass(EOT, EOF)
    mine, eofs = (list(inspect.signature(c.__init__).parameters) for c in (EOT, EOF))
    assert [a for a in mine if a != "min_residual"] == eofs and "min_residual" in mine
    assert inspect.signature(EOT.__init__).parameters["min_residual"].default == 1e-3
    m = EOT(n_modes=3, standardize=True, use_coslat=True, random_state=7, min_residual=0.01)
    prm = m.get_params()
    assert prm["n_modes"] == 3 and prm["standardize"] is True and prm["use_coslat"] is True and prm["random_state"] == 7
    assert prm["min_residual"] == 0.01 and prm["solver_kwargs"] == {}
    assert EOT().get_params()["min_residual"] == 1e-3
    assert m.attrs["model"] == "Empirical orthogonal teleconnections"
    assert m.ctx is None                                       # nothing touched a device
    assert not m.preprocessor.masked_ok                        # a land mask is compacted, not kept as zero columns


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 2.0, float("nan"), "0.1", None])
def test_min_residual_must_lie_in_the_open_unit_interval(bad):
    from xeofs_amd.single import EOT

    with pytest.raises(ValueError, match="min_residual"):
        EOT(min_residual=bad)


def test_argument_checks_without_a_context():
    import xeofs_amd as xe
    from xeofs_amd import engine
    from xeofs_amd.single import EOT, eot

    m = EOT(n_modes=2)
    X = np.zeros((6, 4), dtype=np.complex64)
    with pytest.raises(TypeError, match="complex"):
        m.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(6), "x": np.arange(4)}), dim="time")
    assert m.ctx is None                                       # refused before a context is bound
    with pytest.raises(ValueError, match="n_modes"):
        EOT(n_modes=0.5)
    assert eot.MAX_SAMPLES == engine.COLQUAD_NMAX == 16384

    class TooLong:                                             # the limit is checked before anything touches the matrix
        shape = (engine.COLQUAD_NMAX + 1, 8)

    with pytest.raises(ValueError, match="at most 16384 samples, got n_samples = 16385"):
        m._fit_algorithm(TooLong())
    assert m.ctx is None


def test_eot_scores_against_the_restatement():
    from xeofs_amd.single.eot import eot_scores

    X = er.designed_field()
    ref = er.gram_form(X, 3)
    c = np.sum(X * X, axis=0)
    for k in range(3):
        den = ref["den"][k]
        num = ref["all_scores"][k] * den
        got = eot_scores(num, den, c, er.MIN_RESIDUAL)
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, ref["all_scores"][k], rtol=1e-13)
        assert int(np.argmax(got)) == ref["base"][k]
    # the guard: den at or below min_residual c, or c = 0, scores 0 whatever num holds; the lowest index wins a tie
    got = eot_scores([5.0, 5.0, 7.0, 1.0, np.inf], [1.0, 1.0, 1e-3, 0.0, 0.0], [2.0, 2.0, 1.0, 0.0, 1.0], 1e-3)
    np.testing.assert_array_equal(got, [5.0, 5.0, 0.0, 0.0, 0.0])
    assert int(np.argmax(got)) == 0


def test_next_series_and_deflate_against_the_restatement():
    from xeofs_amd.single.eot import deflate, next_series

    X = er.designed_field()
    n = X.shape[0]
    ref = er.gram_form(X, 3)
    G = X @ X.T
    A, T = G.copy(), np.zeros((n, 0))
    for k in range(3):
        r = next_series(T, X[:, ref["base"][k]].astype(np.float32).astype(np.float64))
        assert r.dtype == np.float64 and r.shape == (n,)
        np.testing.assert_allclose(r, ref["series"][:, k], atol=1e-6 * np.abs(ref["series"]).max())     # (float32 input)
        r = next_series(T, X[:, ref["base"][k]])
        np.testing.assert_allclose(r, ref["series"][:, k], atol=1e-13 * np.abs(ref["series"]).max())
        assert np.abs(T.T @ r).max(initial=0.0) <= 1e-14 * np.sqrt(r @ r)
        t = r / np.sqrt(r @ r)
        A = deflate(A, t)
        T = np.concatenate([T, t[:, None]], axis=1)
        P = np.eye(n) - T @ T.T
        np.testing.assert_allclose(A, P @ G @ P, atol=1e-12 * np.abs(G).max())
    # a non-symmetric matrix, and the torch flavour
    rng = np.random.default_rng(0)
    M = rng.standard_normal((n, n))
    t = T[:, 0]
    P = np.eye(n) - np.outer(t, t)
    np.testing.assert_allclose(deflate(M, t), P @ M @ P, atol=1e-13 * np.abs(M).max())
    import torch

    got = deflate(torch.from_numpy(M), torch.from_numpy(t))
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), P @ M @ P, atol=1e-13 * np.abs(M).max())


def test_transform_series_against_the_restatement():
    from xeofs_amd.single.eot import transform_series

    X = er.designed_field()
    ref = er.textbook(X, 3)
    b, B = ref["base"], ref["patterns"]
    got = transform_series(X[:, b], B[b, :])
    np.testing.assert_allclose(got, ref["series"], atol=1e-13 * np.abs(ref["series"]).max())
    Xn = np.random.default_rng(9).standard_normal((7, 36))
    np.testing.assert_allclose(transform_series(Xn[:, b], B[b, :]), er.transform(Xn[:, b], B, b), atol=1e-13)
    # only the strict lower triangle is read
    Mu = B[b, :] + np.triu(np.full((3, 3), 1e6))
    np.testing.assert_array_equal(transform_series(Xn[:, b], Mu), transform_series(Xn[:, b], B[b, :]))


def test_engine_entries_and_limit():
    from xeofs_amd import engine

    assert engine.COLQUAD_NMAX == 16384
    assert callable(engine.colquad) and callable(engine.mat_colquad)
    assert list(inspect.signature(engine.colquad).parameters) == ["ctx", "T", "A", "out"]
    assert list(inspect.signature(engine.mat_colquad).parameters) == ["ctx", "mat", "A", "out"]


def test_new_symbols_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    for s in ("eofx_colquad_f32", "eofx_mat_colquad_f32"):
        assert s in syms and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["eofx_colquad_f32"][1]) == 8
    assert len(_lib.SIGNATURES["eofx_mat_colquad_f32"][1]) == 5
    lib = _lib.load()
    assert hasattr(lib, "eofx_colquad_f32") and hasattr(lib, "eofx_mat_colquad_f32")
    assert lib.eofx_abi_version() == 1
