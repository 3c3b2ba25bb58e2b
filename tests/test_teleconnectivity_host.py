"""Host-side checks of the teleconnectivity model (xeofs_amd.single.Teleconnectivity) that need no GPU: the constructor, the
argument checks that run before any context exists, the GPU-free helpers on hand-made rmin / partner / correlation maps and
against the float64 restatement of tests/teleconnectivity_reference.py, and the two new symbols in the header, the ctypes
table and the built library."""

import inspect
import os
import re

import numpy as np
import pytest

import teleconnectivity_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, Teleconnectivity

    assert xe.single.Teleconnectivity is Teleconnectivity and issubclass(Teleconnectivity, EOF)
    mine, eofs = (list(inspect.signature(c.__init__).parameters) for c in (Teleconnectivity, EOF))
    assert [a for a in mine if a != "max_corr"] == eofs and "max_corr" in mine
    assert inspect.signature(Teleconnectivity.__init__).parameters["max_corr"].default == 0.5
    m = Teleconnectivity(n_modes=3, standardize=True, use_coslat=True, random_state=7, max_corr=0.25)
    prm = m.get_params()
    assert prm["n_modes"] == 3 and prm["standardize"] is True and prm["use_coslat"] is True and prm["random_state"] == 7
    assert prm["max_corr"] == 0.25 and prm["solver_kwargs"] == {}
    assert Teleconnectivity().get_params()["max_corr"] == 0.5 and Teleconnectivity().get_params()["n_modes"] == 2
    assert m.attrs["model"] == "Teleconnectivity" and m.attrs["max_corr"] == 0.25
    assert m.ctx is None                                       # nothing touched a device
    assert not m.preprocessor.masked_ok                        # a land mask is compacted, not kept as zero columns


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 2.0, float("nan"), "0.1", None])
def test_max_corr_must_lie_in_the_open_unit_interval(bad):
    from xeofs_amd.single import Teleconnectivity

    with pytest.raises(ValueError, match="max_corr"):
        Teleconnectivity(max_corr=bad)


@pytest.mark.parametrize("bad", [0, -1, 0.5, 2.0, "2", None])
def test_n_modes_must_be_a_positive_integer(bad):
    from xeofs_amd.single import Teleconnectivity

    with pytest.raises(ValueError, match="n_modes"):
        Teleconnectivity(n_modes=bad)


def test_argument_checks_without_a_context():
    import xeofs_amd as xe
    from xeofs_amd.single import Teleconnectivity

    m = Teleconnectivity(n_modes=2)
    X = np.zeros((6, 4), dtype=np.complex64)
    with pytest.raises(TypeError, match="complex"):
        m.fit(xe.DataArray(X, ("time", "x"), {"time": np.arange(6), "x": np.arange(4)}), dim="time")
    assert m.ctx is None                                       # refused before a context is bound
    with pytest.raises(NotImplementedError, match="not an expansion"):
        m.inverse_transform(None)


def test_scale_vector():
    from xeofs_amd.single.teleconnectivity import scale_vector

    c = np.array([4.0, 0.0, 1e-30, 3.0, -1.0, np.nan, 1e30])
    w = scale_vector(c)
    assert w.dtype == np.float32 and w.shape == c.shape
    np.testing.assert_array_equal(w[[1, 4, 5]], 0.0)           # c > 0 fails: excluded, never a NaN or an infinity
    ok = [0, 2, 3, 6]
    np.testing.assert_array_equal(w[ok], (1.0 / np.sqrt(c[ok])).astype(np.float32))        # float64, rounded ONCE
    assert w[0] == 0.5 and np.all(np.isfinite(w))


def test_candidate_order():
    from xeofs_amd.single.teleconnectivity import candidate_order

    rmin = np.array([-0.5, np.nan, -0.9, 0.1, -0.5, -0.9, 0.0, -0.0, -1e-30], dtype=np.float32)
    got = candidate_order(rmin)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, [2, 5, 0, 4, 8])        # ascending, the lowest index among equals; 0, NaN, > 0 are out
    assert candidate_order(np.array([np.nan, 0.5])).size == 0


def hand_made():
    """six points: (0, 3) the strongest seesaw, 1 a neighbour of 0, (2, 5) the next one, 4 on its own"""
    R = np.eye(6)

    def put(i, j, v):
        R[i, j] = R[j, i] = v

    put(0, 3, -0.9), put(0, 1, 0.8), put(1, 3, -0.7), put(2, 5, -0.6), put(4, 5, -0.2), put(2, 4, 0.1), put(1, 2, 0.3)
    return R


def test_select_pairs_on_hand_made_maps():
    from xeofs_amd.single.teleconnectivity import select_pairs

    R = hand_made()
    rmin, partner = tr.row_minima(R)
    np.testing.assert_array_equal(partner, [3, 3, 5, 0, 5, 2])
    # equal minima of 0 and 3: the lowest index is the base, its partner the other pole; 1 is blocked by its 0.8 with pole 0
    assert select_pairs(rmin, partner, 2, 0.5, R) == [(0, 3), (2, 5)]
    calls = []

    def maps(k, b, a):
        calls.append((k, b, a))
        return R[:, b], R[:, a]

    assert select_pairs(rmin, partner, 2, 0.5, maps) == [(0, 3), (2, 5)] and calls == [(0, 0, 3), (1, 2, 5)]
    # with max_corr above 0.8 point 1 is still open, but its partner 3 is a pole: skipped; 4's partner 5 likewise
    assert select_pairs(rmin, partner, 2, 0.85, R) == [(0, 3), (2, 5)]
    with pytest.raises(ValueError, match="exhausted after 2 modes"):
        select_pairs(rmin, partner, 3, 0.85, R)
    # a tight separation: 2 and 5 have correlation 0 with the poles 0 and 3, so they stay open
    assert select_pairs(rmin, partner, 2, 0.05, R) == [(0, 3), (2, 5)]
    R2 = R.copy()
    R2[2, 0] = R2[0, 2] = R2[5, 3] = R2[3, 5] = 0.06           # now 2 and 5 are blocked, and 4's partner is 5
    with pytest.raises(ValueError, match="exhausted after 1 modes.*max_corr = 0.05"):
        select_pairs(rmin, partner, 2, 0.05, R2)
    # nothing negative at all; NaN rows and -1 partners are never candidates
    with pytest.raises(ValueError, match="exhausted after 0 modes"):
        select_pairs(np.array([0.2, np.nan, 0.0]), np.array([1, -1, 0]), 1, 0.5, np.eye(3))
    # a NaN in a correlation map blocks nothing
    Rn = R.copy()
    Rn[4, :] = np.nan
    assert select_pairs(rmin, partner, 2, 0.5, Rn) == [(0, 3), (2, 5)]


def test_select_pairs_against_the_restatement():
    from xeofs_amd.single.teleconnectivity import select_pairs

    rng = np.random.default_rng(12)
    X = rng.standard_normal((30, 5)) @ rng.standard_normal((5, 40)) + 2.0 * rng.standard_normal((30, 40))
    X -= X.mean(axis=0)
    ref = tr.model(X, 3, 0.6)
    assert select_pairs(ref["rmin"], ref["partner"], 3, 0.6, tr.correlation(X)) == ref["pairs"]
    Xd = tr.designed_field()
    Xd -= Xd.mean(axis=0)
    rd = tr.model(Xd, 3)
    assert select_pairs(rd["rmin"], rd["partner"], 3, 0.5, tr.correlation(Xd)) == rd["pairs"]


def test_half_differences():
    from xeofs_amd.single.teleconnectivity import half_differences

    rng = np.random.default_rng(3)
    X = rng.standard_normal((25, 12))
    X -= X.mean(axis=0)
    ref = tr.model(X, 2, 0.9)
    idx = np.asarray(ref["pairs"]).reshape(-1)
    scale = np.sqrt(24.0) / np.sqrt(np.sum(X[:, idx] ** 2, axis=0))
    np.testing.assert_allclose(half_differences(X[:, idx], scale), ref["scores"], atol=1e-13)
    B = np.arange(8.0).reshape(2, 4)
    np.testing.assert_array_equal(half_differences(B, [2.0, 1.0, 1.0, 4.0]), [[-0.5, -5.0], [1.5, -11.0]])


def test_engine_entries():
    from xeofs_amd import engine

    assert callable(engine.pairmin) and callable(engine.mat_pairmin)
    assert list(inspect.signature(engine.pairmin).parameters) == ["ctx", "T", "w", "out"]
    assert list(inspect.signature(engine.mat_pairmin).parameters) == ["ctx", "mat", "w", "out"]


def test_new_symbols_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    for s in ("eofx_pairmin_f32", "eofx_mat_pairmin_f32"):
        assert s in syms and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["eofx_pairmin_f32"][1]) == 8
    assert len(_lib.SIGNATURES["eofx_mat_pairmin_f32"][1]) == 5
    lib = _lib.load()
    assert hasattr(lib, "eofx_pairmin_f32") and hasattr(lib, "eofx_mat_pairmin_f32")
    assert lib.eofx_abi_version() == 1
