"""Host-side checks of archetypal analysis (xeofs_amd.single.ArchetypalAnalysis) that need no GPU: the constructor and every
refusal, the GPU-free helpers (the FurthestSum start and its ties, the mode order, the float32 step that never exceeds its
float64 value, the objective), the launch plan of csrc/eofx_simplex.hpp (tests/simplex_shim.cpp, compiled with the host C++
compiler) against the documented rule, and the two new symbols in the header, the ctypes table and the built library."""

import inspect
import os
import re

import numpy as np
import pytest

import aa_reference as ar
import simplex_plan as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the constructor
def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, ArchetypalAnalysis

    assert xe.single.ArchetypalAnalysis is ArchetypalAnalysis and issubclass(ArchetypalAnalysis, EOF)
    names = list(inspect.signature(ArchetypalAnalysis.__init__).parameters)[1:]
    assert names == ["n_modes", "center", "standardize", "use_coslat", "check_nans", "sample_name", "feature_name", "random_state",
                     "max_iter", "tol", "inner_iter", "init_iter", "init"]
    m = ArchetypalAnalysis(n_modes=3, random_state=4, init=[4, 2, 9])
    prm = m.get_params()
    assert (prm["n_modes"], prm["max_iter"], prm["tol"], prm["inner_iter"], prm["init_iter"]) == (3, 500, 1e-6, 10, 50)
    assert prm["init"].tolist() == [4, 2, 9] and prm["random_state"] == 4
    assert m.attrs["model"] == "Archetypal analysis"
    assert ArchetypalAnalysis(n_modes=32).n_modes == 32 and ArchetypalAnalysis(tol=0).get_params()["tol"] == 0.0


@pytest.mark.parametrize("kw, exc, word", [
    (dict(n_modes=0), ValueError, "n_modes"), (dict(n_modes=-1), ValueError, "n_modes"), (dict(n_modes=2.5), ValueError, "n_modes"),
    (dict(n_modes=33), NotImplementedError, "32"),
    (dict(tol=-1e-9), ValueError, "tol"), (dict(tol=float("nan")), ValueError, "tol"),
    (dict(max_iter=0), ValueError, "max_iter"), (dict(inner_iter=0), ValueError, "inner_iter"), (dict(init_iter=-3), ValueError, "init_iter"),
    (dict(n_modes=3, init=[1, 2, 2]), ValueError, "distinct"), (dict(n_modes=3, init=[1, 2]), ValueError, "init"),
    (dict(n_modes=2, init=[-1, 2]), ValueError, "init"), (dict(n_modes=2, init=[0.5, 2.0]), ValueError, "init"),
])
def test_the_constructor_refuses_and_names_the_argument(kw, exc, word):
    from xeofs_amd.single import ArchetypalAnalysis

    with pytest.raises(exc, match=word):
        ArchetypalAnalysis(**kw)


def test_the_refusals_that_need_the_number_of_samples():
    from xeofs_amd.single import archetypal as aa

    aa.check_problem(16384, 32, np.array([0, 16383]))
    aa.check_problem(5, 5)
    with pytest.raises(ValueError, match="n_modes"):
        aa.check_problem(4, 5)
    with pytest.raises(NotImplementedError, match="16384"):
        aa.check_problem(16385, 3)
    with pytest.raises(ValueError, match="init"):
        aa.check_problem(10, 2, np.array([3, 10]))
    assert (aa.N_MAX, aa.K_MAX, aa.MAX_REJECTIONS) == (16384, 32, 40)


def test_svd_only_accessors_say_what_to_use():
    from xeofs_amd.single import ArchetypalAnalysis

    m = ArchetypalAnalysis()
    for name in ("singular_values", "explained_variance", "explained_variance_ratio"):
        with pytest.raises(NotImplementedError, match="explained_variance_fraction"):
            getattr(m, name)()


# ------------------------------------------------------------------------------------------------ the helpers
def _gram_of_points(P):
    P = np.asarray(P, dtype=np.float64)
    return P @ P.T


def test_furthest_sum_on_a_designed_set_and_its_ties():
    from xeofs_amd.single.archetypal import furthest_sum

    # a square with a point in the middle, listed twice: every tie goes to the lower index
    pts = [(0, 0), (1, 1), (-1, 1), (-1, -1), (1, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]
    K = _gram_of_points(pts)
    got = furthest_sum(K, 4, 0)
    assert sorted(got.tolist()) == [1, 2, 3, 4]                # the four corners, the first copy of each
    assert got.tolist() == ar.furthest_sum(K, 4, 0).tolist()
    assert furthest_sum(K, 1, 6).tolist() == [6]               # k = 1: the start itself
    # equal points everywhere: all distances 0, the lowest free index every time (0 and 1 beside the start 4; the sweep
    # then frees 4 and takes 2 in its place, and puts 0 and 1 back where they were)
    assert furthest_sum(np.ones((6, 6)), 3, 4).tolist() == [2, 0, 1] == ar.furthest_sum(np.ones((6, 6)), 3, 4).tolist()
    # the two ends of a line from any start
    x = np.linspace(-1.0, 2.0, 11)[:, None]
    for s in range(11):
        assert sorted(furthest_sum(_gram_of_points(x), 2, s).tolist()) == [0, 10]


@pytest.mark.parametrize("seed", range(4))
def test_furthest_sum_against_the_restatement_and_reads_picked_rows_only(seed):
    from xeofs_amd.single.archetypal import furthest_sum

    rs = np.random.RandomState(seed)
    X = rs.standard_normal((40, 7))
    K = X @ X.T
    for k in (1, 2, 5, 40):
        start = int(rs.randint(40))
        got = furthest_sum(K.astype(np.float32), k, start)
        assert got.tolist() == ar.furthest_sum(K.astype(np.float32), k, start).tolist() and np.unique(got).size == k

    class Rows:                                                # a "device tensor" that counts the rows it hands out
        def __init__(self, K):
            self.K, self.rows = K, []

        def data_ptr(self):
            return 0

        def diagonal(self):
            return self

        def detach(self):
            return self

        def cpu(self):
            return self

        def numpy(self):
            return self._v

        def __getitem__(self, i):
            self.rows.append(int(i))
            out = Rows(self.K)
            out._v = self.K[i]
            return out

    R = Rows(K)
    R._v = np.diagonal(K)
    got = furthest_sum(R, 5, 3)
    assert got.tolist() == ar.furthest_sum(K, 5, 3).tolist() and len(R.rows) == 2 * 5 and set(got.tolist()) <= set(R.rows)


def test_mode_order_objective_and_step_down():
    from xeofs_amd.single import archetypal as aa

    A = np.array([[0.2, 0.5, 0.3, 0.0], [0.2, 0.1, 0.7, 0.0], [0.6, 0.4, 0.0, 0.0]])
    assert aa.mode_order(A).tolist() == [0, 1, 2, 3]           # sums 1, 1, 1, 0: the lowest index among equals
    assert aa.mode_order(A[:, ::-1]).tolist() == [1, 2, 3, 0]
    rs = np.random.RandomState(0)
    X = rs.standard_normal((12, 9))
    Aw, Bw = rs.dirichlet(np.ones(3), 12), rs.dirichlet(np.ones(12), 3)
    K = X @ X.T
    Q = K @ Bw.T
    f = aa.objective(np.trace(K), Aw, Q, Aw.T @ Aw, Bw @ Q)
    assert abs(f - ar.objective_direct(X, Aw, Bw)) <= 1e-12 * np.trace(K)
    for x in (1.0 / 3.0, 0.1, 1e-12, 7.0, 1.0, 2.0 ** -30):
        y = aa.step_down(x)
        assert y.dtype == np.float32 and float(y) <= x and float(np.nextafter(y, np.float32(np.inf))) > x


# ------------------------------------------------------------------------------------------------ the plan
def test_the_constants_are_those_the_engine_states():
    from xeofs_amd import engine

    c = sp.constants()
    assert c == dict(SIMPLEX_MMAX=16384, SIMPLEX_KMAX=32, SIMPLEX_REG_MMAX=1024, SIMPLEX_WG=256, SIMPLEX_PG_WG=64)
    assert (engine.SIMPLEX_MMAX, engine.SIMPLEX_KMAX) == (c["SIMPLEX_MMAX"], c["SIMPLEX_KMAX"])
    assert sp.tier_boundary() == c["SIMPLEX_REG_MMAX"]


def test_simplex_plan_against_the_documented_rule():
    def pow2(x):
        return 1 << max(0, int(x - 1).bit_length())

    for m in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384):
        for r in (1, 2, 63, 64, 65, 300, 10 ** 6):
            pl = sp.plan(r, m)
            if m <= 1024:
                lanes = min(64, pow2(m))
                epl = pow2(-(-m // lanes))
                want = dict(tier=0, lanes=lanes, epl=epl, threads=256, rpb=256 // lanes, grid=-(-r // (256 // lanes)), lds=0)
                assert lanes * epl >= m and (lanes * epl < 2 * m or m == 1) and epl <= 16
            else:
                th = 256 if m <= 4096 else 1024
                want = dict(tier=1, lanes=th, epl=-(-m // th), threads=th, rpb=1, grid=r, lds=4 * m)
                assert want["lds"] <= 64 * 1024
            assert pl == want, (r, m, pl, want)
    lib = sp.shim()
    assert [lib.sx_pg_width(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 32]


# ------------------------------------------------------------------------------------------------ the layers
def test_engine_entries():
    from xeofs_amd import engine

    assert list(inspect.signature(engine.simplex_rows).parameters) == ["ctx", "V", "G", "step", "out"]
    assert list(inspect.signature(engine.simplex_pg).parameters) == ["ctx", "A", "Q", "M", "inv_L", "iters", "out"]


def test_new_symbols_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    want = {"eofx_simplex_rows_f32": 10, "eofx_simplex_pg_f32": 12}
    lib = _lib.load()
    for s, nargs in want.items():
        assert s in syms and s in _lib.SIGNATURES and len(_lib.SIGNATURES[s][1]) == nargs and hasattr(lib, s)
    assert lib.eofx_abi_version() == 1
