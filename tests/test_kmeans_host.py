"""Host-side checks of weather-regime clustering (xeofs_amd.single.KMeans) that need no GPU: the constructor and every refusal,
the GPU-free helpers (k-means++ reproducing the restatement's seeds, the best restart and the mode order with their ties, the
classifiability index), the launch plan of csrc/eofx_kmeans.hpp (tests/kmeans_shim.cpp, compiled with the host C++ compiler)
against the documented rule at the limits, and the new symbol in the header, the ctypes table and the built library."""

import inspect
import os
import re

import numpy as np
import pytest

import kmeans_plan as kp
import kmeans_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the constructor
def test_exported_and_constructed_like_eof():
    import xeofs_amd as xe
    from xeofs_amd.single import EOF, KMeans

    assert xe.single.KMeans is KMeans and issubclass(KMeans, EOF)
    names = list(inspect.signature(KMeans.__init__).parameters)[1:]
    assert names == ["n_modes", "n_pca_modes", "n_init", "max_iter", "center", "standardize", "use_coslat", "check_nans", "sample_name",
                     "feature_name", "random_state", "init"]
    prm = KMeans().get_params()
    assert (prm["n_modes"], prm["n_pca_modes"], prm["n_init"], prm["max_iter"], prm["center"], prm["standardize"], prm["use_coslat"],
            prm["check_nans"], prm["random_state"], prm["init"]) == (4, 14, 50, 300, True, False, False, True, None, None)
    m = KMeans(n_modes=3, n_pca_modes=5, n_init=7, max_iter=2500, random_state=4, init=[4, 2, 9])
    prm = m.get_params()
    assert (prm["n_modes"], prm["n_pca_modes"], prm["n_init"], prm["max_iter"]) == (3, 5, 7, 2500)
    assert prm["init"].tolist() == [4, 2, 9] and prm["random_state"] == 4 and m.attrs["model"] == "KMeans weather regimes"
    assert KMeans(n_modes=32, n_pca_modes=32, n_init=4096).n_modes == 32


@pytest.mark.parametrize("kw, exc, word", [
    (dict(n_modes=0), ValueError, "n_modes"), (dict(n_modes=-1), ValueError, "n_modes"), (dict(n_modes=2.5), ValueError, "n_modes"),
    (dict(n_modes=True), ValueError, "n_modes"), (dict(n_modes=33), NotImplementedError, "32"),
    (dict(n_pca_modes=0), ValueError, "n_pca_modes"), (dict(n_pca_modes=0.9), ValueError, "n_pca_modes"),
    (dict(n_pca_modes=33), NotImplementedError, "32"),
    (dict(n_init=0), ValueError, "n_init"), (dict(n_init=4097), NotImplementedError, "4096"),
    (dict(max_iter=0), ValueError, "max_iter"), (dict(max_iter=1.5), ValueError, "max_iter"),
    (dict(n_modes=3, init=[1, 2, 2]), ValueError, "distinct"), (dict(n_modes=3, init=[1, 2]), ValueError, "init"),
    (dict(n_modes=2, init=[-1, 2]), ValueError, "init"), (dict(n_modes=2, init=[0.5, 2.0]), ValueError, "init"),
])
def test_the_constructor_refuses_and_names_the_argument(kw, exc, word):
    from xeofs_amd.single import KMeans

    with pytest.raises(exc, match=word):
        KMeans(**kw)


def test_the_refusals_that_need_the_number_of_samples():
    from xeofs_amd.single import kmeans as km

    km.check_problem(262144, 32, np.array([0, 262143]))
    km.check_problem(5, 5)
    with pytest.raises(ValueError, match="n_modes"):
        km.check_problem(4, 5)
    with pytest.raises(NotImplementedError, match="262144"):
        km.check_problem(262145, 3)
    with pytest.raises(ValueError, match="init"):
        km.check_problem(10, 2, np.array([3, 10]))
    assert (km.K_MAX, km.Q_MAX, km.N_MAX, km.R_MAX, km.LAUNCH_ITERS) == (32, 32, 262144, 4096, 1000)


def test_svd_only_accessors_say_what_to_use():
    from xeofs_amd.single import KMeans

    m = KMeans()
    for name in ("singular_values", "explained_variance", "explained_variance_ratio"):
        with pytest.raises(NotImplementedError, match="explained_variance_fraction"):
            getattr(m, name)()


# ------------------------------------------------------------------------------------------------ the helpers
@pytest.mark.parametrize("n, q, k, R, seed", [(3, 1, 3, 5, 0), (40, 7, 5, 9, 1), (300, 14, 4, 50, 2), (64, 2, 32, 3, None), (10, 3, 1, 4, 7)])
def test_kmeanspp_reproduces_the_seeds_of_the_restatement(n, q, k, R, seed):
    from xeofs_amd.single.kmeans import kmeanspp_seeds

    S = np.random.RandomState(11 * n + q).standard_normal((n, q)).astype(np.float32)
    if seed is None:                                # no seed: the global stream is not touched, the shape and the range hold
        got = kmeanspp_seeds(S, k, R, None)
    else:
        got = kmeanspp_seeds(S, k, R, seed)
        assert got.tolist() == kr.kmeanspp_seeds(S, k, R, seed).tolist()
        assert got[:, 0].tolist() != [got[0, 0]] * R or n < 4          # one stream over the restarts: not R copies of one draw
    assert got.shape == (R, k) and got.dtype == np.int64 and got.min() >= 0 and got.max() < n
    assert all(np.unique(row).size == k for row in got)                # distinct rows of a field without duplicates


def test_kmeanspp_on_duplicates_and_equal_rows():
    from xeofs_amd.single.kmeans import kmeanspp_seeds

    S = np.array([[0.0], [0.0], [5.0], [5.0], [9.0]])
    for seed in range(10):
        got = kmeanspp_seeds(S, 3, 4, seed)
        assert got.tolist() == kr.kmeanspp_seeds(S, 3, 4, seed).tolist()
        assert all(sorted(S[row, 0].tolist()) == [0.0, 5.0, 9.0] for row in got)       # a row equal to a centre has D^2 = 0
    ones = np.ones((4, 2))
    for seed in range(6):
        got = kmeanspp_seeds(ones, 3, 2, seed)
        assert got.tolist() == kr.kmeanspp_seeds(ones, 3, 2, seed).tolist() and all(np.unique(r).size == 3 for r in got)


def test_best_restart_and_mode_order_ties():
    from xeofs_amd.single import kmeans as km

    assert km.best_restart([3.0, 1.0, 2.0, 1.0]) == 1 and km.best_restart([5.0]) == 0 and km.best_restart([2.0, 2.0, 2.0]) == 0
    assert km.best_restart([np.inf, 4.0]) == 1
    for bad in ([], [1.0, np.nan], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            km.best_restart(bad)
    assert km.mode_order([5, 9, 5, 0, 9]).tolist() == [1, 4, 0, 2, 3]
    assert km.mode_order([0, 0, 0]).tolist() == [0, 1, 2] and km.mode_order([7]).tolist() == [0]


def test_classifiability_of_identical_and_permuted_partitions():
    from xeofs_amd.single.kmeans import classifiability

    rs = np.random.RandomState(3)
    P = rs.standard_normal((4, 14))
    assert classifiability(np.stack([P] * 5)) == pytest.approx(1.0, abs=1e-14)
    assert classifiability(np.stack([P, P[[3, 1, 0, 2]], P[::-1], 2.5 * P])) == pytest.approx(1.0, abs=1e-14)
    assert np.isnan(classifiability(P[None]))
    for R in (2, 3, 6):
        C = rs.standard_normal((R, 5, 3))
        C[1, 2] = 0.0
        assert classifiability(C) == pytest.approx(kr.classifiability(C), abs=1e-14)
        assert classifiability(C.astype(np.float32)) == pytest.approx(kr.classifiability(C.astype(np.float32)), abs=1e-14)
    with pytest.raises(ValueError, match="R x k x q"):
        classifiability(P)


# ------------------------------------------------------------------------------------------------ the plan
def test_the_constants_are_those_the_engine_states():
    from xeofs_amd import engine

    c = kp.constants()
    assert c == dict(KMEANS_KMAX=32, KMEANS_QMAX=32, KMEANS_NMAX=262144, KMEANS_RMAX=4096, KMEANS_ITER_MAX=1000, KMEANS_WG=256,
                     KMEANS_ACC_MAX=1024, KMEANS_RED_BYTES=64)
    assert (engine.KMEANS_KMAX, engine.KMEANS_QMAX, engine.KMEANS_NMAX, engine.KMEANS_RMAX, engine.KMEANS_ITER_MAX) == (
        c["KMEANS_KMAX"], c["KMEANS_QMAX"], c["KMEANS_NMAX"], c["KMEANS_RMAX"], c["KMEANS_ITER_MAX"])


def test_kmeans_plan_against_the_documented_rule_at_the_limits():
    worst = 0
    for n in (1, 2, 255, 256, 257, 4099, 10000, 262143, 262144):
        for q in (1, 2, 3, 4, 5, 8, 9, 14, 16, 17, 31, 32):
            for k in (1, 2, 3, 4, 16, 17, 31, 32):
                for R in (1, 50, 300, 4096):
                    pl = kp.plan(n, q, k, R)
                    qp = max(4, 1 << (q - 1).bit_length())
                    g = 64 // qp
                    while g > 1 and g * k * q > 1024:
                        g //= 2
                    acc, c_off = 64, (64 + 4 * g * k * q * 8 + 15) // 16 * 16
                    stage = c_off + k * qp * 4
                    cnt = stage + 4 * 64 * (qp + 1) * 4
                    lab = cnt + 4 * g * k * 4
                    want = dict(grid=R, threads=256, qp=qp, groups=g, rpt=-(-n // 256), acc_off=acc, c_off=c_off, stage_off=stage,
                                cnt_off=cnt, lab_off=lab, lds=lab + 256 * 4)
                    assert pl == want, (n, q, k, R, pl, want)
                    assert qp >= q and qp in (4, 8, 16, 32) and g >= 1 and g * qp <= 64 and (g * k * q <= 1024 or g == 1)
                    assert 4 * g * k * q * 8 <= 32 * 1024                   # the accumulators: 32 KiB at the limits
                    assert c_off % 16 == 0 and stage % 16 == 0 and acc % 8 == 0 and cnt % 4 == 0
                    worst = max(worst, pl["lds"])
    assert kp.plan(262144, 32, 32, 4096)["rpt"] == 1024
    assert worst == kp.plan(1, 32, 32, 1)["lds"] == 64 + 32768 + 4096 + 33792 + 512 + 1024 <= 160 * 1024 // 2     # two workgroups a CU


# ------------------------------------------------------------------------------------------------ the layers
def test_engine_entry():
    from xeofs_amd import engine

    assert list(inspect.signature(engine.kmeans_lloyd).parameters) == ["ctx", "Z", "C0", "max_iter", "out", "want_mind2"]


def test_new_symbol_in_header_and_signatures():
    from xeofs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "eofx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(eofx_[a-z0-9_]+)\s*\(", txt))
    lib = _lib.load()
    s = "eofx_kmeans_lloyd_f32"
    assert s in syms and s in _lib.SIGNATURES and len(_lib.SIGNATURES[s][1]) == 16 and hasattr(lib, s)
    assert lib.eofx_abi_version() == 1
