"""The float64 restatement of weather-regime clustering (tests/kmeans_reference.py) against what does not depend on it: a
brute-force argmin of pairwise distances, the identities of Lloyd's iteration (the inertia never rises; a converged state is
a fixed point in which every centroid is the mean of its members), k-means++ by hand on three points, the classifiability
index on designed partitions -- and, for every case of the GPU operator test, the share of undecided rows the reference alone
meets on its own trajectory.  No GPU."""

import numpy as np
import pytest

import kmeans_reference as kr


def _cdist2(Z, C):
    Z, C = np.asarray(Z, np.float64), np.asarray(C, np.float64)
    return np.array([[np.dot(z - c, z - c) for c in C] for z in Z])


@pytest.mark.parametrize("n, q, k, seed", [(1, 1, 1, 0), (7, 3, 2, 1), (50, 5, 7, 2), (33, 1, 4, 3), (40, 32, 32, 4)])
def test_assign_against_brute_force(n, q, k, seed):
    rs = np.random.RandomState(seed)
    Z, C = rs.standard_normal((n, q)), rs.standard_normal((k, q))
    labels, mind2, margin = kr.assign(Z, C)
    D = _cdist2(Z, C)
    assert labels.tolist() == np.argmin(D, axis=1).tolist()
    np.testing.assert_allclose(mind2, D.min(axis=1), rtol=1e-14, atol=0)
    if k > 1:
        Ds = np.sort(D, axis=1)
        np.testing.assert_allclose(margin, (Ds[:, 1] - Ds[:, 0]) / Ds[:, 1], rtol=1e-12, atol=1e-15)
    else:
        assert (margin == 1.0).all()


def test_assign_ties_and_rows_that_are_not_finite():
    Z = np.array([[0.0, 0.0], [1.0, 1.0], [np.nan, 0.0], [np.inf, 0.0], [2.0, 0.0]])
    C = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])           # 0 and 2 are the same point
    labels, mind2, margin = kr.assign(Z, C)
    assert labels.tolist() == [0, 0, -1, -1, 0]                   # equal distances: the lowest index
    assert margin[0] == 0.0 and margin[1] == 0.0 and margin[4] == 0.0 and margin[2] == 1.0
    assert np.isnan(mind2[2]) and np.isnan(mind2[3]) and mind2[4] == 1.0
    C1, counts = kr.update(Z, labels, C)
    assert counts.tolist() == [3, 0, 0] and C1[0].tolist() == [1.0, 1.0 / 3.0]
    assert C1[1].tolist() == [0.0, 1.0] and C1[2].tolist() == [1.0, 0.0]      # empty clusters keep their centroids


@pytest.mark.parametrize("seed", range(4))
def test_the_inertia_never_rises_and_a_converged_state_is_a_fixed_point(seed):
    rs = np.random.RandomState(seed)
    n, q, k = 300, 4, 5
    Z = rs.standard_normal((n, q)) + 3.0 * rs.standard_normal((k, q))[rs.randint(k, size=n)]
    C0 = Z[rs.choice(n, k, replace=False)]
    out = kr.lloyd(Z, C0, 200)
    assert out["converged"] == 1 and 1 <= out["iters"] < 200
    ins = np.array(out["inertias"])
    assert (np.diff(ins) <= 1e-12 * ins[0]).all() and len(ins) == out["iters"] + 1
    for c in range(k):
        if out["counts"][c]:
            np.testing.assert_allclose(out["C"][c], Z[out["labels"] == c].mean(axis=0), rtol=1e-13, atol=1e-13)
    again = kr.lloyd(Z, out["C"], 5)
    assert again["iters"] == 1 and again["converged"] == 1 and np.array_equal(again["labels"], out["labels"])
    np.testing.assert_allclose(again["C"], out["C"], rtol=1e-14, atol=1e-14)
    # the stopping rule: max_iter = 0 is the assignment alone; a chain of one-step calls ends where one call ends
    zero = kr.lloyd(Z, C0, 0)
    assert zero["iters"] == 0 and zero["converged"] == 0 and np.array_equal(zero["C"], C0)
    C = C0
    for _ in range(out["iters"]):
        st = kr.step(Z, C)
        C = st["C"]
    np.testing.assert_allclose(C, out["C"], rtol=1e-13, atol=1e-13)
    assert st["converged"] == 1 and np.array_equal(st["labels"], out["labels"]) and st["inertia"] == pytest.approx(out["inertia"], rel=1e-13)


def test_kmeanspp_by_hand_on_three_points():
    S = np.array([[0.0], [1.0], [3.0]])
    # from the first centre f: D^2 and the thresholds of u for the second centre
    second = {0: lambda u: 1 if u < 1.0 / 10.0 else 2,          # D^2 = (0, 1, 9)
              1: lambda u: 0 if u < 1.0 / 5.0 else 2,           # D^2 = (1, 0, 4)
              2: lambda u: 0 if u < 9.0 / 13.0 else 1}          # D^2 = (9, 4, 0)
    seen = set()
    for seed in range(40):
        rs = np.random.RandomState(seed)
        want = []
        for _ in range(3):                                      # three restarts from one stream
            f = int(rs.randint(3))
            s = second[f](rs.random_sample())
            t = ({0, 1, 2} - {f, s}).pop()                      # the third centre: the only row with D^2 > 0
            rs.random_sample()
            want.append([f, s, t])
            seen.add((f, s))
        assert kr.kmeanspp_seeds(S, 3, 3, seed).tolist() == want
        assert kr.kmeanspp_seeds(S, 2, 3, seed)[0].tolist() == want[0][:2]
    assert len(seen) == 6                                       # every branch of the table was taken
    # all rows equal: the total of D^2 is 0, the lowest free index every time
    rs = np.random.RandomState(5)
    f = int(rs.randint(4))
    assert kr.kmeanspp_seeds(np.ones((4, 2)), 3, 1, 5)[0].tolist() == [f] + [i for i in range(4) if i != f][:2]


def test_classifiability_on_designed_partitions():
    rs = np.random.RandomState(0)
    P = rs.standard_normal((4, 6))
    assert kr.classifiability(np.stack([P, P, P])) == pytest.approx(1.0, abs=1e-15)
    assert kr.classifiability(np.stack([P, P[[2, 0, 3, 1]], 3.0 * P[::-1]])) == pytest.approx(1.0, abs=1e-15)
    assert np.isnan(kr.classifiability(P[None]))
    # two restarts in the plane: P = (e1, e2), Q = (e1, (e1 + e2) / sqrt 2): c(P, Q) = min(1, cos 45) and c(Q, P) the same
    Pm = np.array([[1.0, 0.0], [0.0, 1.0]])
    Qm = np.array([[1.0, 0.0], [1.0, 1.0]])
    assert kr.classifiability(np.stack([Pm, Qm])) == pytest.approx(np.sqrt(0.5), abs=1e-15)
    # c(P, Q) is not symmetric: Q = (e1, e1): c(P, Q) = min(1, 0) = 0, c(Q, P) = 1
    assert kr.classifiability(np.stack([Pm, np.array([[1.0, 0.0], [2.0, 0.0]])])) == pytest.approx(0.5, abs=1e-15)
    assert kr.classifiability(np.stack([Pm, np.zeros((2, 2))])) == 0.0


def test_the_case_list_reaches_every_edge_the_operator_test_names():
    ns, qs, ks, Rs = (set(c[i] for c in kr.CASES) for i in range(4))
    assert ns >= {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 4099}
    assert qs >= {1, 2, 3, 4, 5, 16, 31, 32} and ks >= {1, 2, 3, 31, 32} and Rs >= {1, 2, 3, 300}
    assert sum(c[2] == c[0] for c in kr.CASES) >= 3                               # k = n
    assert {c[4] for c in kr.CASES} == {"blobs", "decades", "dups"}
    assert len({kr.case_id(c) for c in kr.CASES}) == len(kr.CASES)


@pytest.mark.parametrize("case", kr.CASES, ids=kr.case_id)
def test_the_reference_alone_keeps_the_undecided_share(case):
    """the float64 trajectory of STEPS one-step launches from every start of the case: the rows whose margin is at most
    2 (q + 3) 2^-24, in either assignment of a step, stay within 0.1 % of the rows (one row is always allowed)"""
    n, q, k, R, _ = case
    Z, C0 = kr.make_case(case)
    assert Z.shape == (n, q) and C0.shape == (R, k, q) and Z.dtype == np.float32 and np.isfinite(Z).all()
    thr, worst = kr.undecided_margin(q), 0
    for r in range(min(R, 12)):                                                   # (the first dozen of 300 starts)
        C = C0[r].astype(np.float64)
        for _ in range(kr.STEPS):
            st = kr.step(Z, C)
            worst = max(worst, int((st["margin0"] <= thr).sum()), int((st["margin"] <= thr).sum()))
            C = st["C"].astype(np.float32).astype(np.float64)                     # (a launch hands float32 centroids on)
    print(f"{kr.case_id(case)}: undecided rows at most {worst} of {n}, allowed {kr.allowed_undecided(n)}")
    assert worst <= kr.allowed_undecided(n), f"seed {kr.case_seed(case)}"
