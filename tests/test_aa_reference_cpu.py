"""The float64 restatement of archetypal analysis (tests/aa_reference.py) checked on its own, without a GPU: the sort-based
projection against Michelot's fixed point and the KKT conditions of the projection, the Gram form of the objective against
|X - A B X|^2 computed directly, the monotone history, the rank bound f >= sum_{i > k} s_i^2, and the planted field."""

import numpy as np
import pytest

import aa_reference as ar


def designed_rows(m, rs):
    rows = [rs.standard_normal(m), 10.0 * rs.standard_normal(m), np.linspace(-1.0, 1.0, m), np.full(m, 0.25),
            -1.0 - rs.random_sample(m), 10.0 ** rs.uniform(-5, 5, m), rs.dirichlet(np.ones(m))]
    one = np.zeros(m)
    one[m // 2] = 1.0
    big = rs.standard_normal(m)
    big[0] += 50.0
    return np.stack(rows + [one, big])


@pytest.mark.parametrize("m", [1, 2, 3, 17, 64, 257, 2000])
def test_sort_projection_against_michelot_and_the_kkt_conditions(m):
    rs = np.random.RandomState(m)
    U = designed_rows(m, rs)
    P, tau = ar.project_sort(U)
    scale = np.maximum(1.0, np.abs(U).max(axis=1))
    assert np.all(P >= 0.0) and np.all(np.abs(P.sum(axis=1) - 1.0) <= 4e-16 * m * scale)
    # KKT: x_j = u_j - tau where x_j > 0, and u_j - tau <= 0 where x_j = 0
    assert np.all(np.abs(np.where(P > 0.0, P - (U - tau[:, None]), 0.0)) == 0.0)
    assert np.all(np.where(P == 0.0, U - tau[:, None], -1.0) <= 0.0)
    for i in range(U.shape[0]):
        Pm, tm, rounds = ar.project_michelot(U[i])
        assert abs(tm - tau[i]) <= 8e-16 * m * scale[i] and np.all(np.abs(Pm - P[i]) <= 8e-16 * m * scale[i]) and rounds <= 12
    # a point of the simplex is its own projection; the projection is idempotent
    W = rs.dirichlet(np.ones(m), 5)
    assert np.all(np.abs(ar.project_sort(W)[0] - W) <= 4e-16)
    assert np.all(np.abs(ar.project_sort(P)[0] - P) <= 4e-16 * scale[:, None])


def test_the_projection_is_the_nearest_point():
    rs = np.random.RandomState(3)
    U = rs.standard_normal((6, 9))
    P, _ = ar.project_sort(U)
    d0 = np.sum((P - U) ** 2, axis=1)
    for _ in range(200):
        W = rs.dirichlet(rs.choice([0.2, 1.0, 5.0]) * np.ones(9), 6)
        assert np.all(np.sum((W - U) ** 2, axis=1) >= d0 - 1e-12)


def test_gram_form_of_the_objective_against_the_direct_one():
    rs = np.random.RandomState(1)
    X = rs.standard_normal((30, 55))
    K = X @ X.T
    for _ in range(5):
        A, B = rs.dirichlet(np.ones(4), 30), rs.dirichlet(0.3 * np.ones(30), 4)
        assert abs(ar.objective_gram(np.trace(K), A, K @ B.T, B) - ar.objective_direct(X, A, B)) <= 1e-12 * np.trace(K)


def test_pg_steps_never_increase_the_objective_and_stay_on_the_simplex():
    rs = np.random.RandomState(2)
    X, Z = rs.standard_normal((50, 20)), rs.standard_normal((5, 20))
    Q, M = X @ Z.T, Z @ Z.T
    A = np.full((50, 5), 0.2)
    f = [np.sum((X - A @ Z) ** 2)]
    for _ in range(8):
        A = ar.pg_steps(A, Q, M, 1.0 / ar.lambda_max(M), 3, round_m=False)
        f.append(np.sum((X - A @ Z) ** 2))
        assert np.all(A >= 0.0) and np.all(np.abs(A.sum(axis=1) - 1.0) <= 1e-14)
    assert np.all(np.diff(f) <= 1e-12 * f[0]) and f[-1] < 0.9 * f[0]


@pytest.mark.parametrize("n, p, k", [(300, 500, 4), (257, 129, 8)])
def test_noisy_mixtures_monotone_history_and_the_rank_bound(n, p, k):
    X = ar.noisy_mixtures(n, p, k, seed=n)
    Xc = X - X.mean(axis=0)
    K = Xc @ Xc.T
    idx = ar.furthest_sum(K, k, 7)
    r = ar.fit(K, k, idx)
    h = r["history"]
    assert len(h) >= 2 and np.all(np.diff(h) <= 0.0) and h[0] <= r["f_start"] and not r["stalled"]
    s = np.linalg.svd(Xc, compute_uv=False)
    assert r["f"] >= np.sum(s[k:] ** 2) and r["f"] < 0.6 * r["trK"]
    A, B = r["A"], r["B"]
    assert np.all(A >= 0) and np.all(B >= 0) and np.allclose(A.sum(1), 1, atol=1e-12) and np.allclose(B.sum(1), 1, atol=1e-12)
    assert abs(ar.objective_direct(Xc, A, B) - r["f"]) <= 1e-10 * r["trK"]
    assert np.all(np.diff(A.sum(axis=0)) <= 0.0)               # the order of the modes
    # a replay of the recorded steps reproduces the fit
    again = ar.fit(K, k, idx, replay=r["steps"])
    assert np.allclose(again["A"], A, atol=1e-12) and np.allclose(again["B"], B, atol=1e-12)


@pytest.mark.parametrize("init", [[0, 1, 2], [10, 50, 90], None])
def test_the_planted_field_is_recovered(init):
    vertices = (5, 40, 77)
    X, W = ar.planted_field(vertices=vertices)
    Xc = X - X.mean(axis=0)
    K = Xc @ Xc.T
    if init is None:
        for start in (0, 33, 95):
            assert sorted(ar.furthest_sum(K, 3, start).tolist()) == list(vertices)
        init = ar.furthest_sum(K, 3, 33)
    r = ar.fit(K, 3, init)
    picked = r["B"].argmax(axis=1)
    assert sorted(picked.tolist()) == list(vertices)
    perm = [vertices.index(v) for v in picked]
    assert np.abs(r["A"] - W[:, perm]).max() <= 0.02 and r["f"] <= 1e-4 * r["trK"]
