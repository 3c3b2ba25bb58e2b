"""The float64 restatement of trend EOF analysis (tests/trend_reference.py) against brute force -- an O(n^2) rank count -- and the
closed forms: every row of Q is a permutation of 0 .. n - 1, so its mean is (n - 1) / 2 and its variance (ddof = 1)
n (n + 1) / 12.  No GPU."""

import numpy as np
import pytest

import trend_reference as tr


def special_series(n, rng):
    """the kinds of series the GPU test sorts, as rows of one float32 panel"""
    t = np.arange(n, dtype=np.float32)
    rows = [rng.standard_normal(n).astype(np.float32), np.full(n, 2.5, np.float32), rng.integers(0, 2, n).astype(np.float32),
            -t, t.copy(), np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32),
            (rng.integers(-3, 4, n) * np.float32(1e-45)).astype(np.float32)]
    mixed = rng.standard_normal(n).astype(np.float32)
    mixed[rng.random(n) < 0.2] = np.inf
    mixed[rng.random(n) < 0.2] = -np.inf
    nan_pos = np.frombuffer(np.uint32(0x7fc00001).tobytes(), np.float32)[0]
    nan_neg = np.frombuffer(np.uint32(0xffc00000).tobytes(), np.float32)[0]
    mixed[rng.random(n) < 0.15] = nan_pos
    mixed[rng.random(n) < 0.15] = nan_neg
    rows.append(mixed)
    one = np.full(n, -1.0, np.float32)
    one[n // 2] = -7.0
    rows.append(one)
    return np.stack(rows)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 17, 64, 65])
def test_order_positions_is_the_brute_force_rank_count(n):
    T = special_series(n, np.random.default_rng(n))
    Q = tr.order_positions(T)
    assert Q.shape == T.shape
    for j in range(T.shape[0]):
        assert np.array_equal(Q[j], tr.brute_positions(T[j])), j
        assert np.array_equal(np.sort(Q[j]), np.arange(n))


def test_ties_negative_zero_and_nans():
    nan = np.float32(np.nan)
    T = np.array([[0.0, -0.0, 0.0, -0.0], [1.0, nan, -np.inf, -nan], [np.inf, nan, np.inf, 3.0e38]], dtype=np.float32)
    assert np.array_equal(tr.order_positions(T), [[0, 1, 2, 3], [2, 0, 1, 3], [3, 0, 2, 1]])
    assert np.array_equal(tr.order_positions(np.full((1, 9), 4.0, np.float32))[0], np.arange(9))
    with pytest.raises(TypeError):
        tr.order_positions(np.zeros((2, 3)))


@pytest.mark.parametrize("n", [2, 5, 64, 257])
def test_closed_forms_of_a_permutation(n):
    rng = np.random.default_rng(100 + n)
    T = rng.standard_normal((6, n)).astype(np.float32)
    Q = tr.order_positions(T).astype(np.float64)
    np.testing.assert_allclose(Q.mean(axis=1), (n - 1) / 2.0, rtol=1e-15)
    np.testing.assert_allclose(Q.var(axis=1, ddof=1), n * (n + 1) / 12.0, rtol=1e-13)
    w = rng.random(6) + 0.5
    Z64 = (Q - (n - 1) / 2.0) * w[:, None]
    np.testing.assert_allclose(np.sum(Z64 * Z64) / (n - 1), tr.total_variance(n, w), rtol=1e-13)
    Z = tr.rank_values(Q.astype(np.int64), w)
    assert Z.dtype == np.float32 and np.array_equal(Z, Z64.astype(np.float32))
    assert np.array_equal(tr.rank_values(Q.astype(np.int64)), (Q - (n - 1) / 2.0).astype(np.float32))


def test_regression_on_the_standardized_series():
    rng = np.random.default_rng(5)
    n, p, k = 40, 7, 3
    X = rng.standard_normal((n, p))
    S = rng.standard_normal((n, k)) * [3.0, 0.1, 20.0] + [5.0, -2.0, 0.0]
    Sh = tr.standardized(S)
    np.testing.assert_allclose(Sh.mean(axis=0), 0.0, atol=1e-14)
    np.testing.assert_allclose(Sh.std(axis=0, ddof=1), 1.0, rtol=1e-14)
    R = tr.regression(X, S)
    for j in range(p):
        for m in range(k):
            # the least-squares slope of column j on the standardized series m (unit variance: slope = covariance)
            slope = np.polyfit(Sh[:, m], X[:, j], 1)[0]
            np.testing.assert_allclose(R[j, m], slope, rtol=1e-10, atol=1e-12)


def test_restate_of_a_monotone_rank_one_field():
    n, p = 30, 5
    g = np.exp(np.arange(n) / 7.0)
    a = np.array([2.0, -1.0, 0.5, -3.0, 1.5])
    X = (g[:, None] * a).astype(np.float32)
    V = np.sign(a)[:, None] / np.sqrt(p)
    ref = tr.restate(X, V)
    for j in range(p):
        assert np.array_equal(ref["Q"][j], np.arange(n) if a[j] > 0 else np.arange(n)[::-1])
    assert ref["s"][1] <= 1e-12 * ref["s"][0]
    np.testing.assert_allclose(ref["s"][0] ** 2 / (n - 1), ref["total_variance"], rtol=1e-13)
