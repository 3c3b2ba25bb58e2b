"""The float64 restatement of the teleconnectivity model (tests/teleconnectivity_reference.py) against a brute-force
numpy.corrcoef form written with loops, and the identities of the definition.  No GPU."""

import numpy as np
import pytest

import teleconnectivity_reference as tr


def brute_force(X, n_modes, max_corr):
    """the definition with numpy.corrcoef and loops over the points"""
    n, p = X.shape
    R = np.corrcoef(X.T)
    R = 0.5 * (R + R.T)                                # (symmetric bit for bit: the two poles of a seesaw tie exactly)
    rmin, partner = np.full(p, np.nan), np.full(p, -1)
    for j in range(p):
        for i in range(p):
            if i != j and not np.isnan(R[j, i]) and (partner[j] < 0 or R[j, i] < rmin[j]):
                rmin[j], partner[j] = R[j, i], i
    Z = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    blocked, pairs, scores, comps = set(), [], [], []
    order = sorted((j for j in range(p) if rmin[j] < 0.0), key=lambda j: (rmin[j], j))
    for k in range(n_modes):
        b = next(j for j in order if j not in blocked and partner[j] not in blocked)
        a = int(partner[b])
        s = (Z[:, b] - Z[:, a]) / 2.0
        pairs.append((b, a))
        scores.append(s)
        comps.append(np.array([np.corrcoef(X[:, j], s)[0, 1] for j in range(p)]))
        blocked |= {j for j in range(p) if max(abs(R[j, b]), abs(R[j, a])) > max_corr}
    return rmin, partner, pairs, np.stack(scores, axis=1), np.stack(comps, axis=1)


@pytest.mark.parametrize("n,p,seed,max_corr", [(40, 25, 0, 0.5), (15, 30, 1, 0.3), (60, 12, 2, 0.7)])
def test_restatement_against_brute_force(n, p, seed, max_corr):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 4)) @ rng.standard_normal((4, p)) + rng.standard_normal((n, p)) + 3.0
    K = 2
    rmin, partner, pairs, S, C = brute_force(X, K, max_corr)
    ref = tr.model(X - X.mean(axis=0), K, max_corr)
    np.testing.assert_allclose(ref["rmin"], rmin, atol=1e-13)
    np.testing.assert_array_equal(ref["partner"], partner)
    assert ref["pairs"] == pairs == ref["choice"]
    np.testing.assert_allclose(ref["scores"], S, atol=1e-12 * np.abs(S).max())
    np.testing.assert_allclose(ref["components"], C, atol=1e-12)
    Xc = X - X.mean(axis=0)
    for k in range(K):
        sh = S[:, k] / np.linalg.norm(S[:, k])
        np.testing.assert_allclose(ref["sv"][k], np.linalg.norm(Xc.T @ sh), rtol=1e-12)
    np.testing.assert_allclose(ref["total_variance"], X.var(axis=0, ddof=1).sum(), rtol=1e-12)
    np.testing.assert_allclose(ref["explained_variance"], ref["sv"] ** 2 / (n - 1.0), rtol=1e-15)


def test_constant_columns_are_nan_and_never_partners():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 9))
    X[:, 3] = 0.0
    X -= X.mean(axis=0)
    ref = tr.model(X, 1)
    assert np.isnan(ref["rmin"][3]) and ref["partner"][3] == -1 and 3 not in ref["partner"]
    assert ref["components"][3, 0] == 0.0
    one = tr.row_minima(np.array([[1.0]]))
    assert np.isnan(one[0][0]) and one[1][0] == -1


def test_the_lowest_index_wins_a_tie():
    R = np.array([[1.0, -0.5, -0.5, 0.1], [-0.5, 1.0, 0.2, 0.0], [-0.5, 0.2, 1.0, -0.5], [0.1, 0.0, -0.5, 1.0]])
    rmin, partner = tr.row_minima(R)
    np.testing.assert_array_equal(partner, [1, 0, 0, 2])
    np.testing.assert_array_equal(rmin, [-0.5, -0.5, -0.5, -0.5])


def test_identities():
    rng = np.random.default_rng(8)
    n, p, K = 50, 30, 3
    X = rng.standard_normal((n, 5)) @ rng.standard_normal((5, p)) + 2.0 * rng.standard_normal((n, p))
    X -= X.mean(axis=0)
    ref = tr.model(X, K, 0.6)
    # relabelling the points relabels the map and the partners
    perm = rng.permutation(p)
    pr = tr.model(X[:, perm], K, 0.6)
    np.testing.assert_allclose(pr["rmin"], ref["rmin"][perm], atol=1e-14)
    inv = np.argsort(perm)
    np.testing.assert_array_equal(pr["partner"], inv[ref["partner"][perm]])
    # scaling a column (a feature weight) changes no correlation
    sc = tr.model(X * rng.uniform(0.5, 2.0, p), K, 0.6)
    np.testing.assert_allclose(sc["rmin"], ref["rmin"], atol=1e-13)
    assert sc["pairs"] == ref["pairs"]
    # the poles have opposite signs, |comp| <= 1 up to rounding, and the index correlates equally strongly with both
    C = ref["components"]
    for k, (b, a) in enumerate(ref["pairs"]):
        assert C[b, k] > 0.0 > C[a, k]
        np.testing.assert_allclose(C[b, k], -C[a, k], atol=1e-12)
        assert C[b, k] == pytest.approx(np.sqrt((1.0 - ref["rmin"][b]) / 2.0), abs=1e-12)
    assert np.abs(C).max() <= 1.0 + 1e-12
    # later poles are separated from earlier ones
    R = tr.correlation(X)
    for k in range(1, K):
        for m in range(k):
            for x in ref["pairs"][k]:
                assert max(abs(R[x, ref["pairs"][m][0]]), abs(R[x, ref["pairs"][m][1]])) <= 0.6


def test_the_designed_field_has_its_margins():
    X = tr.designed_field()
    X -= X.mean(axis=0)
    ref = tr.model(X, 3)
    assert [frozenset(q) for q in ref["pairs"]] == [frozenset(q) for q in tr.DESIGNED_PAIRS]
    B, Bj = tr.pair_bound(X)
    R = tr.correlation(X)
    for k, (b, a) in enumerate(ref["pairs"]):
        row = np.delete(R[b], [b, a])
        assert row.min() - R[b, a] > 0.03 > 100 * Bj[b]                  # the partner of a pole: no near tie
        key = np.where(ref["open"][k], ref["rmin"], np.inf)
        assert np.sort(key)[2] - ref["rmin"][b] > 0.03                   # the next candidate after the pair itself
    with pytest.raises(ValueError, match="exhausted"):
        tr.model(X, 30, 0.05)
