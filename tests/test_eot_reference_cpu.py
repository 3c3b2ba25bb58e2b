"""The two float64 restatements of empirical orthogonal teleconnections (tests/eot_reference.py) against each other and
against the identities of the method, without a GPU: the textbook form (explicit p x p covariance, explicit deflation of the
field) and the Gram form the model uses must name the same base points and agree to 1e-10 relative on scores, series and
patterns, on random fields and on the designed field of tests/test_gpu_eot.py."""

import numpy as np
import pytest

import eot_reference as er

RTOL = 1e-10


def random_field(n, p, seed):
    rng = np.random.default_rng(seed)
    k = min(n, p, 6)
    X = rng.standard_normal((n, k)) @ (rng.standard_normal((k, p)) * np.linspace(3.0, 0.5, k)[:, None])
    X = X + 0.3 * rng.standard_normal((n, p))
    return X - X.mean(axis=0)


FIELDS = {"33x70": (33, 70, 1), "64x129": (64, 129, 2), "130x65": (130, 65, 3), "designed": None}


def field(name):
    return er.designed_field() if FIELDS[name] is None else random_field(*FIELDS[name])


@pytest.mark.parametrize("name", list(FIELDS))
def test_textbook_and_gram_form_agree(name):
    X = field(name)
    K = 3 if name == "designed" else 5
    a, g = er.textbook(X, K), er.gram_form(X, K)
    np.testing.assert_array_equal(a["base"], g["base"])
    for key in ("score", "series", "patterns", "all_scores", "den"):
        scale = np.abs(a[key]).max()
        assert np.abs(a[key] - g[key]).max() <= RTOL * scale, key


@pytest.mark.parametrize("name", list(FIELDS))
def test_identities(name):
    X = field(name)
    n, p = X.shape
    K = 3 if name == "designed" else 5
    for ref in (er.textbook(X, K), er.gram_form(X, K)):
        R, B, b = ref["series"], ref["patterns"], ref["base"]
        rn2 = np.sum(R * R, axis=0)
        # score_b = |w|^2 with w = X^T t = beta |r|
        np.testing.assert_allclose(ref["score"], np.sum(B * B, axis=0) * rn2, rtol=RTOL)
        # beta_k[b_k] = 1
        np.testing.assert_allclose(B[b, np.arange(K)], 1.0, rtol=RTOL)
        # the series are mutually orthogonal
        Gm = R.T @ R
        assert np.abs(Gm - np.diag(rn2)).max() <= RTOL * rn2.max()
        # the explained variances sum to what the deflation removed from the field
        XK = X - R @ B.T
        np.testing.assert_allclose(ref["score"].sum() / (n - 1), (np.sum(X * X) - np.sum(XK * XK)) / (n - 1), rtol=RTOL)
        # the transform recursion returns the series of the training field
        np.testing.assert_allclose(er.transform(X[:, b], B, b), R, atol=RTOL * np.abs(R).max())
        assert len(set(b.tolist())) == K


def test_designed_field_has_its_margin():
    X = er.designed_field()
    assert X.shape == (er.DESIGNED_N, 36) and np.abs(X.mean(axis=0)).max() < 1e-14
    ref = er.textbook(X, 3)
    assert tuple(ref["base"]) == er.DESIGNED_BASE
    for k in range(3):
        s = np.sort(ref["all_scores"][k])[::-1]
        assert s[1] < 0.95 * s[0]                              # measured: 0.882, 0.869, 0.797


def test_given_base_points_are_followed():
    X = random_field(33, 70, 1)
    free = er.textbook(X, 3)
    forced = [int(free["base"][0]), int(np.argsort(free["all_scores"][1])[-2]), 4]
    a, g = er.textbook(X, 3, base=forced), er.gram_form(X, 3, base=forced)
    assert a["base"].tolist() == forced and g["base"].tolist() == forced
    assert np.abs(a["patterns"] - g["patterns"]).max() <= RTOL * np.abs(a["patterns"]).max()


def test_a_duplicate_of_a_base_point_is_guarded():
    X = random_field(33, 20, 5)
    b0 = int(er.textbook(X, 1)["base"][0])
    dup = (b0 + 7) % 20
    X[:, dup] = X[:, b0]
    ref = er.textbook(X, 4)                                    # (identical columns of C: identical arithmetic, an exact tie)
    first = min(b0, dup)
    assert ref["base"][0] == first                             # the lowest index among equals
    assert (b0 + dup - first) not in ref["base"].tolist()
    assert np.all(ref["all_scores"][1:, [b0, dup]] == 0.0)
