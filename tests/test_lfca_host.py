"""CPU tests of the host helpers of low-frequency component analysis (xeofs_amd/single/lfca.py): the Lanczos weights, the
mirror index, the closed-form linear trend and the constructor's argument checks.  No GPU."""

import numpy as np
import pytest

from xeofs_amd.single.lfca import LFCA, default_half_width, lanczos_weights, linear_trend, reflect_index


def response(w, f):
    """the amplitude response w_0 + 2 sum_k w_k cos(2 pi f k) of the symmetric filter w_|k|"""
    k = np.arange(1, w.size)
    return w[0] + 2.0 * np.sum(w[1:] * np.cos(2.0 * np.pi * f * k))


@pytest.mark.parametrize("cutoff,h", [(40, 60), (24, 33), (2.5, 1), (10.0, 7), (120, 5)])
def test_weights_sum_to_one(cutoff, h):
    w = lanczos_weights(cutoff, h)
    assert w.dtype == np.float64 and w.shape == (h + 1,)
    assert abs(w[0] + 2.0 * w[1:].sum() - 1.0) <= 1e-15
    # symmetric by construction: the filter is w_|k|, so the two-sided kernel equals its reverse
    full = np.concatenate([w[:0:-1], w])
    assert np.array_equal(full, full[::-1]) and full.size == 2 * h + 1
    assert abs(response(w, 0.0) - 1.0) <= 1e-15


def test_weights_are_duchons():
    """against the definition written out term by term"""
    cutoff, h = 40, 60
    fc = 1.0 / cutoff
    raw = [2.0 * fc]
    for k in range(1, h + 1):
        sigma = np.sin(np.pi * k / (h + 1)) / (np.pi * k / (h + 1))
        raw.append(np.sin(2.0 * np.pi * fc * k) / (np.pi * k) * sigma)
    raw = np.array(raw)
    np.testing.assert_allclose(lanczos_weights(cutoff, h), raw / (raw[0] + 2.0 * raw[1:].sum()), rtol=1e-14, atol=1e-18)


def test_amplitude_response():
    cutoff, h = 40, 60
    w = lanczos_weights(cutoff, h)
    fc = 1.0 / cutoff
    at_cut, low = response(w, fc), response(w, fc / 4)
    print(f"response at fc = {at_cut:.4f}, at fc / 4 = {low:.4f}")
    assert abs(at_cut - 0.5) <= 0.05
    assert low > 0.95


def test_weight_errors():
    for cutoff in (2, 1.5, 0, -3, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            lanczos_weights(cutoff, 5)
    with pytest.raises(ValueError, match="half-width"):
        lanczos_weights(10, 0)


@pytest.mark.parametrize("n", [2, 3, 17])
def test_reflect_index_is_numpys_reflect(n):
    base = np.arange(n)
    for h in range(0, n):
        want = np.pad(base, h, mode="reflect")
        got = reflect_index(np.arange(-h, n + h), n)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, h)
    with pytest.raises(ValueError):
        reflect_index(np.array([-n]), n)
    with pytest.raises(ValueError):
        reflect_index(np.array([2 * (n - 1) + 1]), n)


def test_linear_trend_is_polyfit():
    rng = np.random.default_rng(0)
    for n, p in [(2, 3), (3, 1), (50, 7), (601, 4)]:
        S = (rng.standard_normal((n, p)) + 0.01 * np.arange(n)[:, None] * rng.standard_normal(p) + 5.0).astype(np.float32)
        tr = linear_trend(S)
        assert tr.shape == (2, p) and tr.dtype == np.float64
        t = np.arange(n, dtype=np.float64)
        for j in range(p):
            b, a = np.polyfit(t, S[:, j].astype(np.float64), 1)
            scale = np.abs(S[:, j]).max()
            assert abs(tr[0, j] - a) <= 1e-11 * scale and abs(tr[1, j] - b) <= 1e-11 * scale, (n, j)
    with pytest.raises(ValueError):
        linear_trend(np.zeros((1, 3)))
    with pytest.raises(ValueError):
        linear_trend(np.zeros(5))


def test_default_half_width():
    assert default_half_width(600, 40) == 60
    assert default_half_width(500, 24) == 36
    assert default_half_width(30, 40) == 29
    assert default_half_width(1000, 2.5) == 4


def test_constructor_errors():
    for cutoff in (2, 1, 0.0, -5):
        with pytest.raises(ValueError, match="cutoff"):
            LFCA(n_modes=2, cutoff=cutoff)
    for window in (4, 120, 0, 2.5):
        with pytest.raises(ValueError, match="window must be an odd"):
            LFCA(n_modes=2, cutoff=10, window=window)
    for window in (1, -3):
        with pytest.raises(ValueError, match="at least 3"):
            LFCA(n_modes=2, cutoff=10, window=window)
    with pytest.raises(ValueError, match="n_modes must be smaller or equal to n_pca_modes"):
        LFCA(n_modes=11, cutoff=10, n_pca_modes=10)
    m = LFCA(n_modes=3, cutoff=40, window=121, detrend=False, n_pca_modes=20)
    prm = m.get_params()
    assert prm["cutoff"] == 40 and prm["window"] == 121 and prm["detrend"] is False and prm["n_pca_modes"] == 20
    assert m.attrs["model"] == "LFCA"


def test_window_against_the_sample_count():
    """h > n - 1 is an error at fit time, where n is known; the check is the model's `_half_width`"""
    m = LFCA(n_modes=1, cutoff=10, window=21)
    assert m._half_width(11) == 10
    with pytest.raises(ValueError, match="n_samples - 1"):
        m._half_width(10)
    assert LFCA(n_modes=1, cutoff=10)._half_width(8) == 7          # the default is clipped to n - 1


def test_exported_from_single():
    import xeofs_amd as xe

    assert xe.single.LFCA is LFCA
