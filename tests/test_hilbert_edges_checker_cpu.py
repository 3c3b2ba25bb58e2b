"""The error measure of tests/test_gpu_hilbert_edges.py, and its own test (no GPU).

The Hilbert stage's earlier tests scale the error by the maximum of the whole field.  The one-kernel route puts two features
into one complex transform (series of up to 8192 samples), so the rounding of a feature is relative to the larger of the
two -- and to nothing else: whatever a feature picks up from another pair (stale LDS, a wrong coefficient slot, a prefetched
register that survives a trip) is an error however small it is next to the largest feature of the field.  `check_groups`
holds every feature to the scale of its own transform group."""

import numpy as np

from oracle import eof_oracle as orc


def pair_group(p):
    """series of up to 8192 samples: features 2j and 2j + 1 share a transform (an odd last feature is alone)"""
    return lambda f: [g for g in (f, f ^ 1) if g < p]


def own_group(f):
    """longer series (one feature per workgroup, or per hipFFT batch row)"""
    return [f]


def group_ratios(got, ref_part, ref_complex, group):
    """per feature: max_t |got - ref_part| over the largest |ref_complex| of its group (0 / 0 counts as 0)"""
    got, ref_part = np.asarray(got, dtype=np.float64), np.asarray(ref_part, dtype=np.float64)
    assert got.shape == ref_part.shape == ref_complex.shape, (got.shape, ref_part.shape, ref_complex.shape)
    p = got.shape[1]
    err = np.abs(got - ref_part).max(axis=0)
    own = np.abs(ref_complex).max(axis=0)
    scale = np.array([max(own[g] for g in group(f)) for f in range(p)])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / scale)


def check_groups(got, ref_part, ref_complex, group, tol, what=""):
    """assert  max_t |got[t, f] - ref_part[t, f]| <= tol * max(|ref_complex[:, g]| for g in group(f))  for every feature f;
    -> the largest ratio error / scale (for the record)"""
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    r = group_ratios(got, ref_part, ref_complex, group)
    worst = int(np.argmax(r))
    assert r[worst] <= tol, f"{what}: feature {worst} of {r.size} is off by {r[worst]:.3e} of its group's scale (allowed {tol:.1e})"
    return float(r[worst])


def _field(n, p, factors):
    t = np.arange(n)[:, None]
    x = np.linspace(0, 2 * np.pi, p)[None, :]
    X = 3.0 * np.cos(0.21 * t - 2 * x) + 1.7 * np.cos(0.37 * t + 3 * x + 0.4) + 0.9 * np.sin(0.11 * t - x) + 0.01 * t
    return X * np.asarray(factors, dtype=np.float64)[None, :]


def test_own_scale_form_rejects_what_the_whole_field_form_accepts():
    """one late feature off by 1e-5 of ITS OWN scale in a field whose largest feature is 1e6 times bigger"""
    n, p, f = 96, 9, 7
    factors = np.ones(p); factors[0] = 1.0e6
    ref = orc.hilbert_transform(_field(n, p, factors), padding="exp", decay_factor=0.35)
    own = np.abs(ref).max(axis=0)
    assert own[0] >= 0.9e6 * own[f] and own[f ^ 1] <= 2.0 * own[f]
    for part in (ref.imag, ref.real):
        assert check_groups(part.copy(), part, ref, pair_group(p), 2e-6) == 0.0
        got = part.copy()
        got[n // 3, f] += 1e-5 * own[f]
        assert np.abs(got - part).max() <= 2e-6 * np.abs(ref).max()          # the whole-field form: accepted
        for group in (pair_group(p), own_group):
            try:
                check_groups(got, part, ref, group, 2e-6, "perturbed")
            except AssertionError as e:
                assert f"feature {f} of {p}" in str(e)
            else:
                raise AssertionError("the own-scale form accepted a 1e-5 perturbation")
        r = group_ratios(got, part, ref, pair_group(p))
        assert np.count_nonzero(r) == 1 and 4e-6 <= r[f] <= 1e-5              # (the partner is at most twice as large)


def test_groups_and_degenerate_scales():
    assert pair_group(5)(0) == [0, 1] and pair_group(5)(3) == [3, 2] and pair_group(5)(4) == [4] and own_group(3) == [3]
    n, p = 40, 5
    factors = np.array([1.0, 1.0e-3, 1.0e3, 0.0, 1.0])
    ref = orc.hilbert_transform(_field(n, p, factors), padding=None)
    got = ref.imag.copy()
    got[:, 1] += 1e-6 * np.abs(ref[:, 0]).max()                # the small partner of a pair: bounded by the PAIR's scale ...
    assert 0.9e-6 <= check_groups(got, ref.imag, ref, pair_group(p), 2e-6) <= 1.1e-6
    r = group_ratios(got, ref.imag, ref, own_group)             # ... and far off its own
    assert r[1] > 5e-4
    got = ref.imag.copy()
    got[3, 3] = 1e-30                                           # an all-zero feature alone in its group: exact zeros or nothing
    assert check_groups(got, ref.imag, ref, pair_group(p), 2e-6) <= 1e-30
    assert np.isinf(group_ratios(got, ref.imag, ref, own_group)[3])
    got[3, 3] = np.nan
    try:
        check_groups(got, ref.imag, ref, pair_group(p), 2e-6)
    except AssertionError as e:
        assert "non-finite" in str(e)
    else:
        raise AssertionError("NaN accepted")
