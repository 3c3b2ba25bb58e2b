"""Host logic of xeofs_amd.single.DINEOF (no GPU): the choice of the cross-validation points, the grouping of flat indices
into words of the gap mask, the stopping rule, the choice of the mode count, and the constructor's validation."""

import numpy as np
import pytest

from xeofs_amd.single import dineof as dn


def test_cv_selection_is_reproducible_avoids_gaps_and_has_m_unique_entries():
    n, p = 40, 57
    gap = np.random.default_rng(0).random(n * p) < 0.3
    n_valid = int((~gap).sum())
    m = dn.cv_count(n_valid, 0.05, 30)
    assert m == max(30, int(round(0.05 * n_valid))) and m > 30
    picks = []
    for _ in range(2):
        cand = dn.cv_candidates(n * p, m, random_state=11)
        assert cand.dtype == np.int64 and cand.size == 2 * m and np.unique(cand).size == cand.size
        picks.append(dn.cv_keep(cand, gap[cand], m))
    assert np.array_equal(picks[0], picks[1])                        # reproducible from the seed
    idx = picks[0]
    assert idx.size == m and np.unique(idx).size == m                # m entries, no duplicates
    assert not gap[idx].any()                                        # never a gap
    assert idx.min() >= 0 and idx.max() < n * p
    assert not np.array_equal(idx, dn.cv_keep(dn.cv_candidates(n * p, m, 12), gap[dn.cv_candidates(n * p, m, 12)], m))
    # the first m survivors, in drawing order
    cand = dn.cv_candidates(n * p, m, random_state=11)
    assert np.array_equal(idx, cand[~gap[cand]][:m])


def test_cv_count_floor_and_small_fields():
    assert dn.cv_count(1000, 0.01, 30) == 30 and dn.cv_count(10000, 0.01, 30) == 100
    assert dn.cv_candidates(50, 30, 0).size == 50                    # never more candidates than entries


def test_group_bits():
    p, ldw = 100, 5                                                  # ceil(100 / 32) = 4 words, one of padding
    # two indices in one word, bit 31, and the same columns in another row
    idx = np.array([3 * p + 33, 3 * p + 40, 0 * p + 31, 3 * p + 31, 7 * p + 99])
    words, masks = dn.group_bits(idx, p, ldw)
    assert words.dtype == np.int64 and masks.dtype == np.int32
    assert words.tolist() == [0, 3 * ldw, 3 * ldw + 1, 7 * ldw + 3]
    assert masks.view(np.uint32).tolist() == [1 << 31, 1 << 31, (1 << 1) | (1 << 8), 1 << 3]
    assert masks[0] < 0                                              # bit 31 is the sign of an int32 word
    # an index beyond 2^32
    p, ldw = 1 << 20, (1 << 20) // 32
    big = (1 << 13) * p + 77                                         # 2^33 + 77
    assert big >= 1 << 32
    words, masks = dn.group_bits([big, 5], p, ldw)
    assert words.tolist() == [0, (1 << 13) * ldw + 2] and masks.view(np.uint32).tolist() == [1 << 5, 1 << 13]
    # nothing
    words, masks = dn.group_bits(np.empty(0, np.int64), 10, 1)
    assert words.size == 0 and masks.size == 0
    # against a dense mask
    rng = np.random.default_rng(3)
    n, p = 9, 70
    ldw = 3
    idx = rng.choice(n * p, 200, replace=False)
    words, masks = dn.group_bits(idx, p, ldw)
    assert np.all(np.diff(words) > 0)
    dense = np.zeros((n, ldw * 32), bool)
    dense[idx // p, idx % p] = True
    ref = np.packbits(dense, axis=1, bitorder="little").view(np.uint32).reshape(-1)
    got = np.zeros(n * ldw, np.uint32)
    got[words] = masks.view(np.uint32)
    assert np.array_equal(got, ref)


def test_stop_rule_and_mode_choice():
    assert dn.converged(sum_d2=4.0e-6 * 10, count=10, tol=1e-3, rms=2.0)            # sqrt(4e-6) = 2e-3 <= 1e-3 * 2
    assert not dn.converged(sum_d2=4.1e-6 * 10, count=10, tol=1e-3, rms=2.0)
    assert dn.converged(0.0, 0, 1e-3, 1.0)                                           # nothing to fill
    curve = [0.9, 0.5, 0.2, 0.21]
    assert [dn.stop_raising(curve[:i]) for i in range(1, 5)] == [False, False, False, True]
    assert dn.optimal_modes(curve) == 3
    assert dn.optimal_modes([0.3]) == 1 and not dn.stop_raising([0.3])
    assert dn.optimal_modes([0.5, 0.2, 0.2]) == 2 and not dn.stop_raising([0.5, 0.2, 0.2])      # a tie: the fewer modes
    assert dn.optimal_modes([0.5, 0.4, 0.3]) == 3                                    # n_modes exhausted: the last


def test_parameter_validation():
    import xeofs_amd as xe

    m = xe.single.DINEOF()
    prm = m.get_params()
    assert (prm["n_modes"], prm["cv_fraction"], prm["cv_min"], prm["tol"], prm["max_iter"]) == (10, 0.01, 30, 1e-3, 50)
    assert m.attrs["model"] == "DINEOF" and isinstance(m, xe.single.EOF)
    for bad in (dict(n_modes=0), dict(n_modes=2.5), dict(n_modes=257), dict(cv_fraction=0.0), dict(cv_fraction=1.0),
                dict(cv_min=0), dict(tol=0.0), dict(tol=-1.0), dict(max_iter=0), dict(n_modes=250),
                dict(solver_kwargs={"n_oversamples": -1})):
        with pytest.raises(ValueError):
            xe.single.DINEOF(**bad)
    xe.single.DINEOF(n_modes=246)                                    # 246 + 10 = the widest sketch
