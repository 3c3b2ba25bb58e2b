"""Host-side tests of multi-view canonical correlation analysis (xeofs_amd.multi.CCA): the public surface and the float64
algebra that runs on the host between the kernels -- no GPU."""

import inspect

import numpy as np
import pytest


def test_multi_cca_is_exported_with_the_references_defaults():
    import xeofs_amd as xe

    assert hasattr(xe, "multi") and hasattr(xe.multi, "CCA")
    sig = inspect.signature(xe.multi.CCA.__init__).parameters
    want = dict(n_modes=2, use_coslat=False, check_nans=True, c=0, pca=True, variance_fraction=0.99, init_pca_modes=0.75,
                compute=True, eps=1e-6, random_state=None, solver="auto", solver_kwargs={}, ctx=None)
    for name, default in want.items():
        assert name in sig and sig[name].default == default, name
    assert list(sig)[1:10] == ["n_modes", "use_coslat", "check_nans", "c", "pca", "variance_fraction", "init_pca_modes",
                               "compute", "eps"]                                   # the reference's positional order
    m = xe.multi.CCA()
    assert m.attrs["model"] == "CCA" and m.get_params()["variance_fraction"] == 0.99 and not m.is_deferred


def test_the_abi_symbol_and_the_engine_constants():
    from xeofs_amd import _lib, engine

    assert "eofx_viewcov_f64" in _lib.SIGNATURES
    assert (engine.VIEWCOV_PMAX, engine.VIEWCOV_MMAX) == (4096, 64)
    assert callable(engine.viewcov)


def test_parameter_broadcasting_and_its_length_check():
    from xeofs_amd.multi.cca import process_parameter

    assert process_parameter("c", 0.5, 0, 3) == [0.5, 0.5, 0.5]
    assert process_parameter("c", None, 0, 2) == [0, 0]
    assert process_parameter("use_coslat", [True, False], False, 2) == [True, False]
    assert process_parameter("init_pca_modes", (0.5, 7), 0.75, 2) == [0.5, 7]
    with pytest.raises(ValueError, match=r"number of views passed should match number of parameter c"
                                         r"len\(views\)=3 and len\(c\)=2"):
        process_parameter("c", [0.1, 0.2], 0, 3)


def test_process_init_pca_modes():
    from xeofs_amd.multi.cca import process_init_pca_modes

    # a float is that share of min(n_samples, n_features), truncated; an integer > 1 is taken as it is
    assert process_init_pca_modes([0.75, 0.75, 1.0, 5], 130, [40, 57, 23, 300]) == [30, 42, 23, 5]
    assert process_init_pca_modes([0.75], 10, [40]) == [7]
    msg = "init_pca_modes must be either a float <= 1.0 or an integer > 1"
    for bad in (1.5, 1, 0, -3, "all", None, True):
        with pytest.raises(ValueError, match=msg):
            process_init_pca_modes([bad], 130, [40])


def test_variance_fraction_truncation():
    from xeofs_amd.multi.cca import pca_modes_to_keep

    # cumulative 0.5, 0.8, 0.9, 0.95, 0.99 less 1e-6: with fraction 0.9 the first three are at or below it, plus one
    r = [0.5, 0.3, 0.1, 0.05, 0.04]
    assert pca_modes_to_keep(r, 0.9) == (4, None)
    # an exact hit on the fraction counts as "at or below" because of the - 1e-6 ...
    assert pca_modes_to_keep(r, 0.8) == (3, None)
    # ... and a fraction a hair under it does not
    assert pca_modes_to_keep(r, 0.8 - 2e-6) == (2, None)
    # never reached: every mode is at or below, the count is one more than there are (the caller has no more to give),
    # and the reference's warning is produced
    keep, warning = pca_modes_to_keep(r, 0.995)
    assert keep == 6
    assert warning == "Warning: variance fraction 0.9950 is not reached. Only 0.9900 of variance is explained."
    # no warning when the modes explain more than 0.9999 although the fraction is not reached
    keep, warning = pca_modes_to_keep([0.7, 0.29999], 1.0)
    assert keep == 3 and warning is None
    # at least 2
    assert pca_modes_to_keep([0.999, 0.001], 0.5) == (2, None)
    assert pca_modes_to_keep([0.6, 0.3, 0.1], 0.1) == (2, None)


def test_the_shift_of_D():
    from xeofs_amd.multi.cca import shift_diagonal, shift_matrix

    d = np.array([3.0, 0.5, 2.0])
    np.testing.assert_allclose(shift_diagonal(d, 1e-6, 2), (d + 1e-6) / 2, rtol=1e-15)          # positive: only eps
    dn = np.array([3.0, -0.25, 2.0])
    np.testing.assert_allclose(shift_diagonal(dn, 1e-3, 3), (dn + 0.25 + 1e-3) / 3, rtol=1e-15)
    assert shift_diagonal(dn, 1e-3, 3).min() > 0.0
    # the dense form is cca.py:582-586 written out, and agrees with the diagonal one on a diagonal matrix
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, 6))
    D = A + A.T                                                                    # indefinite
    lam_min = np.linalg.eigvalsh(D).min()
    assert lam_min < 0
    want = (D - (min(0, lam_min) - 1e-6) * np.eye(6)) / 2
    np.testing.assert_allclose(shift_matrix(D, 1e-6, 2), want, rtol=1e-15, atol=1e-15)
    assert np.linalg.eigvalsh(shift_matrix(D, 1e-6, 2)).min() > 0.0
    np.testing.assert_allclose(np.diag(shift_matrix(np.diag(dn), 1e-3, 3)), shift_diagonal(dn, 1e-3, 3), rtol=1e-14)


def test_the_whitened_standard_form_against_lapacks_generalised_solver():
    from scipy.linalg import eigh

    from xeofs_amd.multi.cca import fix_signs, gevp_dense, gevp_diagonal, whitened_form

    rng = np.random.default_rng(1)
    p, k = 37, 4
    A = rng.standard_normal((p, p))
    C = A + A.T
    C[:10, :10] = 0.0
    C[10:, 10:][:12, :12] = 0.0                                                    # diagonal blocks removed, as in the model
    d = rng.uniform(0.2, 5.0, p)
    lam_ref, X_ref = eigh(C, np.diag(d), subset_by_index=[p - k, p - 1])
    lam_ref, X_ref = lam_ref[::-1], fix_signs(X_ref[:, ::-1])
    lam, X = gevp_diagonal(C, d, k)
    assert np.all(np.diff(lam) < 0)
    gap = np.diff(np.linalg.eigvalsh(whitened_form(C, d)[0])[-(k + 1):]).min()        # of the wanted ones, and to the next
    assert gap > 0.05
    scale = np.abs(lam_ref).max()
    np.testing.assert_allclose(lam, lam_ref, rtol=0, atol=64 * p * 2.0 ** -53 * scale)
    assert np.abs(X - X_ref).max() <= 64 * p * 2.0 ** -53 * scale / gap * np.abs(X_ref).max()
    np.testing.assert_allclose(X.T @ (d[:, None] * X), np.eye(k), atol=1e-12)      # x^T D x = 1
    np.testing.assert_allclose(C @ X, (d[:, None] * X) * lam, atol=1e-11 * scale)
    lam_d, X_d = gevp_dense(C, np.diag(d), k)
    np.testing.assert_allclose(lam_d, lam_ref, rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(X_d, X_ref, atol=1e-12)


def test_the_sign_rule():
    from xeofs_amd.multi.cca import fix_signs

    x = np.array([[0.5, -0.5, 2.0],
                  [-3.0, 0.5, -2.0],
                  [1.0, -0.25, 1.0]])
    got = fix_signs(x)
    # column 0: the largest modulus is -3 -> flipped; column 1: a tie of -0.5 and 0.5, the lowest index decides -> flipped;
    # column 2: a tie of 2 and -2, the lowest index is positive -> kept
    np.testing.assert_array_equal(got, x * np.array([-1.0, -1.0, 1.0]))
    np.testing.assert_array_equal(fix_signs(got), got)
    assert x[0, 0] == 0.5                                                          # the argument is not modified


def test_total_explained_covariance_takes_every_second_modulus():
    from xeofs_amd.multi.cca import total_explained_covariance

    # two views: the block cross-covariance [[0, K], [K^T, 0]] has the eigenvalues +-s(K); its singular values are every
    # s twice, so every second one is the singular values of K
    rng = np.random.default_rng(2)
    K = rng.standard_normal((5, 7))
    M = np.block([[np.zeros((5, 5)), K], [K.T, np.zeros((7, 7))]])
    s = np.linalg.svd(K, compute_uv=False)
    sv = np.linalg.svd(M, compute_uv=False)
    assert np.isclose(total_explained_covariance(np.linalg.eigvalsh(M), 5), sv[::2][:5].sum(), rtol=1e-13)
    assert np.isclose(total_explained_covariance(np.linalg.eigvalsh(M), 5), s.sum(), rtol=1e-13)
    assert np.isclose(total_explained_covariance(np.linalg.eigvalsh(M), 3), s[:3].sum(), rtol=1e-13)


ACCESSORS = ["weights", "components", "scores", "explained_variance", "explained_variance_ratio", "explained_covariance",
             "explained_covariance_ratio", "transform", "stats", "data", "preprocessors", "compute"]


@pytest.mark.parametrize("accessor", ACCESSORS)
def test_compute_false_defers_the_fit_until_a_fitted_quantity_is_read(accessor, monkeypatch):
    """compute=False on chunked views: fit returns at once, and the first read of any fitted quantity -- every accessor,
    `transform`, `stats`, `data`, `preprocessors` -- runs the fit (_deferred.py).  The fit itself is replaced by a stand-in
    that records the call and leaves the fitted state of a two-view, two-mode model, so no GPU is needed."""
    import xeofs_amd as xe
    from xeofs_amd.multi.cca import CCA
    from xeofs_amd.preprocessing import Preprocessor

    n, ps, k = 6, (3, 4), 2
    rng = np.random.default_rng(3)
    views = [xe.DataArray(rng.standard_normal((n, P)).astype(np.float32), ("time", f"x{i}"), chunks=((n,), (P,)))
             for i, P in enumerate(ps)]
    calls = []

    class Mat:                                                                     # the little of a resident matrix the accessors touch
        def __init__(self, X):
            self.n, self.X = X.shape[0], X

        def free(self):
            pass

    def fake_fit_now(self, vs, dim):
        calls.append(dim)
        pres = []
        for v in vs:
            pre = Preprocessor(True, False, False, True)
            pre.sample_dims = ("time",)
            pre.fields = pre._fields(v, pre.sample_dims)
            pre.valid_feature, pre.valid_sample = np.ones(v.shape[1], bool), np.ones(n, bool)
            pres.append(pre)
        self._preprocessors, self.n_views_ = pres, len(vs)
        self.data = dict(input_data=[Mat(v.values) for v in vs], weights=[np.ones((P, k), np.float32) for P in ps],
                         variates=[np.ones((n, k), np.float32) for _ in ps],
                         canonical_loadings=[np.ones((P, k), np.float32) for P in ps],
                         explained_variance=[np.ones(k) for _ in ps], explained_variance_ratio=[np.ones(k) for _ in ps],
                         explained_covariance=np.ones(k), explained_covariance_ratio=np.ones(k))
        self._stats = dict(eig_route="host")
        return self

    monkeypatch.setattr(CCA, "_fit_now", fake_fit_now)
    model = CCA(n_modes=k, compute=False)
    assert model.fit(views, "time") is model
    assert model.is_deferred and calls == []                                       # nothing has run
    if accessor == "transform":
        with pytest.raises(Exception):                                             # (the stand-in has no engine behind it) ...
            model.transform(views)
    elif accessor in ("stats", "data", "preprocessors"):
        assert getattr(model, accessor)
    elif accessor == "components":
        out = model.components(normalize=False)                                    # (normalize=True reads the resident view)
        assert len(out) == 2 and out[1].values.shape == (k, ps[1])
    else:
        out = getattr(model, accessor)()
        if accessor in ("weights", "scores", "explained_variance", "explained_variance_ratio"):
            assert isinstance(out, list) and len(out) == 2
    assert calls == ["time"] and not model.is_deferred                             # ... but the fit ran, once
    model.weights(), model.scores(), model.stats
    assert calls == ["time"]
    # an in-memory input is fitted at once whatever `compute` says
    calls.clear()
    eager = CCA(n_modes=k, compute=False).fit([xe.DataArray(v.values, v.dims) for v in views], "time")
    assert calls == ["time"] and not eager.is_deferred
