"""xeofs_amd.single.DINEOF against a float64 restatement of its algorithm with numpy's exact SVD (`restate` below).

The restatement is fed the model's own cross-validation points and its recorded iteration counts, so that a stopping
threshold met a rounding error apart cannot desynchronise the two; run freely (n_iterations=None) it applies the stopping
rule itself.

MEASURED_* below: the largest deviations seen on the MI355X; every tolerance is four times its figure (float32
accumulation over some 80 EM steps has no tight derived bound).  A float32 numpy emulation of the exact-route case gave
1.3e-5 absolute on the filled anomalies (a field of scale 9) and 2e-7 on cv_error -- a sanity anchor, not the limit."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# exact route (16 x 333, 20 % gaps): max |filled anomalies - restatement|, max |cv_error - restatement|,
# max |s - restatement| / s[0], |total_variance - restatement| / total_variance
MEASURED_EXACT = dict(filled=1.49e-5, cv_error=1.36e-7, singular_values=2.9e-8, total_variance=6.1e-9)
# streaming route (96 x 200, 30 % gaps): max |cv_error[k] - restatement| for k <= 4, and |RMSE of filled() at the gaps against
# the withheld truth - the restatement's| / the restatement's (0.0517827 against 0.0517876: the model's was the smaller)
MEASURED_STREAM = dict(cv_error=1.21e-7, gap_rmse_excess=9.5e-5)


def make_field(n, p, gap_fraction, seed):
    """a column-centred rank-3 signal of amplitudes 8 / 4 / 2 (unit-RMS series times unit-variance patterns), per-feature
    offsets, noise 0.05; -> (the complete float32 field, the same with `gap_fraction` of its entries NaN)"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((n, 3))
    t -= t.mean(0)
    t /= np.sqrt((t ** 2).mean(0))
    c = rng.standard_normal((p, 3))
    full = (t * np.array([8.0, 4.0, 2.0])) @ c.T + 3.0 * rng.standard_normal(p) + 0.05 * rng.standard_normal((n, p))
    full = full.astype(np.float32)
    gappy = full.copy()
    gappy[rng.random((n, p)) < gap_fraction] = np.nan
    return full, gappy


def restate(X, cv_index, n_modes, tol=1e-3, max_iter=50, n_iterations=None):
    """DINEOF on the float64 field X [n x p] (NaN = gap; centred per feature over its valid entries), with np.linalg.svd.
    n_iterations: the iteration count of every stage (per k tried, then the final stage) to repeat; None: the stopping rule.
    -> dict(filled (anomalies), mean, cv_error, n_iterations, n_modes_optimal, singular_values, total_variance)"""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    gap = np.isnan(X)
    mean = np.nanmean(X, axis=0)
    F = np.where(gap, 0.0, X - mean)
    sumsq_valid = (F ** 2).sum()
    flat = F.reshape(-1)
    truth = flat[cv_index].copy()
    mask = gap.copy()
    mask.reshape(-1)[cv_index] = True
    flat[cv_index] = 0.0

    def stage(k, rms, iters):
        new2 = 0.0
        for it in range(1, (iters or max_iter) + 1):
            U, s, Vt = np.linalg.svd(F, full_matrices=False)
            rec = (U[:, :k] * s[:k]) @ Vt[:k]
            d2 = ((rec - F)[mask] ** 2).sum()
            F[mask] = rec[mask]
            new2 = (rec[mask] ** 2).sum()
            count = int(mask.sum())
            if iters is None and (count == 0 or np.sqrt(d2 / count) <= tol * rms):
                break
        return it, new2

    rms = np.sqrt((F[~mask] ** 2).mean())
    cv_error, its = [], []
    tried = n_modes if n_iterations is None else len(n_iterations) - 1
    for k in range(1, tried + 1):
        its.append(stage(k, rms, None if n_iterations is None else int(n_iterations[k - 1]))[0])
        cv_error.append(float(np.sqrt(((flat[cv_index] - truth) ** 2).mean())))
        if n_iterations is None and k > 1 and cv_error[-1] > cv_error[-2]:
            break
    kopt = int(np.argmin(cv_error)) + 1
    mask = gap
    flat[cv_index] = truth
    rms = np.sqrt(sumsq_valid / (~gap).sum())
    it, new2 = stage(kopt, rms, None if n_iterations is None else int(n_iterations[-1]))
    its.append(it)
    s = np.linalg.svd(F, compute_uv=False)[:kopt]
    return dict(filled=F, mean=mean, cv_error=np.array(cv_error), n_iterations=np.array(its), n_modes_optimal=kopt,
                singular_values=s, total_variance=(sumsq_valid + new2) / (n - 1))


def _array(values, name="sst"):
    import xeofs_amd as xe

    n, p = values.shape
    return xe.DataArray(values, dims=("time", "x"), coords={"time": np.arange(n), "x": np.arange(p)}, name=name)


@pytest.fixture(autouse=True)
def _ctx(ctx):
    return ctx


EXACT_SEED, STREAM_SEED = 5, 3


@pytest.fixture(scope="module")
def exact_case(ctx):
    import xeofs_amd as xe

    full, gappy = make_field(16, 333, 0.2, EXACT_SEED)
    model = xe.single.DINEOF(n_modes=6, cv_fraction=0.03, tol=1e-3, random_state=1).fit(_array(gappy), "time")
    x64 = gappy.astype(np.float64)
    free = restate(x64, model.data["cv_index"], 6)
    ref = restate(x64, model.data["cv_index"], 6, n_iterations=model.data["n_iterations"])
    return full, gappy, model, free, ref


def test_exact_route_against_restatement(exact_case):
    """Measured on the MI355X (MEASURED_EXACT): filled anomalies 1.49e-5 absolute on a field of scale 9, cv_error 1.36e-7,
    singular values 2.9e-8 of the first, total variance 6.1e-9 relative; both ran 13 / 13 / 12 / 23 / 2 / 2 iterations at
    k = 1 .. 6 and one in the final stage.  The tolerances are four times these."""
    full, gappy, model, free, ref = exact_case
    # the construction converges below max_iter at every k (16-18 iterations for k <= 4, 2 beyond, on the CPU)
    assert np.all(free["n_iterations"] < 50), free["n_iterations"]
    assert np.all(model.data["n_iterations"] < 50), model.data["n_iterations"]
    cv = model.cv_error().values
    assert cv.shape == ref["cv_error"].shape and list(model.cv_error().coords["mode"]) == list(range(1, cv.size + 1))
    assert model.n_modes_optimal == int(np.argmin(cv)) + 1 == ref["n_modes_optimal"]
    assert cv[3] < 0.2 * cv[2]                       # the nan-mean leaves one extra rank: the effective rank is 4
    assert model.n_modes_optimal >= 4
    got = dict(filled=np.abs(model.data["filled_anomalies"].cpu().numpy().astype(np.float64) - ref["filled"]).max(),
               cv_error=np.abs(cv - ref["cv_error"]).max(),
               singular_values=(np.abs(model.singular_values().values - ref["singular_values"]) / ref["singular_values"][0]).max(),
               total_variance=abs(model.data["total_variance"] - ref["total_variance"]) / ref["total_variance"])
    print("DINEOF exact route, deviations from the float64 restatement:", got, "iterations", model.data["n_iterations"],
          "restatement free", free["n_iterations"])
    for key, value in got.items():
        assert value <= 4 * MEASURED_EXACT[key], (key, value)


def test_streaming_route_properties(ctx):
    """Measured on the MI355X (MEASURED_STREAM): cv_error for k <= 4 within 1.21e-7 of the restatement's (at k = 5, a mode
    inside the noise bulk that two warm power iterations do not resolve, 0.05439 against 0.05422 -- not compared); RMSE at the
    gaps 0.0517827 against the restatement's 0.0517876, a relative difference of 9.5e-5.  The tolerances are four times
    these; the margin of the RMSE is 1 + 4 x 9.5e-5."""
    import xeofs_amd as xe

    full, gappy = make_field(96, 200, 0.3, STREAM_SEED)
    model = xe.single.DINEOF(n_modes=6, cv_fraction=0.03, tol=1e-3, random_state=2).fit(_array(gappy), "time")
    assert 6 + 10 < 96                               # the randomized path and the warm start are really used
    ref = restate(gappy.astype(np.float64), model.data["cv_index"], 6, n_iterations=model.data["n_iterations"])
    cv = model.cv_error().values
    assert cv.size >= 4 and model.n_modes_optimal >= 4
    dev = np.abs(cv[:4] - ref["cv_error"][:4]).max()
    gap = np.isnan(gappy)
    rmse = lambda filled: float(np.sqrt(((filled[gap] - full[gap].astype(np.float64)) ** 2).mean()))
    mine, theirs = rmse(model.filled().values.astype(np.float64)), rmse(ref["filled"] + ref["mean"])
    print("DINEOF streaming route: cv_error", cv, "restatement", ref["cv_error"], "max deviation k <= 4", dev,
          "gap RMSE", mine, "restatement", theirs, "iterations", model.data["n_iterations"])
    assert theirs < 0.1                              # the restatement alone reaches about the noise level (0.05)
    assert dev <= 4 * MEASURED_STREAM["cv_error"]
    assert mine <= theirs * (1 + 4 * MEASURED_STREAM["gap_rmse_excess"])


def test_gap_free_input_is_eof(ctx):
    """k* = 4 here: three signal modes and one of the noise bulk, which no fixed count of power iterations converges -- the
    model's last decomposition follows EOF's recipe (sketch, oversampling, iterations), so all four agree."""
    import xeofs_amd as xe

    full, _ = make_field(40, 120, 0.0, 9)
    X = _array(full)
    model = xe.single.DINEOF(n_modes=5, random_state=3).fit(X, "time")
    assert model.data["n_gaps"] == 0 and model.data["n_iterations"][-1] == 1
    k = model.n_modes_optimal
    # only the cross-validation points were ever filled, and they hold their own values again
    assert np.array_equal(model.filled().values, full)
    F = model.data["filled_anomalies"].cpu().numpy()
    assert np.array_equal(F.reshape(-1)[model.data["cv_index"]], model.data["cv_truth"])
    eof = xe.single.EOF(n_modes=k, random_state=3).fit(X, "time")
    s, ref = model.singular_values().values, eof.singular_values().values
    assert np.all(np.abs(s - ref) <= 1e-5 * ref[0]), (s, ref)          # the tolerances of test_gpu_models.py (EOF against the oracle)
    c, cref = model.components().values.reshape(k, -1), eof.components().values.reshape(k, -1)
    print("DINEOF gap-free: k* =", k, "cv_error", model.cv_error().values, "|cos|", [abs(float(np.dot(c[j], cref[j]))) for j in range(k)])
    for j in range(k):
        assert abs(np.dot(c[j], cref[j])) >= 1 - 1e-5, j
    assert abs(model.data["total_variance"] - eof.data["total_variance"]) <= 1e-5 * eof.data["total_variance"]


def test_filled_keeps_valid_values_and_fills_gaps(exact_case):
    full, gappy, model, _, _ = exact_case
    out = model.filled()
    assert out.dims == ("time", "x") and out.values.dtype == gappy.dtype and out.values.shape == gappy.shape
    valid = ~np.isnan(gappy)
    assert np.array_equal(out.values[valid].view(np.int32), gappy[valid].view(np.int32))        # bit for bit
    assert not np.isnan(out.values).any()
    assert np.sqrt(((out.values[~valid] - full[~valid]) ** 2).mean()) < 0.5                     # (noise 0.05, field scale 9)


def test_land_mask_and_missing_sample(ctx):
    import xeofs_amd as xe

    rng = np.random.default_rng(12)
    full, gappy = make_field(30, 8 * 12, 0.15, 12)
    v = gappy.reshape(30, 8, 12).copy()
    land = rng.random((8, 12)) < 0.2
    v[:, land] = np.nan
    v[7] = np.nan
    X = xe.DataArray(v, dims=("time", "lat", "lon"),
                     coords={"time": np.arange(30), "lat": np.linspace(-35, 35, 8), "lon": np.arange(12) * 30.0}, name="sst")
    model = xe.single.DINEOF(n_modes=4, cv_min=20, random_state=0).fit(X, "time")
    out = model.filled().values
    assert np.isnan(out[:, land]).all() and np.isnan(out[7]).all()
    rest = np.ones(30, bool)
    rest[7] = False
    assert not np.isnan(out[rest][:, ~land]).any()
    keep = ~np.isnan(v)
    assert np.array_equal(out[keep], v[keep])
    k = model.n_modes_optimal
    comps, scores = model.components(), model.scores()
    eof_like = xe.single.EOF(n_modes=k).fit(xe.DataArray(out, dims=X.dims, coords=X.coords), "time")
    assert comps.dims == eof_like.components().dims == ("mode", "lat", "lon") and comps.shape == (k, 8, 12)
    assert list(comps.coords["mode"]) == list(eof_like.components().coords["mode"])
    assert np.isnan(comps.values[:, land]).all() and not np.isnan(comps.values[:, ~land]).any()
    assert scores.dims == ("mode", "time") and np.isnan(scores.values[:, 7]).all() and not np.isnan(scores.values[:, rest]).any()


def test_standardize_and_coslat_statistics(ctx):
    import xeofs_amd as xe
    from xeofs_amd.preprocessing import Preprocessor

    full, gappy = make_field(30, 8 * 12, 0.15, 13)
    coords = {"time": np.arange(30), "lat": np.linspace(-70, 70, 8), "lon": np.arange(12) * 30.0}
    dims = ("time", "lat", "lon")
    model = xe.single.DINEOF(n_modes=3, standardize=True, use_coslat=True, cv_min=20, random_state=0)
    model.fit(xe.DataArray(gappy.reshape(30, 8, 12), dims=dims, coords=coords), "time")
    assert not np.isnan(model.filled().values).any() and model.n_modes_optimal >= 1
    # on a gap-free field the statistics are the Preprocessor's
    X = xe.DataArray(full.reshape(30, 8, 12), dims=dims, coords=coords)
    model = xe.single.DINEOF(n_modes=3, standardize=True, use_coslat=True, cv_min=20, random_state=0).fit(X, "time")
    pre = Preprocessor(True, True, True, ctx=ctx)
    pre.fit_transform(X, "time").free()
    mine = model.preprocessor
    # Both are float64 statistics of the same float32 entries.  The Preprocessor's (one pass of sums about a sample c of the
    # feature, tests/test_gpu_preprocess_routes.py) err by (k + 2) u mean|x - c| + 2 u |mean| in the mean and by
    # 3 (k + 2) u sum (x - c)^2 in M2 -- at most ten times M2 with c within three deviations of the mean, half of that
    # relative in the deviation; the reductions here sum k terms as well.  Four and two times those: the two sides, MARGIN 2.
    k, u = 30, 2.0 ** -53
    np.testing.assert_allclose(mine.mean_, pre.mean_, rtol=0, atol=8 * (k + 2) * u * np.abs(full).max())
    np.testing.assert_allclose(mine.std_, pre.std_, rtol=64 * (k + 2) * u)
    np.testing.assert_allclose(mine.feature_weights, pre.feature_weights, rtol=0, atol=0)
    assert np.array_equal(mine.valid_feature, pre.valid_feature) and np.array_equal(mine.valid_sample, pre.valid_sample)


def test_rotator_and_transform(exact_case):
    import xeofs_amd as xe

    full, gappy, model, _, _ = exact_case
    rot = xe.single.EOFRotator(n_modes=3).fit(model)
    assert rot.components().shape == (3, 333) and not np.isnan(rot.components().values).any()
    # transform keeps EOF's behaviour: complete new data are projected, isolated NaNs raise EOF's error
    sc = model.transform(_array(full))
    assert sc.shape == (model.n_modes_optimal, 16) and not np.isnan(sc.values).any()
    eof = xe.single.EOF(n_modes=3).fit(_array(full), "time")
    with pytest.raises(ValueError) as theirs:
        eof.transform(_array(gappy))
    with pytest.raises(ValueError) as mine:
        model.transform(_array(gappy))
    assert str(mine.value) == str(theirs.value)
