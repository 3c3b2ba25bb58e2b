"""GPU tests of sparse PCA by variable projection (csrc/eofx_spca.hpp, xeofs_amd.spca, xeofs_amd.single.SparsePCA).

The checker is a float64 numpy restatement of the algorithm (Erichson et al. 2020, variable projection) written from its
equations: the thin SVD C = U D V^T, B = A = V[:, :k], alpha, beta scaled by D_0^2, nu = 1 / (D_0^2 + beta), kappa = nu
alpha, then per iteration Z = V D^2 V^T B, A = polar(Z), G = V D^2 V^T (A - B) - beta B, B = prox(B + nu G, kappa) and the
objective 1/2 |D V^T (I - B A^T)|^2 + alpha |B|_1 + beta/2 |B|^2.  Solver-level tests feed the SAME float64 C to both;
model-level tests feed the restatement the engine's own preprocessed matrix (promoted to float64) and the same sketch.
Results are compared up to one sign per mode (the engine signs V by its deterministic rule).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMMA = 0.1


# ------------------------------------------------------------------------------------------------ the restatement
def prox(x, reg, kappa):
    if reg == "l0":
        return np.where(x ** 2 < 2 * kappa, 0.0, x)
    return np.sign(x) * np.maximum(np.abs(x) - kappa, 0.0)


def polar(Z):
    U, s, Wt = np.linalg.svd(Z, full_matrices=False)
    return U @ Wt, s


def restate_spca(C, k, alpha=1e-3, beta=1e-3, reg="l1", max_iter=500, tol=1e-6, check=True, robust=False):
    C = np.asarray(C, np.float64)
    _, D, Vt = np.linalg.svd(C, full_matrices=False)
    V = Vt.T
    B = V[:, :k].copy()
    d0 = D[0] ** 2
    a2, b2 = alpha * d0, beta * d0
    nu = 1.0 / (d0 + b2)
    kappa = nu * a2
    S = np.zeros_like(C)
    obj = []
    for it in range(max_iter):
        if robust:
            XS = C - S
            XB = C @ B
            A, dt = polar(XS.T @ XB)
            R = XS - XB @ A.T
            G = C.T @ (R @ A) - b2 * B
        else:
            A, dt = polar((V * D ** 2) @ (Vt @ B))
            G = (V * D ** 2) @ (Vt @ (A - B)) - b2 * B
        B = prox(B + nu * G, reg, kappa)
        if robust:
            R = C - C @ B @ A.T
            S = prox(R, "l1", GAMMA)
            R = R - S
        else:
            R = (Vt.T * D).T - (Vt.T * D).T @ B @ A.T
        o = 0.5 * np.sum(R ** 2) + a2 * np.sum(np.abs(B)) + 0.5 * b2 * np.sum(B ** 2)
        if robust:
            o += GAMMA * np.sum(np.abs(S))
        obj.append(o)
        if check and it > 0 and abs(obj[-2] - obj[-1]) / obj[-1] < tol:
            break
    return dict(B=B, A=A, dtilde=dt, objective=np.array(obj), n_iter=len(obj), kappa=kappa, nu=nu)


def orth(Y):
    return np.linalg.qr(Y, mode="reduced")[0]


def restate_qb(X, l, n_subspace, omega):
    Q = orth(X @ omega)
    for _ in range(n_subspace):
        Z = orth(X.T @ Q)
        Q = orth(X @ Z)
    return Q.T @ X


def restate_rqb(X, l, n_subspace, n_blocks, omega):
    if n_blocks <= 1:
        return restate_qb(X, l, n_subspace, omega)
    K = [restate_qb(X[rows], l, n_subspace, omega) for rows in np.array_split(np.arange(X.shape[0]), n_blocks)]
    return restate_qb(np.concatenate(K, axis=0), l, n_subspace, omega)


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def ctx():
    from xeofs_amd import engine

    return engine.default_context()


def planted(m, p, rank=3, seed=0, noise=0.05):
    """m x p: a sparse rank-`rank` signal (each loading nonzero on a tenth of the columns) plus noise"""
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((p, rank)) * (rng.random((p, rank)) < 0.1)
    F = rng.standard_normal((m, rank)) * np.array([10.0, 6.0, 3.0][:rank])
    return F @ L.T + noise * rng.standard_normal((m, p))


def mode_signs(Be, Br):
    s = np.sign(np.sum(Be * Br, axis=0))
    return np.where(s == 0, 1.0, s)


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def solve(ctx, C, k, **kw):
    from xeofs_amd import spca

    Ct = spca._dev64(ctx, np.ascontiguousarray(np.asarray(C, np.float64).T))
    out = spca.spca_solve(ctx, Ct, k, **kw)
    return dict(out, B=out["B"].cpu().numpy(), A=out["A"].cpu().numpy())


def check_solver_parity(got, ref, tol=1e-9, obj_tol=1e-10):
    assert got["n_iter"] == ref["n_iter"], (got["n_iter"], ref["n_iter"])
    assert rel(got["objective"], ref["objective"]) <= obj_tol, rel(got["objective"], ref["objective"])
    s = mode_signs(got["B"], ref["B"])
    assert rel(got["B"] * s, ref["B"]) <= tol, rel(got["B"] * s, ref["B"])
    # A is unique on the modes whose B column is not zero; a zero column's completion is the engine's own (deviation 2):
    # there A only has to stay orthonormal
    live = np.any(ref["B"] != 0, axis=0)
    assert rel(got["A"][:, live] * s[live], ref["A"][:, live]) <= tol, rel(got["A"][:, live] * s[live], ref["A"][:, live])
    np.testing.assert_allclose(got["A"].T @ got["A"], np.eye(got["A"].shape[1]), atol=1e-12)
    assert rel(got["dtilde"], ref["dtilde"]) <= tol
    zero_e, zero_r = got["B"] == 0, ref["B"] == 0
    differ = zero_e != zero_r
    if differ.any():       # only entries whose pre-threshold value lies within 1e-8 of the threshold may differ
        assert differ.sum() <= 2, differ.sum()
        vals = np.abs(np.where(zero_e, ref["B"], got["B"] * s))[differ]
        assert np.all(vals <= 1e-8 * max(1.0, np.abs(ref["B"]).max())), vals


# ------------------------------------------------------------------------------------------------ solver level
@pytest.mark.parametrize("p, reg, check", [(300, "l1", True), (5000, "l1", True), (200000, "l1", True), (5000, "l0", True),
                                           (3000, "l1", False), (3000, "l0", False)])
def test_solver_parity(ctx, p, reg, check):
    C = planted(20, p, seed=p)
    kw = dict(alpha=1e-3 if reg == "l1" else 1e-4, beta=1e-3, regularizer=reg, max_iter=200 if check else 40, tol=1e-6,
              check=check)
    got = solve(ctx, C, 5, **kw)
    ref = restate_spca(C, 5, kw["alpha"], kw["beta"], reg, kw["max_iter"], kw["tol"], check)
    assert got["route"] == "kernel"
    if not check:
        assert got["n_iter"] == kw["max_iter"]
    check_solver_parity(got, ref)
    assert (got["B"] == 0).any() and (got["B"] != 0).any()      # the planted loadings are sparse, so is B


def test_solver_general_route(ctx):
    """more singular vectors than the loop kernels take (the exact route on a wide-enough matrix)"""
    C = planted(140, 400, seed=3)
    got = solve(ctx, C, 4, max_iter=60)
    ref = restate_spca(C, 4, max_iter=60)
    assert got["route"] == "general"
    check_solver_parity(got, ref)


@pytest.mark.parametrize("check", [True, False])
def test_solver_robust(ctx, check):
    C = planted(20, 300, seed=5)
    C[3, 17] += 40.0                                            # a gross outlier for S to take
    got = solve(ctx, C, 3, robust=True, max_iter=25, check=check)
    ref = restate_spca(C, 3, max_iter=25, check=check, robust=True)
    assert got["route"] == "robust"
    check_solver_parity(got, ref, tol=1e-8, obj_tol=1e-10)


def test_solver_argument_errors(ctx):
    from xeofs_amd import spca

    C = planted(20, 300)
    with pytest.raises(ValueError):
        solve(ctx, C, 301)
    with pytest.raises(ValueError):
        solve(ctx, C, 3, regularizer="l2")
    with pytest.raises(NotImplementedError):
        solve(ctx, C, 3, robust=True, regularizer="l0")
    with pytest.raises(ValueError, match="finite"):             # the engine's EOFX_ERR_ARG
        solve(ctx, C, 3, alpha=float("nan"))
    with pytest.raises(ValueError, match="max_iter"):
        solve(ctx, C, 3, max_iter=0)
    assert spca.SPCA_KMAX == 64 and spca.SPCA_LMAX == 128


def test_solver_bitwise_repeatable(ctx):
    C = planted(20, 50000, seed=9)
    a, b = solve(ctx, C, 5, max_iter=60), solve(ctx, C, 5, max_iter=60)
    assert np.array_equal(a["B"], b["B"]) and np.array_equal(a["A"], b["A"])
    assert np.array_equal(a["objective"], b["objective"])


# ------------------------------------------------------------------------------------------------ model level
def field(n=60, p=500, seed=0, nan_cols=()):
    from xeofs_amd import labelled

    X = planted(n, p, seed=seed, noise=0.1).astype(np.float32)
    X[:, list(nan_cols)] = np.nan
    return labelled.DataArray(X, ("time", "x"), {"time": np.arange(n), "x": np.arange(p)})


def engine_matrix(model):
    return model.data["input_data"].download().astype(np.float64)


# The engine's QB products are float32 (f32 MFMA, relative error ~1e-6 per product); the variable-projection loop then
# runs in float64 on a C that differs from the restatement's float64 C at that level.  With a fixed iteration count
# (compute=False) the soft-thresholding map is Lipschitz, so B, A and the explained variance stay within ~1e-4 of the
# restatement's (the bound below, relative to the largest entry); entries near the threshold may switch between 0 and a
# value of that size.
MODEL_TOL = 2e-4


@pytest.mark.parametrize("n_subspace, n_blocks", [(0, 1), (2, 1), (1, 2)])
def test_model_randomized_route(n_subspace, n_blocks):
    from xeofs_amd import engine
    from xeofs_amd.single import SparsePCA

    k, over, seed = 3, 10, 7
    m = SparsePCA(n_modes=k, n_subspace=n_subspace, n_blocks=n_blocks, random_state=seed, compute=False, max_iter=60)
    m.fit(field(), "time")
    assert m.stats["route"] == "randomized" and m.stats["n_iter"] == 60
    X = engine_matrix(m)
    omega = engine.sketch_matrix(X.shape[1], k + over, seed).astype(np.float64)
    Cq = restate_rqb(X, k + over, n_subspace, n_blocks, omega)
    assert m.stats["rows_compressed"] == Cq.shape[0]
    ref = restate_spca(Cq, k, max_iter=60, check=False)
    s = mode_signs(m.data["components"], ref["B"])
    assert rel(m.data["components"] * s, ref["B"]) <= MODEL_TOL
    assert rel(m.data["components_normal"] * s, ref["A"]) <= MODEL_TOL
    n = X.shape[0]
    ev = ref["dtilde"] / (Cq.shape[0] - 1) * (k + over - 1) / (n - 1)
    assert rel(m.data["explained_variance"], ev) <= MODEL_TOL
    np.testing.assert_allclose(m.data["scores"] * s, X @ ref["B"], atol=MODEL_TOL * np.abs(X @ ref["B"]).max())


def test_model_exact_route():
    from xeofs_amd.single import SparsePCA

    k = 25
    m = SparsePCA(n_modes=k, max_iter=80)              # auto: max(40, 30) < 500 and 25 > int(0.8 * 30)
    m.fit(field(40, 30, seed=2), "time")
    assert m.stats["route"] == "exact"
    X = engine_matrix(m)
    ref = restate_spca(X, k, max_iter=80)
    assert abs(m.stats["n_iter"] - ref["n_iter"]) <= 2
    if m.stats["n_iter"] == ref["n_iter"]:
        s = mode_signs(m.data["components"], ref["B"])
        assert rel(m.data["components"] * s, ref["B"]) <= MODEL_TOL
    assert rel(m.data["explained_variance"], ref["dtilde"] / (X.shape[0] - 1)) <= MODEL_TOL


# ------------------------------------------------------------------------------------------------ behaviour
def test_masked_features_give_nan_components():
    from xeofs_amd import labelled
    from xeofs_amd.single import SparsePCA

    m = SparsePCA(n_modes=2, random_state=1).fit(field(nan_cols=(3, 40, 41)), "time")
    comps = labelled.unpack(m.components())[0]
    assert comps.shape == (2, 500)
    assert np.all(np.isnan(comps[:, [3, 40, 41]]))
    assert np.isfinite(np.delete(comps, [3, 40, 41], axis=1)).all()


def test_dataset_and_list_inputs():
    from xeofs_amd import labelled
    from xeofs_amd.single import SparsePCA

    a, b = field(seed=1), field(seed=2)
    ds = labelled.Dataset({"a": a, "b": b})
    out = SparsePCA(n_modes=2, random_state=0).fit(ds, "time").components()
    assert labelled.is_dataset(out) and set(out.data_vars) == {"a", "b"}
    out = SparsePCA(n_modes=2, random_state=0).fit([a, b], "time").components()
    assert isinstance(out, list) and len(out) == 2


def test_transform_and_inverse_transform():
    from xeofs_amd import labelled
    from xeofs_amd.single import SparsePCA

    X = field(seed=4)
    m = SparsePCA(n_modes=3, random_state=0).fit(X, "time")
    sc = labelled.unpack(m.scores())[0]
    tr = labelled.unpack(m.transform(X))[0]
    np.testing.assert_allclose(tr, sc, rtol=1e-5, atol=1e-5 * np.abs(sc).max())
    pre = m.preprocessor
    A = m.data["components_normal"].astype(np.float64)
    for normalized in (False, True):
        scores = m.scores(normalized=normalized)
        rec = labelled.unpack(m.inverse_transform(scores, normalized=normalized))[0]
        expect = m.data["scores"].astype(np.float64) @ A.T + pre.mean_
        np.testing.assert_allclose(rec, expect, rtol=1e-4, atol=1e-4 * np.abs(expect).max())


def test_large_alpha_zeroes_components():
    from xeofs_amd.single import SparsePCA

    m = SparsePCA(n_modes=3, alpha=10.0, random_state=0).fit(field(seed=5), "time")
    assert np.all(m.data["components"] == 0)
    assert np.all(m.data["explained_variance"] == 0)
    A = m.data["components_normal"].astype(np.float64)
    np.testing.assert_allclose(A.T @ A, np.eye(3), atol=1e-6)


def test_compute_false_runs_max_iter():
    from xeofs_amd.single import SparsePCA

    m = SparsePCA(n_modes=2, max_iter=37, tol=1e-2, compute=False, random_state=0).fit(field(seed=6), "time")
    assert m.stats["n_iter"] == 37 and len(m.stats["objective"]) == 37
    m2 = SparsePCA(n_modes=2, max_iter=37, tol=1e-2, random_state=0).fit(field(seed=6), "time")
    assert m2.stats["n_iter"] < 37


def test_two_fits_bitwise_equal():
    from xeofs_amd.single import SparsePCA

    X = field(seed=8)
    a = SparsePCA(n_modes=3, random_state=11).fit(X, "time")
    b = SparsePCA(n_modes=3, random_state=11).fit(X, "time")
    for key in ("components", "components_normal", "scores", "explained_variance"):
        assert np.array_equal(a.data[key], b.data[key]), key
