"""tests/rotation_reference.py (the extended-precision rotation step and its error bound, the reference of
tests/test_gpu_rot_step.py) checked without a GPU:

  * modes 2 / 3 on a packed [Re | Im] panel against the complex128 formulas X^H (b (|b|^2 - aux)) and
    b^H ((b / aux) (|b| / aux)^(power - 1)), through `cpanel.embed` and `cpanel.block`, and against the complex long-double
    twin `crot_step_ref`;
  * modes 0 / 1 against one iteration of the oracle's varimax and promax loops;
  * for every case of the GPU test: the bound is finite, and a float64 numpy evaluation of the same formulas stays inside
    MARGIN * B of the long-double result -- the reference alone keeps to its own bound.

Tolerances: the float64 evaluations are held to the derived bound itself (`rotation_reference` docstring); the oracle
comparison goes through an m x m SVD and inverses of well-conditioned matrices, 1e-9 relative to the largest entry.
"""
import numpy as np
import pytest

import rotation_reference as rref
from oracle import eof_oracle as orc
from xeofs_amd import cpanel

needs_extended = pytest.mark.skipif(not rref.EXTENDED, reason="long double is float64 on this platform")


def _f64_step(c):
    """the same formulas in plain float64 numpy"""
    X, R, aux, mode, power = c["X"].astype(np.float64), c["R"], c["aux"], c["mode"], c["power"]
    b = X @ R
    if mode == 0:
        return X.T @ (b * (b * b - aux))
    if mode == 1:
        z = b / aux
        return b.T @ (z * np.abs(z) ** (power - 1))
    a2 = b * b + np.roll(b * b, c["half"], axis=1)
    if mode == 2:
        return X.T @ (b * (a2 - aux))
    return b.T @ ((b / aux) * (np.sqrt(a2) / aux) ** (power - 1))


def test_case_list_covers_the_issue():
    """every width, mode, column count, small row count and power; the row counts past the launchers' caps"""
    C = rref.CASES
    assert len(set(C)) == len(C)
    assert {(c[0], c[1]) for c in C} == {(L, md) for md in range(4) for L in (32, 64, 128, 256) if md < 2 or L >= 64}
    for L, mode in {(c[0], c[1]) for c in C}:
        mine = [c for c in C if c[0] == L and c[1] == mode]
        ms = {2, L - 1, L} if mode < 2 else {2, L // 2 - 1, L // 2}
        powers = {1, 2, 3, 4} if mode & 1 else {1}
        assert {(c[2], c[3], c[4]) for c in mine if not c[5] and c[3] < 100} == {(m, r, p) for m in ms for r in (1, 31, 32, 33)
                                                                             for p in powers}
        assert any(c[3] == rref.rows_past_cap(L) for c in mine)
    assert [rref.rows_past_cap(L) for L in (32, 64, 128, 256)] == [16416, 16416, 8224, 2080]
    assert rref.n_partials(16416, 64) == 512 and rref.n_partials(8224, 128) == 256 and rref.n_partials(2080, 256) == 64
    assert rref.n_partials(33, 64) == 2 and rref.n_partials(1, 256) == 1
    assert any(c[5] for c in C)


def test_case_inputs_follow_the_padding_rule():
    for case in rref.CASES:
        L, mode, m, rows, power, spread = case
        c = rref.case_inputs(case)
        X, R, aux = c["X"], c["R"], c["aux"]
        assert X.dtype == np.float32 and X.shape == (rows, L) and R.shape == (L, L) and aux.shape == (L,)
        live = ~rref.padding_mask(L, mode, m).all(0)
        assert live.sum() == (m if mode < 2 else 2 * m)
        assert not X[:, ~live].any() and not R[~live].any() and not R[:, ~live].any()
        assert (aux[~live] == (1.0 if mode & 1 else 0.0)).all() and (aux[live] > 0).all()
        if rows >= 31:
            assert np.count_nonzero(~X.any(1)) == 2
        if mode >= 2:
            assert np.array_equal(R, cpanel.embed(c["Rc"], c["half"]))
            assert np.array_equal(X, cpanel.pack(rref.unpack(X, m, c["half"]), c["half"]))
            assert np.abs(c["Rc"].conj().T @ c["Rc"] - np.eye(m)).max() < 1e-13
        else:
            assert np.abs(R[:m, :m].T @ R[:m, :m] - np.eye(m)).max() < 1e-13
        if spread:
            s = np.abs(X).max(0)[:m]
            assert s.max() / s.min() > 1e5


@needs_extended
@pytest.mark.parametrize("case", rref.CASES, ids=rref.case_id)
def test_bound_covers_float64_numpy(case):
    """B is finite, non-negative, an exact zero on the padding, and covers a float64 evaluation of the same formulas"""
    c = rref.case_inputs(case)
    G, B = rref.case_reference(case)
    L, mode, m = case[:3]
    assert np.isfinite(G.astype(np.float64)).all() and np.isfinite(B.astype(np.float64)).all() and (B >= 0).all()
    pad = rref.padding_mask(L, mode, m)
    assert not G[pad].any() and not B[pad].any()
    assert G[~pad].any()
    got = _f64_step(c)
    err = np.abs(got.astype(rref.LD) - G)
    lim = rref.MARGIN * B + rref.TINY
    assert (err <= lim).all(), float((err / lim).max())
    # the bound is tight enough to see an error of order 1 in a single entry's terms: far below the entries' own scale
    scale = np.abs(G).max()
    assert float(B.max()) < 1e-9 * float(scale)


@needs_extended
@pytest.mark.parametrize("case", [c for c in rref.CASES if c[1] >= 2], ids=rref.case_id)
def test_complex_modes_equal_complex128(case):
    c = rref.case_inputs(case)
    L, mode, m = case[:3]
    half, power = c["half"], c["power"]
    G, B = rref.case_reference(case)
    Z = rref.unpack(c["X"], m, half)
    b = Z @ c["Rc"]
    a = np.abs(b)
    ref = Z.conj().T @ (b * (a * a - c["auxh"])) if mode == 2 else b.conj().T @ ((b / c["auxh"]) * (a / c["auxh"]) ** (power - 1))
    got = cpanel.block(G.astype(np.float64), m, half)
    bre, bim = rref.block_sum(B.astype(np.float64), m, half)
    # (+ one float64 rounding of each of the four blocks, taken when G is rounded for cpanel.block)
    Ga = np.abs(G.astype(np.float64))
    rre, rim = rref.block_sum(Ga, m, half)
    assert (np.abs(got.real - ref.real) <= rref.MARGIN * bre + rref.U * rre + rref.TINY).all()
    assert (np.abs(got.imag - ref.imag) <= rref.MARGIN * bim + rref.U * rim + rref.TINY).all()
    # the complex long-double twin agrees to long-double rounding
    twin = rref.crot_step_ref(Z, c["Rc"], c["auxh"], mode, power)
    Gr, Gi = G[:m, :m] + G[half:half + m, half:half + m], G[:m, half:half + m] - G[half:half + m, :m]
    tol = 2.0 ** -60 * (case[3] + L) * float(Ga.max()) * 4
    assert float(np.abs(twin.real - Gr).max()) <= tol and float(np.abs(twin.imag - Gi).max()) <= tol


def _loadings(seed, p, m):
    rng = np.random.default_rng(seed)
    S = 0.1 * rng.standard_normal((p, m))
    S[np.arange(p), rng.integers(0, m, p)] += rng.uniform(1, 3, p)
    return S @ np.diag(np.linspace(2, 1, m)) @ np.linalg.qr(rng.standard_normal((m, m)))[0]


@pytest.mark.parametrize("p,m,power", [(300, 5, 2), (900, 12, 4), (200, 3, 3)])
def test_real_modes_reproduce_one_oracle_iteration(p, m, power):
    """mode 0 with R = I is the `transformed` of the oracle's first varimax iteration; mode 1 on the re-normalised varimax
    solution is the X^H P of its promax regression.  rtol = 2 ends the oracle's loop after that one iteration."""
    X = _loadings(p + m, p, m)
    eps = np.finfo(np.float64).eps
    h = np.sqrt((X * X).sum(1))
    Xn = X / (h + eps)[:, None]
    W = (Xn * Xn).sum(0)
    G0, B0 = rref.rot_step_ref(Xn, np.eye(m), W / p, 0)
    Uu, sv, VT = np.linalg.svd(G0.astype(np.float64))
    R1 = Uu @ VT
    Xv, Rv = orc.varimax(X, max_iter=1, rtol=2.0)
    assert np.abs(R1 - Rv).max() < 1e-9
    assert np.isfinite(B0.astype(np.float64)).all()
    Xo, Ro, phio = orc.promax(X, power=power, max_iter=1, rtol=2.0)
    h2 = np.sqrt((Xv * Xv).sum(1))
    Xp = Xv / (h2 + eps)[:, None]
    G1, B1 = rref.rot_step_ref(Xp, np.eye(m), np.abs(Xp).max(0), 1, power)
    Lm = np.linalg.inv(Xp.T @ Xp) @ G1.astype(np.float64)
    Lm = Lm @ np.sqrt(np.diag(np.diag(np.linalg.inv(Lm.T @ Lm))))
    Li = np.linalg.inv(Lm)
    assert np.abs(Rv @ Lm - Ro).max() < 1e-9 * np.abs(Ro).max()
    assert np.abs(Li @ Li.T - phio).max() < 1e-9 * np.abs(phio).max()
    assert np.abs(h2[:, None] * (Xp @ Lm) - Xo).max() < 1e-9 * np.abs(Xo).max()


def test_argument_checks():
    X, R = np.zeros((3, 4), np.float32), np.eye(4)
    with pytest.raises(ValueError):
        rref.rot_step_ref(X, R, np.ones(4), 4)
    with pytest.raises(ValueError):
        rref.rot_step_ref(X, np.eye(3), np.ones(4), 0)
    with pytest.raises(ValueError):
        rref.crot_step_ref(X[:, :2], np.eye(2), np.ones(2), 1)
