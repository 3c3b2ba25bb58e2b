"""Host-side check behind tests/test_gpu_plane_producers.py::test_bound_far_above_the_maximum (no GPU needed).

A plane producer splits the panel with the scale of a BOUND on its maximum, not of the maximum itself.  fp16 is a floating-point
format: the hi term keeps its 11 bits at any scale, only the magnitude below which the lo term turns subnormal moves up, from
2^-38 max |Y| to 2^-38 bound per element.  The numpy emulation of the f16x3 product (tests/test_product_model_host.py: power-of-two
scaling, two-term round-to-nearest split, hi*hi + hi*lo + lo*hi, exact accumulation) run with the bound's scale on the GPU test's
own adversarial inputs -- one entry of the field 2^10 times the rest -- stays inside the product model of
tests/test_gpu_product_routes.py with the bound in place of the maximum, against float64 and against the emulation with the
maximum's scale: the model admits the case, which is what the GPU test then asserts of the kernels."""
import numpy as np
import pytest

import test_gpu_plane_producers as planes
import test_gpu_product_routes as routes
import test_product_model_host as model


def emulate_with_panel_bound(A, B, b_bound):
    sa, sb = model._scale_for(np.abs(A).max()), model._scale_for(b_bound)
    ah, al = model._split(A * np.float32(sa))
    bh, bl = model._split(B * np.float32(sb))
    return (ah.T @ bh + ah.T @ bl + al.T @ bh) / (sa * sb)


@pytest.mark.parametrize("extra_slack", [1.0, 2.0 ** 10])
def test_model_admits_a_bound_far_above_the_maximum(extra_slack):
    n, p, L = 300, 200, 64
    X = planes.field(n, p, seed=11, outlier=True).astype(np.float64)
    Xp = (X - X.mean(0)).astype(np.float32)                                     # the centred float32 matrix
    Q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((n, L)))
    Y = (Xp.astype(np.float64).T @ Q).astype(np.float32)                        # the panel X'^T Z, [p x L]
    bound = float(np.float32(2.0) * np.sqrt(np.float32(n)) * np.abs(Xp).max()) * extra_slack
    true_max = float(np.abs(Y).max())
    slack = bound / true_max
    assert slack >= 2.0 ** 6 and true_max <= bound
    A = np.ascontiguousarray(Xp.T)                                              # W = X' Y = A^T Y with A = X'^T [p x n]
    ref, rel, _ = routes.product_bounds(A, Y, routes.TOL["f16x3"])
    A64, B64 = np.abs(A.astype(np.float64)), np.abs(Y.astype(np.float64))
    absb = 2.0 ** -38 * (A64.max() * B64.sum(0)[None, :] + bound * A64.sum(0)[:, None])
    w_bound, w_max = emulate_with_panel_bound(A, Y, bound), model.emulate_f16x3(A, Y)
    used_ref = float((np.abs(w_bound - ref) / (rel + absb)).max())
    used_max = float((np.abs(w_bound - w_max) / (rel + absb)).max())
    print(f"slack 2^{np.log2(slack):.2f}: |W(bound) - float64| uses {used_ref:.3g} of the model, |W(bound) - W(maximum)| {used_max:.3g}")
    assert used_ref <= 1.0 and used_max <= 1.0
    # the absolute term is what the slack moves: the bound's scale leaves the hi plane's 11 bits alone
    hi_b, _ = model._split(Y * np.float32(model._scale_for(bound)))
    hi_m, _ = model._split(Y * np.float32(model._scale_for(true_max)))
    big = np.abs(Y) >= 2.0 ** -8 * true_max                                     # (entries whose hi term is a normal fp16 at either scale)
    assert np.array_equal((hi_b / model._scale_for(bound))[big], (hi_m / model._scale_for(true_max))[big])
