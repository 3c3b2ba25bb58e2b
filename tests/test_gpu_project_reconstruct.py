"""`engine.project` (eofx_project_f32) and `engine.reconstruct` (eofx_reconstruct_f32, reconstruct_kernel), the two entries
every model runs after its fit, per element against float64.

reconstruct   out = S V^T in float32, k summed in chunks of 64 with a partial last chunk, 64 x 64 output tiles zero-filled
              at the n and p edges.  Against the float64 product of the float32 inputs:
              |err| <= (k + 1) 2^-24 sum_j |S_ij| |V_cj| + k 2^-149  (k products and k additions of one float32 rounding
              each, any order, plus underflow).  Shapes below, at and above one tile in both directions, mode counts around
              the chunk.  The mixed signs of S and V keep the bound far below the entries' scale.
project       scatter_rows (masked in-place matrices) -> import into a round_up(k, 32)-wide panel -> panel_mul at the
              context's final precision -> export.  Matrices come from `engine.preprocess` in the layouts of
              tests/test_gpu_product_routes.py (written, in place, masked in place; its field generator, its TOL and its
              `_check`), reference: the float64 product of the float32 matrix the engine holds.
Each case prints its worst error / bound.
"""

import numpy as np
import pytest

from test_gpu_product_routes import TOL, _check, _layout_field, product_bounds

pytestmark = pytest.mark.gpu

REC_SHAPES = [(1, 1), (63, 65), (64, 64), (65, 130), (130, 63), (3, 700)]
REC_MODES = [1, 10, 64, 65, 128, 200]


def _rec_check(ctx, S, V, what):
    from xeofs_amd import engine

    n, k = S.shape
    p = V.shape[0]
    got = engine.reconstruct(ctx, S, V)
    assert got.shape == (n, p) and got.dtype == np.float32
    assert np.isfinite(got).all(), f"{what}: elements unwritten or not finite"
    S64, V64 = S.astype(np.float64), V.astype(np.float64)
    ref = S64 @ V64.T
    bound = (k + 1) * 2.0 ** -24 * (np.abs(S64) @ np.abs(V64).T) + k * 2.0 ** -149
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / bound).max())
    print(f"REC {what} n={n} p={p} k={k} max(err/bound)={ratio:.3g}")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{what}: {len(bad)} elements outside the bound, first at {bad[0]}, worst ratio {ratio:.3g}"
    return ref, bound


@pytest.mark.parametrize("k", REC_MODES)
@pytest.mark.parametrize("n,p", REC_SHAPES)
def test_reconstruct_every_tile_edge_and_chunk(ctx, n, p, k):
    rng = np.random.default_rng(1000 * n + 10 * p + k)
    S = rng.standard_normal((n, k)).astype(np.float32)
    V = rng.standard_normal((p, k)).astype(np.float32)
    ref, bound = _rec_check(ctx, S, V, "gauss")
    if k >= 10 and n * p >= 64:
        assert np.median(bound) < 1e-4 * np.abs(ref).max()          # mixed signs: the bound is far below the entries' scale


def test_reconstruct_decaying_modes(ctx):
    """mode scales falling from 1 to 1e-6 over 65 modes, and two samples that load on the last mode only.  Without the second
    k-chunk (the one mode past 64) every element would still be within 1e-5 of the largest entry -- what the only earlier
    assertion on this kernel asked -- but those two rows would be wrong by all they hold."""
    n, p, k = 65, 130, 65
    rng = np.random.default_rng(5)
    scale = 10.0 ** (-6.0 * np.arange(k) / (k - 1))
    S = (rng.standard_normal((n, k)) * scale).astype(np.float32)
    V = rng.standard_normal((p, k)).astype(np.float32)
    S[[7, 64], :64] = 0.0
    ref, bound = _rec_check(ctx, S, V, "decay")
    lost = S[:, :64].astype(np.float64) @ V[:, :64].astype(np.float64).T
    assert np.abs(lost - ref).max() <= 1e-5 * np.abs(ref).max()      # the design of the case, not the kernel
    assert (np.abs(lost - ref) > bound)[[7, 64]].all()


def test_reconstruct_mismatched_modes(ctx):
    from xeofs_amd import engine

    with pytest.raises(ValueError, match="do not have the same number of modes"):
        engine.reconstruct(ctx, np.ones((5, 3), np.float32), np.ones((7, 4), np.float32))
    with pytest.raises(ValueError, match="do not have the same number of modes"):
        engine.reconstruct(ctx, np.ones(5, np.float32), np.ones((7, 1), np.float32))


# ----------------------------------------------------------------------------------------------------------------------
PROJ_SHAPES = [(301, 900), (29, 44)]
PROJ_MODES = [1, 31, 32, 33, 64, 100]


def _field(n, P, masked):
    """the field of test_gpu_product_routes._layout_field; its mask is laid out for hundreds of features, so the 44-feature
    field gets one of its own by the same rules: whole runs and isolated points, the valid features at least 0.6 of all and
    more than the samples"""
    if P >= 400:
        return _layout_field(n, P, masked, seed=n + P)
    X, w = _layout_field(n, P, False, seed=n + P)
    if masked:
        X[:, [3, 4, 5, 6, 17, 30, 42, 43]] = np.nan
    return X, w


@pytest.mark.parametrize("n,P", PROJ_SHAPES)
@pytest.mark.parametrize("layout", ["written", "in_place", "masked"])
def test_project_every_layout_and_width(ctx, layout, n, P):
    """k below, at and above the 32-column panel width and the 64-column tile, on a written matrix, an in-place one and a
    masked in-place one (V scattered to the physical features first)"""
    import torch
    from xeofs_amd import engine

    masked = layout == "masked"
    X, w = _field(n, P, masked)
    m2, st2 = engine.preprocess(ctx, X, True, True, w)                       # the compacted two-layout matrix
    mat, st = engine.preprocess(ctx, X, True, True, w, in_place=layout != "written", allow_masked=masked)
    assert mat.masked == masked
    if layout != "written":
        assert mat.layout() == (False, True)
    valid = st2["valid_feature"]
    assert (not masked and valid.all()) or (masked and 0.6 * P <= valid.sum() < P and valid.sum() > n)
    assert mat.p == m2.p == int(valid.sum()) and mat.n == n
    Xh = mat.download() if layout == "written" else m2.download()          # (bitwise the same matrix: test_in_place_mode)
    tol = TOL[ctx.precision[1]]
    rng = np.random.default_rng(n + P)
    for k in PROJ_MODES:
        V = rng.standard_normal((mat.p, k)).astype(np.float32)
        got = engine.project(ctx, mat, V)
        assert got.shape == (n, k) and got.dtype == np.float32
        ref, rel, _ = product_bounds(np.ascontiguousarray(Xh.T), V, tol)
        _check(torch.from_numpy(got), ref, rel, n, f"project {layout} {n}x{P} k={k}")
        if masked:
            twin = engine.project(ctx, m2, V)
            assert (np.abs(got.astype(np.float64) - twin) <= 2 * rel + 1e-300).all(), "masked and compacted projections differ"
        # up to 64 modes the projection streams the field where it lies; a 128-wide panel (k = 100) lets an unmasked
        # in-place matrix build its sample-contiguous layout first (panel_mul's rule for wide panels), a masked one never does
        if layout == "masked" or (layout == "in_place" and k <= 64):
            assert not mat.has_sample_layout()
    for bad in (mat.p + 1, mat.p - 1):
        with pytest.raises(ValueError, match="a different NaN pattern in the new data"):
            engine.project(ctx, mat, np.ones((bad, 3), np.float32))
    if masked:
        with pytest.raises(ValueError, match="a different NaN pattern in the new data"):
            engine.project(ctx, mat, np.ones((P, 3), np.float32))      # the physical feature count is not the matrix's
    mat.free()
    m2.free()
