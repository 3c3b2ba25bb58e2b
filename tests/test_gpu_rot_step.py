"""`eofx_panel_rot_step_f64` (rot_step_kernel, rot_step_wide_kernel<128>, <256>; modes 0 .. 3) and
`eofx_panel_row_normalize_f32` at their edges, straight from device panels -- no model fit.

Rotation step: every case of tests/rotation_reference.py (its docstring lists them and derives the bound; the module is
checked on its own in tests/test_rotation_reference_cpu.py).  Per case
  * |G - G_ref| <= MARGIN * B elementwise on the whole L x L result, G_ref and B from the long-double reference,
  * the padding block of G (rows and columns >= m, within each half in the complex modes) is an exact zero,
  * a second launch returns the same bits (the partials are reduced in a fixed order),
  * modes 2 / 3: `cpanel.block(G)` against the step written in complex long-double arithmetic, within the same bound mapped
    through the block sum.
Each case prints `ROT L=.. mode=.. rows=.. max(err/bound)=..`.

Row normalisation: out = x / (||x|| + 2.220446049250313e-16) per row in long double; the kernel computes the quotient in
float64 and rounds it once to float32, hence |out - ref| <= 2^-24 |ref| (1 + 1e-6) + 2^-149 per element (the 1e-6 leaves
6e-14 |ref| for the float64 arithmetic -- a 256-term sum of squares, a square root, a reciprocal and a product, about 1e-15).
"""

import numpy as np
import pytest

import rotation_reference as rref

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
needs_extended = pytest.mark.skipif(not rref.EXTENDED, reason="long double is float64 on this platform")


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@needs_extended
@pytest.mark.parametrize("case", rref.CASES, ids=rref.case_id)
def test_rot_step_within_derived_bound(ctx, case):
    from xeofs_amd import cpanel, engine

    L, mode, m, rows, power, spread = case
    c = rref.case_inputs(case)
    X, R, aux = _dev(c["X"]), _dev(c["R"]), _dev(c["aux"])
    assert X.shape == (rows, L)                                        # not padded to 512: the kernel guards the rows
    g = _bits(engine.panel_rot_step(ctx, X, R, aux, mode, float(power)))
    g2 = _bits(engine.panel_rot_step(ctx, X, R, aux, mode, float(power)))
    Gref, B = rref.case_reference(case)
    assert g.shape == (L, L) and np.isfinite(g).all(), "G has elements that are not finite"
    err = np.abs(g.astype(rref.LD) - Gref)
    lim = rref.MARGIN * B + rref.TINY
    ratio = float((err / lim).max())
    print(f"ROT L={L} mode={mode} m={m} rows={rows} power={power}{' spread' if spread else ''} max(err/bound)={ratio:.3g}")
    bad = np.argwhere(err > lim)
    assert bad.size == 0, f"{len(bad)} elements outside the bound, first at {bad[0]}, worst ratio {ratio:.3g}"
    assert not g[rref.padding_mask(L, mode, m)].any(), "the padding block is not an exact zero"
    assert np.array_equal(g.view(np.int64), g2.view(np.int64)), "a second launch returned other bits"
    if mode >= 2:
        half = c["half"]
        ref = rref.crot_step_ref(rref.unpack(c["X"], m, half), c["Rc"], c["auxh"], mode, power)
        got = cpanel.block(g, m, half)
        bre, bim = rref.block_sum(B, m, half)
        rre, rim = rref.block_sum(np.abs(g), m, half)                    # (one float64 rounding inside cpanel.block)
        ere, eim = np.abs(got.real.astype(rref.LD) - ref.real), np.abs(got.imag.astype(rref.LD) - ref.imag)
        assert (ere <= rref.MARGIN * bre + rref.U * rre + rref.TINY).all(), float((ere / (rref.MARGIN * bre + rref.TINY)).max())
        assert (eim <= rref.MARGIN * bim + rref.U * rim + rref.TINY).all(), float((eim / (rref.MARGIN * bim + rref.TINY)).max())


@pytest.mark.parametrize("L,mode", [(48, 0), (64, 4), (32, 2), (64, -1), (32, 3)])
def test_rot_step_argument_checks(ctx, L, mode):
    """an error code, the ValueError of the Python entry, and nothing launched: G keeps what it held"""
    import torch
    from xeofs_amd import _lib, engine
    from xeofs_amd._lib import ptr

    X = torch.ones((64, L), dtype=torch.float32, device="cuda")
    R = torch.eye(L, dtype=torch.float64, device="cuda")
    aux = torch.ones(L, dtype=torch.float64, device="cuda")
    G = torch.full((L, L), 7.0, dtype=torch.float64, device="cuda")
    rc = ctx.lib.eofx_panel_rot_step_f64(ctx.handle, ptr(X), 64, L, ptr(R), ptr(aux), mode, 1.0, ptr(G))
    assert rc == _lib.ERR_ARG
    assert (_bits(G) == 7.0).all()
    with pytest.raises(ValueError, match="bad argument"):
        engine.panel_rot_step(ctx, X, R, aux, mode)


# ----------------------------------------------------------------------------------------------------------------------
KINDS = ("gauss", "zero", "single", "tiny", "huge")


def _rows_of_kinds(rows, L, shift, seed):
    """row r is of kind KINDS[(r + shift) % 5]: N(0, 1) times 10^U(-3, 3); all zero; one non-zero entry; entries near 1e-20
    (the eps of the denominator dominates the norm); entries near 1e18"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((rows, L)) * 10.0 ** rng.uniform(-3, 3, (rows, 1))
    kind = (np.arange(rows) + shift) % 5
    P[kind == 1] = 0.0
    one = np.flatnonzero(kind == 2)
    keep = P[one, (one * 7) % L].copy()
    P[one] = 0.0
    P[one, (one * 7) % L] = keep
    P[kind == 3] = rng.standard_normal((int((kind == 3).sum()), L)) * 1e-20
    P[kind == 4] = rng.standard_normal((int((kind == 4).sum()), L)) * 1e18
    return P.astype(np.float32), kind


@needs_extended
@pytest.mark.parametrize("L", [32, 64, 128, 256])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 4099])
def test_row_normalize_rounds_once(ctx, rows, L):
    """one wave per row, four rows per workgroup: row counts around the quad, every kind of row at every position of a
    short panel (shifts 0 .. 4), out of place into a NaN-filled output and in place"""
    import torch
    from xeofs_amd import engine

    for shift in range(5 if rows <= 5 else 1):
        Ph, kind = _rows_of_kinds(rows, L, shift, seed=1000 * rows + L + shift)
        x = Ph.astype(rref.LD)
        ref = x / (np.sqrt((x * x).sum(1)) + rref.LD(EPS))[:, None]
        lim = 2.0 ** -24 * np.abs(ref) * (1 + 1e-6) + 2.0 ** -149
        P = _dev(Ph)
        out = torch.full((rows, L), float("nan"), dtype=torch.float32, device="cuda")
        got = _bits(engine.panel_row_normalize(ctx, P, out=out))
        assert np.isfinite(got).all(), f"{np.count_nonzero(~np.isfinite(got))} elements unwritten or not finite"
        assert np.array_equal(_bits(P), Ph), "the input panel changed"
        err = np.abs(got.astype(rref.LD) - ref)
        ratio = float((err / lim).max())
        print(f"NORM L={L} rows={rows} shift={shift} max(err/bound)={ratio:.3g}")
        assert (err <= lim).all(), f"worst ratio {ratio:.3g} at {np.argwhere(err > lim)[0]}, kind {KINDS[kind[np.argwhere(err > lim)[0][0]]]}"
        assert not got[kind == 1].any(), "a zero row is not an exact zero"
        single = got[kind == 2]
        assert (np.count_nonzero(single, axis=1) == 1).all()
        if (kind == 3).any():      # eps dominates: far from unit length
            assert (np.abs(got[kind == 3]).max(1) < 1e-2).all()
        inplace = _bits(engine.panel_row_normalize(ctx, P, out=P))
        assert np.array_equal(inplace.view(np.int32), got.view(np.int32)), "in place differs from out of place"
