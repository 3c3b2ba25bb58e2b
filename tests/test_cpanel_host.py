"""Host tests of xeofs_amd/cpanel.py, the [Re | Im] layout of complex panels: every function against plain numpy complex
arithmetic in complex128.  No GPU; panels are host arrays or CPU tensors.  The inputs are float32-representable, so packing
them is exact and what is left is the float64 rounding of the products (rtol 1e-13).
"""

import numpy as np
import pytest
import torch

from xeofs_amd import cpanel, engine

ROWS = 37
WIDTHS = [(32, 32, 5, 5), (32, 64, 20, 40), (64, 64, 33, 33), (128, 128, 100, 100)]      # half_in, half_out, m, m'
RTOL = 1e-13


def _complex(rng, *shape):
    """complex128 values that complex64 holds exactly"""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64).astype(np.complex128)


def _close(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0.0)


@pytest.mark.parametrize("hin,hout,m,mo", WIDTHS)
def test_embed_multiplies_on_the_right(hin, hout, m, mo):
    rng = np.random.default_rng(hin + m)
    P, M = _complex(rng, ROWS, m), _complex(rng, m, mo)
    E = cpanel.embed(M, hin, hout)
    assert E.shape == (2 * hin, 2 * hout) and E.dtype == np.float64
    if hin == hout:
        assert np.array_equal(E, cpanel.embed(M, hin))
    A = cpanel.pack(P, hin)
    assert A.shape == (ROWS, 2 * hin) and A.dtype == np.float32
    out = A.astype(np.float64) @ E
    _close(cpanel.unpack(out, ROWS, mo, hout, np.complex128), P @ M)
    used = np.zeros(2 * hout, bool)
    used[:mo] = used[hout:hout + mo] = True
    assert not out[:, ~used].any()                      # the padding columns stay zero


@pytest.mark.parametrize("hin,hout,m,mo", WIDTHS)
def test_block_of_a_gram_and_of_a_block_stack(hin, hout, m, mo):
    rng = np.random.default_rng(hin + m + 1)
    Ps = [_complex(rng, ROWS, m) for _ in range(3)]
    A = np.concatenate([cpanel.pack(P, hin) for P in Ps], axis=1).astype(np.float64)
    G = A.T @ A
    lp = 2 * hin
    _close(cpanel.block(G, m, hin), Ps[0].conj().T @ Ps[0])
    for i in range(3):
        for j in range(3):
            ref = Ps[i].conj().T @ Ps[j]
            raw = cpanel.block(G, m, hin, i * lp, j * lp)
            _close(raw, ref)
            H = cpanel.block(G, m, hin, i * lp, j * lp, hermitian=True)
            assert np.array_equal(H, H.conj().T)
            assert np.array_equal(H, 0.5 * (raw + raw.conj().T))
            if i != j:                                  # a cross product is not Hermitian: the raw value is not symmetrised
                assert not np.allclose(raw, raw.conj().T)
                _close(cpanel.block(G, m, hin, i * lp, j * lp, hermitian=False), ref)


@pytest.mark.parametrize("hin,hout,m,mo", WIDTHS)
def test_pack_unpack_round_trip(hin, hout, m, mo):
    rng = np.random.default_rng(hin + m + 2)
    Z = _complex(rng, ROWS, m).astype(np.complex64)
    A = cpanel.pack(Z, hin)
    assert np.array_equal(A[:, :m], Z.real) and np.array_equal(A[:, hin:hin + m], Z.imag)
    assert not A[:, m:hin].any() and not A[:, hin + m:].any()
    for panel in (A, torch.from_numpy(A)):
        back = cpanel.unpack(panel, ROWS, m, hin, np.complex64)
        assert back.dtype == np.complex64 and np.array_equal(back, Z)
        wide = cpanel.unpack(panel, ROWS - 3, m, hin, np.complex128)
        assert wide.dtype == np.complex128 and np.array_equal(wide, Z[:ROWS - 3].astype(np.complex128))
    # into an existing padded panel, host array or tensor: only the two r x m slices are written, float64 parts are rounded once
    Zd = Z.astype(np.complex128) * (1.0 + 2.0 ** -30)
    ref = np.full((ROWS + 11, 2 * hin), 7.0, np.float32)
    ref[:ROWS, :m], ref[:ROWS, hin:hin + m] = Zd.real.astype(np.float32), Zd.imag.astype(np.float32)
    host = cpanel.pack(Zd, hin, out=np.full((ROWS + 11, 2 * hin), 7.0, np.float32))
    dev = cpanel.pack(Zd, hin, out=torch.full((ROWS + 11, 2 * hin), 7.0, dtype=torch.float32))
    assert np.array_equal(host, ref) and torch.is_tensor(dev) and np.array_equal(dev.numpy(), ref)
    # a column offset: columns [c0, c0 + m') of both halves
    c0 = m // 2
    part = cpanel.pack(Z[:, c0:] * 2, hin, out=A.copy(), c0=c0)
    exp = Z.copy()
    exp[:, c0:] *= 2
    assert np.array_equal(part, cpanel.pack(exp, hin))


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("hin,hout,m,mo", WIDTHS)
def test_lexicographic_sign(hin, hout, m, mo, conj):
    rng = np.random.default_rng(hin + m + 3)
    Z = _complex(rng, ROWS, m)
    assert all(np.unique(Z[:, j].real).size == ROWS for j in range(m))       # no ties on the real part: max / min are unambiguous
    P = torch.from_numpy(cpanel.pack(Z, hin))
    amax, amin = P.argmax(dim=0), P.argmin(dim=0)        # CPU index tensors over all 2 half columns, like panel_colargminmax
    k = m - 1
    mr, mi, nr, ni = cpanel.lex_extrema(P, amax, amin, k, hin, conj=conj)
    Zc = (Z.conj() if conj else Z)[:, :k]
    for a in (mr, mi, nr, ni):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (k,)
    assert np.array_equal(mr + 1j * mi, Zc.max(axis=0)) and np.array_equal(nr + 1j * ni, Zc.min(axis=0))
    sign = cpanel.lex_sign(mr, mi, nr, ni)
    ref = np.where(np.abs(Zc.max(axis=0)) >= np.abs(Zc.min(axis=0)), 1, -1)
    assert np.array_equal(sign, ref)
    if k >= 20:
        assert (ref == 1).any() and (ref == -1).any()


def test_permute_export(monkeypatch):
    """column j = column idx[j] times w[j], through one embedded product (here: a float64 product on the host in place of the
    device's; the result is rounded to complex64 once, 2^-24 per part)"""
    monkeypatch.setattr(engine, "panel_matmul", lambda ctx, P, E: P.double() @ E)
    rng = np.random.default_rng(11)
    half, k = 32, 6
    Z = _complex(rng, ROWS, k)
    P = torch.from_numpy(np.concatenate([cpanel.pack(Z, half), np.zeros((5, 2 * half), np.float32)]))
    idx, w = rng.permutation(k), rng.standard_normal(k)
    out = cpanel.permute_export(None, P, ROWS, idx, w, half)
    assert out.dtype == np.complex64 and out.shape == (ROWS, k)
    np.testing.assert_allclose(out, Z[:, idx] * w, rtol=2.0 ** -23, atol=0.0)
