"""The layout of the fp16 planes an in-place X Y pass reads its panel from (eofx_plans.hpp, axb_plane_offset -- the one statement
of it that axb_bsplit_kernel and the two plane producers write through), against a NumPy restatement of the order the LDS-DMA
kernel consumes: [column block][feature pair][plane][k-group of 8][column slot c ^ ((c >> 3) & 7)][8 halves].  No GPU."""
import numpy as np
import pytest

import planes_shim


@pytest.fixture(scope="module")
def lib():
    return planes_shim.lib()


def restated_offsets(K_all, L):
    """byte offset of every (column, feature k, plane) of a [K_all x L] panel, by building the nested array the kernel's
    addressing describes and reading where each element landed"""
    ncb, pairs = (L + 63) // 64, K_all // 64
    index = np.arange(ncb * pairs * 2 * 8 * 64 * 8, dtype=np.int64).reshape(ncb, pairs, 2, 8, 64, 8) * 2      # bytes of a half
    col, k, plane = np.meshgrid(np.arange(64 * ncb), np.arange(K_all), np.arange(2), indexing="ij")
    c = col & 63
    return index[col >> 6, k >> 6, plane, (k >> 3) & 7, c ^ ((c >> 3) & 7), k & 7]


def test_constants(lib):
    out = np.zeros(3, np.int32)
    lib.ps_constants(out.ctypes.data)
    assert out.tolist() == [64, 8 * 64 * 16, 2 * 8 * 64 * 16]


@pytest.mark.parametrize("K_all, L", [(64, 32), (256, 64), (320, 96)])
def test_offset_of_every_element(lib, K_all, L):
    want = restated_offsets(K_all, L)
    got = np.empty_like(want)
    for col in range(want.shape[0]):
        for k in range(K_all):
            for plane in range(2):
                got[col, k, plane] = lib.ps_plane_offset(col >> 6, K_all, k, col & 63, plane)
    assert np.array_equal(got, want)
    nbytes = lib.ps_planes_bytes(K_all, L)
    assert nbytes == ((L + 63) // 64) * (K_all // 64) * 16384
    # a bijection onto the halves of the buffer; a (k-group, column, plane) is one aligned 16-byte unit
    assert np.array_equal(np.sort(got.ravel()), np.arange(0, nbytes, 2))
    units = got.reshape(want.shape[0], K_all // 8, 8, 2)
    assert np.all(units[:, :, 0, :] % 16 == 0) and np.all(np.diff(units, axis=2) == 2)
    # the lo plane of a unit lies one plane (8 KiB) behind its hi plane
    assert np.all(got[:, :, 1] - got[:, :, 0] == 8192)
