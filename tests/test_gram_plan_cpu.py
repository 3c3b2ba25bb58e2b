"""The work list of gram_nt_kernel (gram_plan_build in xeofs_amd/csrc/eofx_plans.hpp) without a GPU, through tests/plans_shim.cpp:
the invariants the kernel and the two finish kernels rely on, over a grid of tile counts, stage counts and split counts, and the
Python restatement of the split rule (tests/test_gpu_nt_routes.py: gram_plan) against the header on that whole grid."""
import itertools

import numpy as np
import pytest

import plans_shim
import test_gpu_nt_routes as nt

NTS = [1, 2, 3, 4, 6, 7, 8, 128]
NSTS = [2, 4, 6, 22, 26, 34, 46, 130, 2050]      # even: the callers pad the contraction to 64 features
SPLITS = [0, 1, 2, 3, 5, 16, 40]                 # 0: the plan's own choice


@pytest.fixture(scope="module")
def lib():
    return plans_shim.lib()


def c_gram_plan(lib, nti, ntj, sym, nst_total, S):
    """-> (S, st_per_split, T, grid, items [grid][5] = {bi, bj, st0, nst, slot}, tiles [T][2])"""
    head = np.zeros(4, np.int32)
    assert lib.pl_gram_plan(nti, ntj, int(sym), nst_total, S, head.ctypes.data, None, 0, None, 0) == 1
    items, tiles = np.zeros((int(head[3]), 5), np.int32), np.zeros((int(head[2]), 2), np.int32)
    assert lib.pl_gram_plan(nti, ntj, int(sym), nst_total, S, head.ctypes.data, items.ctypes.data, len(items), tiles.ctypes.data, len(tiles)) == 0
    return int(head[0]), int(head[1]), int(head[2]), int(head[3]), items, tiles


def morton(i, j):
    m = np.zeros_like(i, dtype=np.int64)
    for b in range(12):
        m |= ((i >> b) & 1).astype(np.int64) << (2 * b + 1) | ((j >> b) & 1).astype(np.int64) << (2 * b)
    return m


def check_plan(nti, ntj, sym, nst_total, S_req, plan):
    S, sps, T, grid, items, tiles = plan
    what = (nti, ntj, sym, nst_total, S_req)
    # every tile once -- the upper triangle only when sym --, in non-decreasing Morton order
    want = np.array([(i, j) for i in range(nti) for j in range(i if sym else 0, ntj)], np.int64).reshape(-1, 2)
    assert T == len(want) == len(tiles), what
    code = tiles[:, 0].astype(np.int64) * 4096 + tiles[:, 1]
    assert np.array_equal(np.sort(code), want[:, 0] * 4096 + want[:, 1]), what
    assert (np.diff(morton(tiles[:, 0], tiles[:, 1])) >= 0).all(), what
    # the split: even, a forced S normalised to the number of non-empty splits
    assert sps % 2 == 0 and sps >= 2 and S == -(-nst_total // sps) and (S - 1) * sps < nst_total, what
    if S_req > 0:
        assert sps == (-(-nst_total // S_req) + 1) // 2 * 2, what
    lo = [T * x // 8 for x in range(9)]
    cmax = max(lo[x + 1] - lo[x] for x in range(8))
    assert grid == 8 * cmax * S == len(items), what
    bi, bj, st0, nst, slot = (items[:, c].astype(np.int64) for c in range(5))
    real = nst > 0
    assert (nst[~real] == 0).all() and real.sum() == T * S, what
    # real items: even and at least 2 stages, st0 = split * st_per_split, slot = tile * S + split, unique, below T * S
    tile, split = slot[real] // S, slot[real] % S
    assert (nst[real] % 2 == 0).all() and (nst[real] >= 2).all(), what
    assert (slot[real] >= 0).all() and (slot[real] < T * S).all() and len(np.unique(slot[real])) == T * S, what
    assert np.array_equal(st0[real], split * sps), what
    assert np.array_equal(bi[real], tiles[tile, 0]) and np.array_equal(bj[real], tiles[tile, 1]), what
    # the real items of a tile partition [0, nst_total) in order: no gap, no overlap
    order = np.argsort(slot[real])
    s0, ns = st0[real][order].reshape(T, S), nst[real][order].reshape(T, S)
    assert (s0[:, 0] == 0).all() and np.array_equal(s0[:, 1:], (s0 + ns)[:, :-1]) and ((s0 + ns)[:, -1] == nst_total).all(), what
    # the item at index 8 w + x belongs to XCD x's contiguous patch of tiles; inside the patch the items walk split by split
    # (all tiles of the patch at split 0, then at split 1, ...), the rest of the lane is empty
    idx = np.flatnonzero(real)
    w, x = idx // 8, idx % 8
    lo_x, cnt = np.array(lo)[x], (np.array(lo[1:]) - np.array(lo[:-1]))[x]
    assert (tile >= lo_x).all() and (tile < lo_x + cnt).all() and (w < cnt * S).all(), what
    assert np.array_equal(split, w // np.maximum(cnt, 1)) and np.array_equal(tile, lo_x + w % np.maximum(cnt, 1)), what
    return S, sps


def test_work_list_invariants_and_restated_split_rule(lib):
    count = 0
    for nti, ntj, sym, nst_total, S_req in itertools.product(NTS, NTS, (True, False), NSTS, SPLITS):
        plan = c_gram_plan(lib, nti, ntj, sym, nst_total, S_req)
        S, sps = check_plan(nti, ntj, sym, nst_total, S_req, plan)
        py = nt.gram_plan(nti, ntj, sym, nst_total, S_req)
        assert (py["S"], py["st_per_split"], py["T"], py["grid"]) == plan[:4], (nti, ntj, sym, nst_total, S_req, py, plan[:4])
        assert py["last"] == nst_total - (S - 1) * sps and py["last"] >= 2
        count += 1
    assert count == 8 * 8 * 2 * 9 * 7


def test_forced_split_counts(lib):
    """S = 40 of 26 stages is normalised to 13 splits of 2; S = 5 of 26 stages leaves a last split of exactly 2"""
    S, sps, T, grid, items, _ = c_gram_plan(lib, 2, 2, True, 26, 40)
    assert (S, sps, T, grid) == (13, 2, 3, 8 * 13)
    S, sps, T, grid, items, _ = c_gram_plan(lib, 2, 2, True, 26, 5)
    assert (S, sps) == (5, 6)
    last = items[(items[:, 3] > 0) & (items[:, 4] % S == S - 1)]
    assert len(last) == T and (last[:, 3] == 2).all() and (last[:, 2] == 24).all()
    assert nt.gram_plan(2, 2, True, 26, 40)["S"] == 13 and nt.gram_plan(2, 2, True, 26, 5)["last"] == 2


def test_restated_plans_of_the_gpu_shape_lists(lib):
    """the plans tests/test_nt_model_host.py reasons with are the header's, at every split count the GPU test forces"""
    for S_req in [s or 0 for s in nt.SPLITS]:
        for n, p in nt.GRAM_SHAPES + [nt.LAYOUT_SHAPE[:2], nt.ODD_SHAPE[:2], nt.SPREAD_GRAM[::-1]]:
            ntile, nst = nt._up(n, 512) // 256, nt._up(p, 64) // 32
            assert tuple(nt.gram_shape_plan(n, p, S_req)[k] for k in ("S", "st_per_split", "T", "grid")) == c_gram_plan(lib, ntile, ntile, True, nst, S_req)[:4]
        for n, p, L in nt.TMUL_SHAPES + [nt.LAYOUT_SHAPE, nt.ODD_SHAPE]:
            got = c_gram_plan(lib, nt._up(p, 512) // 256, nt._up(L, 256) // 256, False, nt._up(n, 64) // 32, S_req)[:4]
            assert tuple(nt.tmul_shape_plan(n, p, L, S_req)[k] for k in ("S", "st_per_split", "T", "grid")) == got
        for rows, L, Lo in nt.MATMUL_SHAPES:
            got = c_gram_plan(lib, rows // 256, nt._up(Lo, 256) // 256, False, nt._up(L, 64) // 32, S_req)[:4]
            assert tuple(nt.matmul_shape_plan(rows, L, Lo, S_req)[k] for k in ("S", "st_per_split", "T", "grid")) == got
