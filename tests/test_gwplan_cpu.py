"""The host plan of geographically weighted PCA (xeofs_amd/csrc/eofx_gwplan.hpp: Morton tiling, bounds, the CSR list of neighbour
tiles) without a GPU: plain C++ compiled into tests/plans_shim.cpp with the host compiler and called through ctypes.  The plan
may only leave out a tile pair whose weights are ALL exactly 0.0 in float64 -- computed here in numpy with gw_weight's formula
(csrc/eofx_gw.hpp) from the plan's own geo arrays, as the kernel does."""
import numpy as np
import pytest

import plans_shim

METRICS = {"euclidean": 0, "haversine": 1}
KERNELS = {"bisquare": 0, "gaussian": 1, "exponential": 2}
EARTH_RADIUS = 6371.0
# bandwidths at which the lists leave tile pairs out on the wide location sets below: a bisquare weight is 0 beyond bw, a
# gaussian one underflows beyond sqrt(1500) bw (39 bw), an exponential one beyond 1500 bw (km for haversine, coordinate units
# for euclidean: the sets span 20 x 120 degrees, about 13 000 km)
BANDWIDTH = {("haversine", "bisquare"): 500.0, ("haversine", "gaussian"): 50.0, ("haversine", "exponential"): 2.0,
             ("euclidean", "bisquare"): 8.0, ("euclidean", "gaussian"): 0.5, ("euclidean", "exponential"): 0.02}
SIZES = [1, 16, 17, 700]


@pytest.fixture(scope="module")
def lib():
    return plans_shim.lib()


def locations(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "dateline":      # longitudes 170 .. 190, written in [-180, 180): the set straddles the dateline
        lon = rng.uniform(170.0, 190.0, n)
        return np.stack([np.where(lon >= 180.0, lon - 360.0, lon), rng.uniform(-60.0, 60.0, n)], 1)
    if kind == "polar":         # a cap around the north pole, the pole itself included
        xy = np.stack([rng.uniform(-180.0, 180.0, n), rng.uniform(75.0, 90.0, n)], 1)
        xy[0] = (0.0, 90.0)
        return xy
    if kind == "equal":
        return np.tile([[12.5, -33.0]], (n, 1))
    assert kind == "axis"       # one degenerate axis: every point at the same second coordinate
    return np.stack([rng.uniform(-150.0, 150.0, n), np.full(n, 40.0)], 1)


def weights(gi, gj, metric, kernel, bw):
    """gw_weight of every pair: gi [a x 3], gj [b x 3] as the plan stores them ({lon, lat, cos lat} in radians, or {x, y, 0})"""
    gi, gj = gi[:, None, :], gj[None, :, :]
    if metric == "haversine":
        slat, slon = np.sin(0.5 * (gj[..., 1] - gi[..., 1])), np.sin(0.5 * (gj[..., 0] - gi[..., 0]))
        a = np.clip(slat * slat + gi[..., 2] * gj[..., 2] * (slon * slon), 0.0, 1.0)
        d = EARTH_RADIUS * (2.0 * np.arctan2(np.sqrt(a), np.sqrt(1.0 - a)))
    else:
        d = np.sqrt((gj[..., 0] - gi[..., 0]) ** 2 + (gj[..., 1] - gi[..., 1]) ** 2)
    u = d / bw
    if kernel == "bisquare":
        return np.where(d <= bw, (1.0 - u * u) ** 2, 0.0)
    with np.errstate(under="ignore"):
        return np.exp(-0.5 * (u * u)) if kernel == "gaussian" else np.exp(-0.5 * u)


class Plan:
    def __init__(self, lib, xy, metric, kernel, bw, sorted_=True, first=0, count=None, chunk=None):
        xy = np.ascontiguousarray(xy, np.float64)
        n = xy.shape[0]
        count = n if count is None else count
        h = lib.gwp_build(xy.ctypes.data, n, first, count, chunk or count, int(sorted_), METRICS[metric], KERNELS[kernel], bw)
        try:
            sz = np.zeros(8, np.int64)
            lib.gwp_sizes(h, sz.ctypes.data)
            nch, self.ctiles, ncols, nrowptr, self.visited, self.possible, self.ntiles, centres = sz.tolist()
            self.nb_perm, self.nb_geo = np.zeros(n, np.int64), np.zeros((n, 3))
            self.rowptr, self.cols = np.zeros(nrowptr, np.int32), np.zeros(max(ncols, 1), np.int32)
            self.info, self.c_perm, self.c_geo = np.zeros((nch, 5), np.int64), np.zeros(centres, np.int64), np.zeros((centres, 3))
            lib.gwp_copy(h, self.nb_perm.ctypes.data, self.nb_geo.ctypes.data, self.rowptr.ctypes.data, self.cols.ctypes.data,
                         self.info.ctypes.data, self.c_perm.ctypes.data, self.c_geo.ctypes.data)
            self.cols = self.cols[:ncols]
        finally:
            lib.gwp_free(h)

    def chunks(self):
        """(index, first, count, centre tiles, centres' offset in c_perm / c_geo, the chunk's rowptr, its cols) -- as gw_run reads them"""
        off = 0
        for ci, (first, count, off_tiles, off_cols, tiles) in enumerate(self.info.tolist()):
            rp = self.rowptr[off_tiles + ci:off_tiles + ci + tiles + 1]
            yield ci, first, count, tiles, off, rp, self.cols[off_cols:off_cols + rp[-1]]
            off += count


def check_plan(pl, xy, metric, kernel, bw, T, centres):
    """-> True when the lists leave a tile pair out.  centres: the rows of xy that must appear as centres, each once."""
    n = xy.shape[0]
    assert np.array_equal(np.sort(pl.nb_perm), np.arange(n))
    assert np.array_equal(np.sort(pl.c_perm), np.sort(centres))
    assert pl.ntiles == (n + T - 1) // T and pl.visited == pl.cols.size and pl.visited <= pl.possible
    listed_all = 0
    for ci, first, count, tiles, off, rp, cols in pl.chunks():
        assert tiles == (count + T - 1) // T and rp[0] == 0 and np.all(np.diff(rp) >= 0)
        w = weights(pl.c_geo[off:off + count], pl.nb_geo, metric, kernel, bw)
        # any weight != 0 per (centre tile, neighbour tile)
        pad = np.zeros((tiles * T, pl.ntiles * T), bool)
        pad[:count, :n] = w != 0.0
        live = pad.reshape(tiles, T, pl.ntiles, T).any(axis=(1, 3))
        listed = np.zeros((tiles, pl.ntiles), bool)
        for a in range(tiles):
            row = cols[rp[a]:rp[a + 1]]
            assert np.all(np.diff(row) > 0) and (row.size == 0 or (row[0] >= 0 and row[-1] < pl.ntiles))      # ascending, in range
            listed[a, row] = True
        assert not (live & ~listed).any(), (metric, kernel, n, np.argwhere(live & ~listed)[:3])
        listed_all += int(listed.sum())
    assert listed_all == pl.visited
    return pl.visited < pl.possible


@pytest.mark.parametrize("metric", list(METRICS))
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_unlisted_tile_pairs_have_zero_weights(lib, metric, kernel):
    T = plans_shim.constants(lib)["GW_T"]
    bw = BANDWIDTH[(metric, kernel)]
    pruned = {}
    for kind in ("dateline", "polar", "equal", "axis"):
        for n in SIZES:
            xy = locations(kind, n, n)
            # sorted: every location is a centre, in chunks of 2 tiles; a sorted plan's chunk tiles are the neighbour tiles themselves
            pl = Plan(lib, xy, metric, kernel, bw, chunk=2 * T)
            pruned[(kind, n)] = check_plan(pl, xy, metric, kernel, bw, T, np.arange(n))
            assert np.array_equal(pl.c_perm, pl.nb_perm) and np.array_equal(pl.c_geo, pl.nb_geo)
            assert [c[1] for c in pl.chunks()] == list(range(0, n, 2 * T)) and pl.ctiles == pl.ntiles
            # unsorted: the centres [first, first + count) as one chunk, tiled among themselves
            first, count = n // 3, n - n // 2
            pu = Plan(lib, xy, metric, kernel, bw, sorted_=False, first=first, count=count)
            check_plan(pu, xy, metric, kernel, bw, T, np.arange(first, first + count))
            assert len(pu.info) == 1 and pu.info[0].tolist()[:2] == [first, count]
    # the check above is not vacuous: on the wide sets the lists leave tile pairs out -- and never where all points coincide
    assert pruned[("dateline", 700)] and pruned[("axis", 700)]
    assert not any(pruned[("equal", n)] for n in SIZES)


@pytest.mark.parametrize("metric", list(METRICS))
def test_bandwidth_above_the_diameter_lists_every_pair(lib, metric):
    T = plans_shim.constants(lib)["GW_T"]
    bw = 25000.0 if metric == "haversine" else 1000.0          # (half the earth's circumference is 20 015 km)
    for kind in ("dateline", "polar", "equal", "axis"):
        for n in SIZES:
            xy = locations(kind, n, n)
            pl = Plan(lib, xy, metric, "bisquare", bw, chunk=3 * T)
            assert pl.visited == pl.possible == pl.ntiles ** 2
            assert not check_plan(pl, xy, metric, "bisquare", bw, T, np.arange(n))
