// eofx_gwplan.hpp -- the host plan of geographically weighted PCA (kernels: eofx_gw.hpp): the locations in Morton order, cut
// into tiles with a bound each, and per tile of centres the CSR list of the neighbour tiles that can hold a weight > 0.
// Plain C++17, no HIP: tests/test_gwplan_cpu.py checks the lists against the float64 weights without a GPU.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "eofx.h"

namespace eofx {

constexpr int GW_T = 16;          // locations per tile (one weight per thread for a 16 x 16 tile pair)
constexpr double GW_EARTH_RADIUS = 6371.0;   // xeofs/utils/constants.py AVG_EARTH_RADIUS, km

// One set of locations cut into tiles of GW_T in Morton order of their (normalised) coordinates, with a bound per tile
// and per group of 16 tiles: for haversine the unit-vector centre and angular radius (handles the dateline and the
// poles), for euclidean the bounding box.
struct GwTiles {
  std::vector<int64_t> perm;   // sorted position -> row of X
  std::vector<double> geo;     // [3 x sorted position] (eofx_gw.hpp gw_weight)
  std::vector<std::array<double, 4>> tile, group;
  int64_t count = 0, ntiles = 0;
};

inline double gw_angle(const double* a, const double* b) {
  const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  return std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

inline std::array<double, 4> gw_bound(const std::vector<double>& u, int64_t s0, int64_t s1, int metric) {
  if (metric == EOFX_GW_METRIC_EUCLIDEAN) {
    std::array<double, 4> b{u[3 * s0], u[3 * s0], u[3 * s0 + 1], u[3 * s0 + 1]};
    for (int64_t s = s0 + 1; s < s1; ++s) {
      b[0] = std::min(b[0], u[3 * s]);
      b[1] = std::max(b[1], u[3 * s]);
      b[2] = std::min(b[2], u[3 * s + 1]);
      b[3] = std::max(b[3], u[3 * s + 1]);
    }
    return b;
  }
  double c[3] = {0.0, 0.0, 0.0};
  for (int64_t s = s0; s < s1; ++s)
    for (int d = 0; d < 3; ++d) c[d] += u[3 * s + d];
  const double nrm = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  for (int d = 0; d < 3; ++d) c[d] = nrm > 1e-9 * (double)(s1 - s0) ? c[d] / nrm : u[3 * s0 + d];
  double rho = 0.0;
  for (int64_t s = s0; s < s1; ++s) rho = std::max(rho, gw_angle(c, &u[3 * s]));
  return {c[0], c[1], c[2], rho};
}

// a lower bound of every distance between two bounded sets (km for haversine, less a margin of 1e-9 rad for rounding)
inline double gw_lower(const std::array<double, 4>& a, const std::array<double, 4>& b, int metric) {
  if (metric == EOFX_GW_METRIC_EUCLIDEAN) {
    const double dx = std::max({0.0, a[0] - b[1], b[0] - a[1]}), dy = std::max({0.0, a[2] - b[3], b[2] - a[3]});
    return std::sqrt(dx * dx + dy * dy);
  }
  const double th = gw_angle(a.data(), b.data()) - a[3] - b[3] - 1e-9;
  return th > 0.0 ? GW_EARTH_RADIUS * th : 0.0;
}

// true when every weight at a distance >= dlb is exactly 0 in float64 (bisquare: beyond the bandwidth; gaussian and
// exponential: exp of an argument below -750 underflows to 0)
inline bool gw_zero(double dlb, int kernel, double bw) {
  const double u = dlb / bw;
  if (kernel == EOFX_GW_KERNEL_BISQUARE) return dlb > bw;
  if (kernel == EOFX_GW_KERNEL_GAUSSIAN) return 0.5 * u * u > 750.0;
  return 0.5 * u > 750.0;
}

inline uint64_t gw_morton(uint32_t x, uint32_t y) {
  uint64_t k = 0;
  for (int b = 0; b < 16; ++b) k |= (uint64_t)((x >> b) & 1u) << (2 * b) | (uint64_t)((y >> b) & 1u) << (2 * b + 1);
  return k;
}

inline void gw_tile(const double* xy, int64_t first, int64_t count, int metric, const double* box, GwTiles& t) {
  t.count = count;
  t.ntiles = (count + GW_T - 1) / GW_T;
  std::vector<std::pair<uint64_t, int64_t>> key((size_t)count);
  for (int64_t i = 0; i < count; ++i) {
    const double* c = xy + 2 * (first + i);
    const double fx = box[1] > box[0] ? (c[0] - box[0]) / (box[1] - box[0]) : 0.0;
    const double fy = box[3] > box[2] ? (c[1] - box[2]) / (box[3] - box[2]) : 0.0;
    key[(size_t)i] = {gw_morton((uint32_t)std::min(65535.0, std::max(0.0, fx * 65535.0)),
                                (uint32_t)std::min(65535.0, std::max(0.0, fy * 65535.0))), first + i};
  }
  std::sort(key.begin(), key.end());
  t.perm.resize((size_t)count);
  t.geo.resize(3 * (size_t)count);
  std::vector<double> u(3 * (size_t)count);
  for (int64_t s = 0; s < count; ++s) {
    const int64_t i = key[(size_t)s].second;
    t.perm[(size_t)s] = i;
    const double x = xy[2 * i], y = xy[2 * i + 1];
    if (metric == EOFX_GW_METRIC_HAVERSINE) {
      const double lon = x * (M_PI / 180.0), lat = y * (M_PI / 180.0);
      t.geo[3 * s] = lon;
      t.geo[3 * s + 1] = lat;
      t.geo[3 * s + 2] = std::cos(lat);
      u[3 * s] = std::cos(lat) * std::cos(lon);
      u[3 * s + 1] = std::cos(lat) * std::sin(lon);
      u[3 * s + 2] = std::sin(lat);
    } else {
      t.geo[3 * s] = u[3 * s] = x;
      t.geo[3 * s + 1] = u[3 * s + 1] = y;
      t.geo[3 * s + 2] = u[3 * s + 2] = 0.0;
    }
  }
  t.tile.clear();
  t.group.clear();
  for (int64_t a = 0; a < t.ntiles; ++a) t.tile.push_back(gw_bound(u, a * GW_T, std::min(count, (a + 1) * GW_T), metric));
  for (int64_t g = 0; g < t.ntiles; g += 16)
    t.group.push_back(gw_bound(u, g * GW_T, std::min(count, (g + 16) * GW_T), metric));
}

// Per chunk of centres: its tiles and the CSR list (ascending) of neighbour tiles that hold a weight > 0
struct GwChunk {
  int64_t first = 0, count = 0, off_tiles = 0, off_cols = 0;
  GwTiles c;
};

struct GwPlan {
  GwTiles nb;
  std::vector<GwChunk> chunks;
  std::vector<int> rowptr, cols;     // concatenated over the chunks (rowptr entries relative to the chunk's off_cols)
  int64_t visited = 0, possible = 0, ctiles = 0;
  int64_t first = 0;                 // the location range [first, first + count) of an unsorted plan (0 when sorted)
  bool sorted = false;
};

// sorted: the centres are ALL locations in the neighbours' Morton order, cut into chunks of `chunk` (a multiple of GW_T)
// sorted positions, so a chunk's tiles are the neighbour tiles themselves and spatially compact whatever the input order.
// Otherwise the centres are the locations [first, first + count) as ONE chunk, tiled among themselves.
inline void gw_plan(const double* xy, int64_t n, int64_t first, int64_t count, int64_t chunk, bool sorted, int metric, int kernel,
                    double bw, GwPlan& plan) {
  double box[4] = {xy[0], xy[0], xy[1], xy[1]};
  for (int64_t i = 0; i < n; ++i) {
    box[0] = std::min(box[0], xy[2 * i]);
    box[1] = std::max(box[1], xy[2 * i]);
    box[2] = std::min(box[2], xy[2 * i + 1]);
    box[3] = std::max(box[3], xy[2 * i + 1]);
  }
  gw_tile(xy, 0, n, metric, box, plan.nb);
  plan.sorted = sorted;
  plan.first = sorted ? 0 : first;
  if (!sorted) chunk = count;
  const int64_t ng = (int64_t)plan.nb.group.size();
  const int64_t lo = sorted ? 0 : first, hi = sorted ? n : first + count;
  for (int64_t c0 = lo; c0 < hi; c0 += chunk) {
    GwChunk ch;
    ch.first = c0;
    ch.count = std::min(chunk, hi - c0);
    ch.off_tiles = plan.ctiles;
    ch.off_cols = (int64_t)plan.cols.size();
    if (sorted) {
      GwTiles& t = ch.c;
      t.count = ch.count;
      t.ntiles = (ch.count + GW_T - 1) / GW_T;
      t.perm.assign(plan.nb.perm.begin() + c0, plan.nb.perm.begin() + c0 + ch.count);
      t.geo.assign(plan.nb.geo.begin() + 3 * c0, plan.nb.geo.begin() + 3 * (c0 + ch.count));
      t.tile.assign(plan.nb.tile.begin() + c0 / GW_T, plan.nb.tile.begin() + c0 / GW_T + t.ntiles);
    } else {
      gw_tile(xy, c0, ch.count, metric, box, ch.c);
    }
    for (int64_t a = 0; a < ch.c.ntiles; ++a) {
      plan.rowptr.push_back((int)((int64_t)plan.cols.size() - ch.off_cols));
      for (int64_t g = 0; g < ng; ++g) {
        if (gw_zero(gw_lower(ch.c.tile[a], plan.nb.group[g], metric), kernel, bw)) continue;
        for (int64_t t = g * 16; t < std::min(plan.nb.ntiles, (g + 1) * 16); ++t)
          if (!gw_zero(gw_lower(ch.c.tile[a], plan.nb.tile[t], metric), kernel, bw)) plan.cols.push_back((int)t);
      }
    }
    plan.rowptr.push_back((int)((int64_t)plan.cols.size() - ch.off_cols));
    plan.ctiles += ch.c.ntiles;
    plan.possible += ch.c.ntiles * plan.nb.ntiles;
    plan.chunks.push_back(std::move(ch));
  }
  plan.visited = (int64_t)plan.cols.size();
}

}  // namespace eofx
