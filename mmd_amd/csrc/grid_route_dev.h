// What the lane-per-query walk kernels share (grid_route.hip, route_seeds.hip and, through window_walk_dev.h, window_goals.hip and
// window_apart.hip): the status codes, the entry of a query, the lattice tile of a cell and the descent's step.  (The entry points'
// shared argument checks are host code: walk_args.h.)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"

namespace mmd {

constexpr int WALK_THREADS = 64;                           // one lane per query
constexpr int GRID_UNREACHED = MMD_GRID_DIST_UNREACHED;
// the status codes of mmd_grid_descend, which the window walks report as well (they have no tile list and never give WALK_TILES)
constexpr int WALK_OK = 0, WALK_UNREACHED_START = 1, WALK_STUCK = 2, WALK_TILES = 3, WALK_OUTSIDE = 4;

__device__ __forceinline__ long long floor_div(long long a, long long b) {     // b > 0
  const long long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// The entry of query q: its start cell s, its field f, the field's cells `dist` and d0 = dist[s].  The start and the field index are
// device data and may be anything: a start outside the grid or a field outside [0, n_fields) reads nothing (dist is then field 0's, never
// dereferenced) and gives d0 = GRID_UNREACHED.  A query with d0 == GRID_UNREACHED takes no walk, and `no_walk` is its status:
// WALK_OUTSIDE, or WALK_UNREACHED_START for a start of the grid that the field does not reach.
struct WalkEntry {
  int2 s;
  int f;
  const int* dist;
  int d0, no_walk;
};
__device__ __forceinline__ WalkEntry walk_entry(const int* __restrict__ dist_all, int nx, int ny, int n_fields, const int2* __restrict__ starts,
                                                const int* __restrict__ field, int q) {
  WalkEntry e;
  e.s = starts[q];
  e.f = field[q];
  const bool inside = e.f >= 0 && e.f < n_fields && e.s.x >= 0 && e.s.x < nx && e.s.y >= 0 && e.s.y < ny;
  e.dist = dist_all + (size_t)(inside ? e.f : 0) * nx * ny;
  e.d0 = inside ? e.dist[(size_t)e.s.x * ny + e.s.y] : GRID_UNREACHED;
  e.no_walk = inside ? WALK_UNREACHED_START : WALK_OUTSIDE;
  return e;
}

// One step of mmd_grid_descend's walk from cell (ix, iy), which holds d > 0, in lattice tile (ta, tb): the neighbours in the order +x,
// -x, +y, -y that lie inside the grid and hold exactly d - 1; the first of them in the tile, else the first.  Four scattered 4-byte loads.
// Returns 1 (stayed in the tile), 0 (entered another one: ta, tb are the new tile) or -1 (no candidate; nothing moved).
__device__ __forceinline__ int descend_step(const int* __restrict__ dist, int nx, int ny, int tile, int o_i, int o_j, int d, int& ix, int& iy,
                                            long long& ta, long long& tb) {
  int cx = -1, cy = -1;
  bool same = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int jx = ix + (k == 0) - (k == 1), jy = iy + (k == 2) - (k == 3);
    if (jx < 0 || jx >= nx || jy < 0 || jy >= ny || same) continue;
    if (dist[(size_t)jx * ny + jy] != d - 1) continue;
    const bool in_tile = floor_div((long long)jx - o_i, tile) == ta && floor_div((long long)jy - o_j, tile) == tb;
    if (cx < 0 || in_tile) { cx = jx; cy = jy; same = in_tile; }
  }
  if (cx < 0) return -1;
  ix = cx; iy = cy;
  if (same) return 1;
  ta = floor_div((long long)ix - o_i, tile);
  tb = floor_div((long long)iy - o_j, tile);
  return 0;
}

}  // namespace mmd
