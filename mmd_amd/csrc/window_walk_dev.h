// What the walk kernels of a world fleet share (window_goals.hip, window_apart.hip): the step rule of
// mmd_amd/fleet_subgoals.py::window_goal on grid_route_dev.h's entry of a query and status codes, the walk, the window's origin.  Every
// value is an exact integer.  (The entry points' shared argument checks are host code: walk_args.h.)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"
#include "grid_route_dev.h"

namespace mmd {

constexpr int WG_THREADS = WALK_THREADS;

// One step of the walk from cell (ix, iy), whose neighbours on a shortest path hold `want` (= d - 1, d >= 1 the cell's own value): the
// neighbours that lie inside the grid and hold exactly `want`, the first of +x, -x and the first of +y, -y; the axis on which the
// field's goal g is farther from the current cell goes first (x on a tie), the other axis serves where that one has no candidate; no step
// is taken that would leave the box of Chebyshev radius `reach` round the start s.  g is device data: any two words (the differences are
// taken in 64 bits).  Four scattered 4-byte loads.  Returns 1 (stepped: ix, iy are the next cell), 0 (the next cell lies outside the box;
// nothing moved) or -1 (no candidate: the field was not converged; nothing moved).
__device__ __forceinline__ int window_step(const int* __restrict__ dist, int nx, int ny, int2 s, int2 g, int reach, int want, int& ix,
                                           int& iy) {
  const bool xp = ix + 1 < nx && dist[(size_t)(ix + 1) * ny + iy] == want;
  const bool xm = ix > 0 && dist[(size_t)(ix - 1) * ny + iy] == want;
  const bool yp = iy + 1 < ny && dist[(size_t)ix * ny + iy + 1] == want;
  const bool ym = iy > 0 && dist[(size_t)ix * ny + iy - 1] == want;
  const int sx = xp ? 1 : xm ? -1 : 0, sy = yp ? 1 : ym ? -1 : 0;      // the first candidate of each axis, 0: none
  if (sx == 0 && sy == 0) return -1;
  const long long ax = llabs((long long)g.x - ix), ay = llabs((long long)g.y - iy);
  const bool along_x = sx != 0 && (ax >= ay || sy == 0);
  const int jx = along_x ? ix + sx : ix, jy = along_x ? iy : iy + sy;
  if (max(abs(jx - s.x), abs(jy - s.y)) > reach) return 0;
  ix = jx; iy = jy;
  return 1;
}

// The walk of a query from s with d0 = dist[s] != GRID_UNREACHED: at most min(max_steps, d0) steps (d falls by one per step, so the loop
// counter IS d0 - d; d0 <= 0: no step).  (ix, iy) is the last cell reached, `steps` the steps taken; returns WALK_OK or WALK_STUCK.
__device__ __forceinline__ int window_walk(const int* __restrict__ dist, int nx, int ny, int2 s, int2 g, int reach, int max_steps, int d0,
                                           int& ix, int& iy, int& steps) {
  ix = s.x; iy = s.y; steps = 0;
  const int bound = min(max_steps, d0);
  for (int k = 0; k < bound; ++k) {
    const int r = window_step(dist, nx, ny, s, g, reach, d0 - k - 1, ix, iy);
    if (r < 0) return WALK_STUCK;
    if (r == 0) break;
    ++steps;
  }
  return WALK_OK;
}

// the origin cell of the window of `window` cells per side round the start s, clamped to the grid
__device__ __forceinline__ int2 window_origin(int2 s, int nx, int ny, int window) {
  return make_int2(min(max(s.x - window / 2, 0), nx - window), min(max(s.y - window / 2, 0), ny - window));
}

}  // namespace mmd
