// World fleets: every robot's next sub-goal and window, read off its goal's distance field (include/mmd_amd.h: mmd_grid_window_goals).
// The definition is the numpy function window_goal of mmd_amd/world_fleet.py, where the two facts a fleet rests on (containment of the
// walk's box in the window, progress per call) are stated and argued; every value here is an exact integer.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mmd_amd.h"
#include "common.h"
#include "window_walk_dev.h"

namespace mmd {

// One lane per query.  From the start cell c0 with d0 = dist[c0], at most min(max_steps, d0) times: one step of the rule (window_walk_dev.h:
// window_step); the walk ends before a step that would leave the box of Chebyshev radius `reach` round c0.  The lanes of a wave walk
// unrelated cells: four scattered 4-byte loads per step and lane, no LDS, no atomics, nothing that waits on another workgroup.
__global__ __launch_bounds__(WG_THREADS) void grid_window_goals_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                       const int2* __restrict__ starts, const int* __restrict__ field,
                                                                       const int2* __restrict__ goals, int n_queries, int reach,
                                                                       int max_steps, int window, int2* __restrict__ cells,
                                                                       int2* __restrict__ origins, int4* __restrict__ summary) {
  const int q = blockIdx.x * WG_THREADS + threadIdx.x;
  if (q >= n_queries) return;
  const int2 s = starts[q];
  const int f = field[q];
  const bool inside = f >= 0 && f < n_fields && s.x >= 0 && s.x < nx && s.y >= 0 && s.y < ny;
  const int* dist = dist_all + (size_t)(inside ? f : 0) * nx * ny;
  const int d0 = inside ? dist[(size_t)s.x * ny + s.y] : WG_UNREACHED;
  if (d0 == WG_UNREACHED) {
    cells[q] = make_int2(0, 0);
    origins[q] = make_int2(0, 0);
    summary[q] = make_int4(-1, -1, inside ? WG_UNREACHED_START : WG_OUTSIDE, 0);
    return;
  }
  int ix, iy, steps;
  const int status = window_walk(dist, nx, ny, s, goals[f], reach, max_steps, d0, ix, iy, steps);
  const int remaining = d0 - steps;
  cells[q] = make_int2(ix, iy);
  origins[q] = window_origin(s, nx, ny, window);
  summary[q] = make_int4(steps, remaining, status, status == WG_OK && remaining == 0);
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_grid_window_goals(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev, const int32_t* field_dev,
                          const int32_t* goals_dev, int n_queries, int reach, int max_steps, int window, int32_t* cells_dev,
                          int32_t* origins_dev, int32_t* summary_dev, void* stream) {
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "mmd_grid_window_goals: a grid of %d x %d cells (1 to %d per side)", nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(n_fields >= 0, "mmd_grid_window_goals: n_fields = %d (>= 0)", n_fields);
  MMD_REQUIRE(n_queries >= 0 && n_queries <= INT_MAX - WG_THREADS, "mmd_grid_window_goals: n_queries = %d (0 to 2^31 - 65)", n_queries);
  MMD_REQUIRE(window >= 1 && window <= nx && window <= ny, "mmd_grid_window_goals: window = %d cells (1 to min(nx, ny) = %d)", window,
              nx < ny ? nx : ny);
  MMD_REQUIRE(reach >= 1 && reach <= window / 2 - 1, "mmd_grid_window_goals: reach = %d cells (1 to window / 2 - 1 = %d)", reach,
              window / 2 - 1);
  MMD_REQUIRE(max_steps >= 1, "mmd_grid_window_goals: max_steps = %d (>= 1)", max_steps);
  if (n_queries == 0) return 0;
  MMD_REQUIRE(dist_dev || n_fields == 0, "mmd_grid_window_goals: NULL dist with n_fields = %d", n_fields);
  MMD_REQUIRE(goals_dev || n_fields == 0, "mmd_grid_window_goals: NULL goals with n_fields = %d", n_fields);
  MMD_REQUIRE(starts_dev, "mmd_grid_window_goals: NULL starts");
  MMD_REQUIRE(field_dev, "mmd_grid_window_goals: NULL field indices");
  MMD_REQUIRE(cells_dev, "mmd_grid_window_goals: NULL cells");
  MMD_REQUIRE(origins_dev, "mmd_grid_window_goals: NULL origins");
  MMD_REQUIRE(summary_dev, "mmd_grid_window_goals: NULL summary");
  hipLaunchKernelGGL(grid_window_goals_kernel, dim3((n_queries + WG_THREADS - 1) / WG_THREADS), dim3(WG_THREADS), 0, (hipStream_t)stream,
                     (const int*)dist_dev, nx, ny, n_fields, (const int2*)starts_dev, (const int*)field_dev, (const int2*)goals_dev,
                     n_queries, reach, max_steps, window, (int2*)cells_dev, (int2*)origins_dev, (int4*)summary_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
