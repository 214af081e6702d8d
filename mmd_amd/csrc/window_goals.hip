// World fleets: every robot's next sub-goal and window, read off its goal's distance field, alone or with the 64 support cells of the
// walk's cell path (include/mmd_amd.h: mmd_grid_window_goals, mmd_grid_window_goal_samples).  The definitions are the numpy functions
// window_goal and window_goal_samples of mmd_amd/fleet_subgoals.py, where the two facts a fleet rests on (containment of the walk's box in the
// window, progress per call) are stated and argued; every value here is an exact integer.  Plain loads and vector stores; no LDS, no
// atomics, no scratch.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mmd_amd.h"
#include "common.h"
#include "seed_dev.h"
#include "walk_args.h"
#include "window_walk_dev.h"

namespace mmd {

static_assert(MMD_ROUTE_SEED_POINTS == 64, "a walk has 64 support cells");

// One lane per query, the body of both kernels.  From the start cell c0 with d0 = dist[c0] (grid_route_dev.h: walk_entry), at most
// min(max_steps, d0) times: one step of the rule (window_walk_dev.h: window_step); the walk ends before a step that would leave the box of
// Chebyshev radius `reach` round c0.  The lanes of a wave walk unrelated cells: four scattered 4-byte loads per step and lane, nothing
// that waits on another workgroup.
// SAMPLES: the lane walks the field twice, with no buffer proportional to the path (grid_descend_samples_kernel's way): the first walk
// fixes `steps`; the second, only for status 0, repeats it and emits sample j when it stands on the path's cell number
// off(j) = (j * steps + 31) / 63, monotone in j: one advancing cursor (seed_dev.h: emit_samples, on a path of steps + 1 cells).  The cursor
// counts in 64 bits, though int32 would hold here: a step lands on a cell that holds one less than the cell before, so the cells of a walk
// are distinct and steps <= d0 < nx * ny <= 2048^2 = 2^22, whatever the field holds; 63 * steps + 31 and (steps + 1) * 63 stay below
// 2^28 + 63.  Each walk's loop runs at most min(max_steps, d0) times, the second one `steps` times; the cursor only grows, 64 emissions in
// all.  Every word of the outputs of the query is written.
template <bool SAMPLES>
__device__ __forceinline__ void window_goals_query(const int* __restrict__ dist_all, int nx, int ny, int n_fields, const int2* __restrict__ starts,
                                                   const int* __restrict__ field, const int2* __restrict__ goals, int n_queries, int reach,
                                                   int max_steps, int window, int2* __restrict__ cells, int2* __restrict__ origins,
                                                   int4* __restrict__ summary, int2* __restrict__ samples) {
  const int q = blockIdx.x * WG_THREADS + threadIdx.x;
  if (q >= n_queries) return;
  const WalkEntry e = walk_entry(dist_all, nx, ny, n_fields, starts, field, q);
  int2* row = SAMPLES ? samples + (size_t)q * MMD_ROUTE_SEED_POINTS : nullptr;
  int status = e.no_walk, steps = 0;
  int2 g = make_int2(0, 0);
  if (e.d0 == GRID_UNREACHED) {
    cells[q] = make_int2(0, 0);
    origins[q] = make_int2(0, 0);
    summary[q] = make_int4(-1, -1, status, 0);
  } else {
    g = goals[e.f];
    int ix, iy;
    status = window_walk(e.dist, nx, ny, e.s, g, reach, max_steps, e.d0, ix, iy, steps);
    const int remaining = e.d0 - steps;
    cells[q] = make_int2(ix, iy);
    origins[q] = window_origin(e.s, nx, ny, window);
    summary[q] = make_int4(steps, remaining, status, status == WALK_OK && remaining == 0);
  }
  if (!SAMPLES) return;
  if (status != WALK_OK) {                                 // a walk that did not end well gives no samples
    for (int j = 0; j < MMD_ROUTE_SEED_POINTS; ++j) row[j] = make_int2(0, 0);
    return;
  }

  int ix = e.s.x, iy = e.s.y, j = 0;
  for (int t = 0;; ++t) {                                  // t = 0 .. steps: the path's cell number
    emit_samples(row, j, steps + 1, t, ix, iy);
    if (t >= steps) break;
    if (window_step(e.dist, nx, ny, e.s, g, reach, e.d0 - t - 1, ix, iy) != 1) break;      // (the first walk passed here)
  }
  for (; j < MMD_ROUTE_SEED_POINTS; ++j) row[j] = make_int2(ix, iy);   // (none left: off(63) = steps.  It keeps "every word is written" off that argument)
}

__global__ __launch_bounds__(WG_THREADS) void grid_window_goals_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                       const int2* __restrict__ starts, const int* __restrict__ field,
                                                                       const int2* __restrict__ goals, int n_queries, int reach,
                                                                       int max_steps, int window, int2* __restrict__ cells,
                                                                       int2* __restrict__ origins, int4* __restrict__ summary) {
  window_goals_query<false>(dist_all, nx, ny, n_fields, starts, field, goals, n_queries, reach, max_steps, window, cells, origins, summary,
                            nullptr);
}

__global__ __launch_bounds__(WG_THREADS) void grid_window_goal_samples_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                              const int2* __restrict__ starts, const int* __restrict__ field,
                                                                              const int2* __restrict__ goals, int n_queries, int reach,
                                                                              int max_steps, int window, int2* __restrict__ cells,
                                                                              int2* __restrict__ origins, int4* __restrict__ summary,
                                                                              int2* __restrict__ samples) {
  window_goals_query<true>(dist_all, nx, ny, n_fields, starts, field, goals, n_queries, reach, max_steps, window, cells, origins, summary,
                           samples);
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_grid_window_goals(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev, const int32_t* field_dev,
                          const int32_t* goals_dev, int n_queries, int reach, int max_steps, int window, int32_t* cells_dev,
                          int32_t* origins_dev, int32_t* summary_dev, void* stream) {
  const char* name = "mmd_grid_window_goals";
  if (const int refused = window_goals_ranges(name, nx, ny, n_fields, n_queries, reach, max_steps, 0, window)) return refused;
  if (n_queries == 0) return 0;
  if (const int refused = window_goals_inputs(name, dist_dev, goals_dev, n_fields, starts_dev, field_dev)) return refused;
  if (const int refused = window_goals_outputs(name, cells_dev, origins_dev, summary_dev)) return refused;
  hipLaunchKernelGGL(grid_window_goals_kernel, dim3((n_queries + WG_THREADS - 1) / WG_THREADS), dim3(WG_THREADS), 0, (hipStream_t)stream,
                     (const int*)dist_dev, nx, ny, n_fields, (const int2*)starts_dev, (const int*)field_dev, (const int2*)goals_dev,
                     n_queries, reach, max_steps, window, (int2*)cells_dev, (int2*)origins_dev, (int4*)summary_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_grid_window_goal_samples(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev, const int32_t* field_dev,
                                 const int32_t* goals_dev, int n_queries, int reach, int max_steps, int window, int32_t* cells_dev,
                                 int32_t* origins_dev, int32_t* summary_dev, int32_t* samples_dev, void* stream) {
  const char* name = "mmd_grid_window_goal_samples";
  if (const int refused = window_goals_ranges(name, nx, ny, n_fields, n_queries, reach, max_steps, 0, window)) return refused;
  if (n_queries == 0) return 0;
  if (const int refused = window_goals_inputs(name, dist_dev, goals_dev, n_fields, starts_dev, field_dev)) return refused;
  if (const int refused = window_goals_outputs(name, cells_dev, origins_dev, summary_dev)) return refused;
  MMD_REQUIRE(samples_dev, "mmd_grid_window_goal_samples: NULL samples");
  hipLaunchKernelGGL(grid_window_goal_samples_kernel, dim3((n_queries + WG_THREADS - 1) / WG_THREADS), dim3(WG_THREADS), 0,
                     (hipStream_t)stream, (const int*)dist_dev, nx, ny, n_fields, (const int2*)starts_dev, (const int*)field_dev,
                     (const int2*)goals_dev, n_queries, reach, max_steps, window, (int2*)cells_dev, (int2*)origins_dev, (int4*)summary_dev,
                     (int2*)samples_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
