// Host only: the argument checks that the entry points of the lane-per-query walk kernels share, each under the caller's name, so that
// every message keeps its prefix.  A function returns 0, or 2 with the error set; the caller returns what is not 0.  The order of an
// entry point's checks is: shapes and ranges (the shared ones, then its own), `if (n_queries == 0) return 0;`, then the pointers.
#pragma once
#include <climits>
#include <cstdint>

#include "../../include/mmd_amd.h"
#include "common.h"

namespace mmd {

constexpr int WALK_ARGS_THREADS = 64;                      // the walk kernels' workgroup: n_queries + 63 must not overflow

inline bool origin_ok(const int32_t o[2]) { return o[0] >= -(1 << 30) && o[0] <= (1 << 30) && o[1] >= -(1 << 30) && o[1] <= (1 << 30); }

// ---- mmd_grid_descend, mmd_grid_descend_samples: all their shared checks (both have their own pointers behind them) ----
// max_tiles_cap: 0 = none
inline int descend_args(const char* name, const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev,
                        const int32_t* field_dev, int n_queries, int tile, const int32_t lattice_origin[2], int max_tiles, int max_tiles_cap,
                        const int32_t* tiles_dev, const int32_t* summary_dev) {
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "%s: a grid of %d x %d cells (1 to %d per side)", name, nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(n_fields >= 0, "%s: n_fields = %d (>= 0)", name, n_fields);
  MMD_REQUIRE(n_queries >= 0 && n_queries <= INT_MAX - WALK_ARGS_THREADS, "%s: n_queries = %d (0 to 2^31 - 65)", name, n_queries);
  MMD_REQUIRE(tile >= 1, "%s: tile = %d cells (>= 1)", name, tile);
  if (max_tiles_cap)
    MMD_REQUIRE(max_tiles >= 1 && max_tiles <= max_tiles_cap, "%s: max_tiles = %d (1 to %d)", name, max_tiles, max_tiles_cap);
  else
    MMD_REQUIRE(max_tiles >= 1, "%s: max_tiles = %d (>= 1)", name, max_tiles);
  MMD_REQUIRE(lattice_origin, "%s: NULL lattice_origin", name);
  MMD_REQUIRE(origin_ok(lattice_origin), "%s: lattice_origin = (%d, %d) (each within +-2^30: a tile index is then an int32)", name,
              lattice_origin[0], lattice_origin[1]);
  if (n_queries == 0) return 0;
  MMD_REQUIRE(dist_dev || n_fields == 0, "%s: NULL dist with n_fields = %d", name, n_fields);
  MMD_REQUIRE(starts_dev, "%s: NULL starts", name);
  MMD_REQUIRE(field_dev, "%s: NULL field indices", name);
  MMD_REQUIRE(tiles_dev, "%s: NULL tiles", name);
  MMD_REQUIRE(summary_dev, "%s: NULL summary", name);
  return 0;
}

// ---- mmd_grid_window_goals, mmd_grid_window_goal_samples, mmd_grid_window_goals_apart: ranges, input pointers, output pointers ----
// Three parts, because the apart entry point has checks of its own between them: sep and n_sweeps behind the ranges, the workspace
// between the inputs and the outputs.  max_steps_cap: 0 = none.
inline int window_goals_ranges(const char* name, int nx, int ny, int n_fields, int n_queries, int reach, int max_steps, int max_steps_cap,
                               int window) {
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "%s: a grid of %d x %d cells (1 to %d per side)", name, nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(n_fields >= 0, "%s: n_fields = %d (>= 0)", name, n_fields);
  MMD_REQUIRE(n_queries >= 0 && n_queries <= INT_MAX - WALK_ARGS_THREADS, "%s: n_queries = %d (0 to 2^31 - 65)", name, n_queries);
  MMD_REQUIRE(window >= 1 && window <= nx && window <= ny, "%s: window = %d cells (1 to min(nx, ny) = %d)", name, window, nx < ny ? nx : ny);
  MMD_REQUIRE(reach >= 1 && reach <= window / 2 - 1, "%s: reach = %d cells (1 to window / 2 - 1 = %d)", name, reach, window / 2 - 1);
  if (max_steps_cap)
    MMD_REQUIRE(max_steps >= 1 && max_steps <= max_steps_cap, "%s: max_steps = %d (1 to %d: a row of the workspace)", name, max_steps,
                max_steps_cap);
  else
    MMD_REQUIRE(max_steps >= 1, "%s: max_steps = %d (>= 1)", name, max_steps);
  return 0;
}

inline int window_goals_inputs(const char* name, const int32_t* dist_dev, const int32_t* goals_dev, int n_fields, const int32_t* starts_dev,
                               const int32_t* field_dev) {
  MMD_REQUIRE(dist_dev || n_fields == 0, "%s: NULL dist with n_fields = %d", name, n_fields);
  MMD_REQUIRE(goals_dev || n_fields == 0, "%s: NULL goals with n_fields = %d", name, n_fields);
  MMD_REQUIRE(starts_dev, "%s: NULL starts", name);
  MMD_REQUIRE(field_dev, "%s: NULL field indices", name);
  return 0;
}

inline int window_goals_outputs(const char* name, const int32_t* cells_dev, const int32_t* origins_dev, const int32_t* summary_dev) {
  MMD_REQUIRE(cells_dev, "%s: NULL cells", name);
  MMD_REQUIRE(origins_dev, "%s: NULL origins", name);
  MMD_REQUIRE(summary_dev, "%s: NULL summary", name);
  return 0;
}

}  // namespace mmd
