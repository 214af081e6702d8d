// World fleets: the seed trajectory of an epoch.  From the 64 support cells of every robot's walk (window_goals.hip:
// mmd_grid_window_goal_samples, or window_apart.hip's shortened walks) every robot's smoothed chain of support points with velocities
// inside its own window, in trajs_final's format (include/mmd_amd.h: mmd_window_seeds).  The definition is the numpy function window_seed
// of mmd_amd/fleet_subgoals.py: the same float32 bits.  Plain loads and vector stores; no LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/mmd_amd.h"
#include "common.h"
#include "seed_dev.h"
#include "wave_dev.h"
#include "window_walk_dev.h"
// every float operation below is one rounding: no fused multiply-add
#pragma clang fp contract(off)

namespace mmd {

constexpr int WS_POINTS = MMD_ROUTE_SEED_POINTS;            // support points of a seed: one wave
static_assert(WS_POINTS == 64 && WS_POINTS == WG_THREADS, "a wave's 64 lanes are a seed's 64 support points");

// ---- the seed: one wave per robot ----
// Lane j is support point j and keeps its point in registers.  An iteration reads both neighbours' points of the iteration before across
// lanes (__shfl_up / __shfl_down by 1: every lane reads before any lane writes, so this is the Jacobi iteration of the definition, with no
// LDS and no barrier), forms the candidate, gathers one texel (4 bytes of the float4 texture) and accepts the candidate iff its value
// exceeds the clearance and the texel is a cell of the robot's window [origin, origin + window) per axis.  Lanes 0 and 63 hold the
// caller's exact points throughout.  The loop runs smooth_iters times; its chain of dependent steps per iteration is two lane reads, the
// texel arithmetic and one gather.  The samples and the origin are device data: any words.  A sample is only converted to a float; the
// gather's index is seed_texel's, clamped to the grid whatever the point holds (a NaN: index 0); the window test is taken in 64 bits.
__global__ __launch_bounds__(WS_POINTS) void window_seeds_kernel(const float4* __restrict__ tex, SeedGrid g, float clearance,
                                                                 const int2* __restrict__ samples, const int2* __restrict__ origins,
                                                                 const int4* __restrict__ summary, int window,
                                                                 const float2* __restrict__ start_points, const float2* __restrict__ goal_points,
                                                                 int smooth_iters, float two_dt, float4* __restrict__ seeds,
                                                                 int* __restrict__ clear_min) {
  const int robot = blockIdx.x, j = threadIdx.x;
  float4* out = seeds + (size_t)robot * WS_POINTS;
  if (summary[robot].z != WALK_OK) {                         // one decision per wave: no chain, no texture read
    out[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j == 0) clear_min[robot] = 0;
    return;
  }
  const int2 c = samples[(size_t)robot * WS_POINTS + j];
  const int2 o = origins[robot];
  const long long lo_i = o.x, lo_j = o.y, hi_i = (long long)o.x + window, hi_j = (long long)o.y + window;
  float2 p = make_float2(g.lo_x + ((float)c.x + 0.5f) * g.pitch_x, g.lo_y + ((float)c.y + 0.5f) * g.pitch_y);
  if (j == 0) p = start_points[robot];
  if (j == WS_POINTS - 1) p = goal_points[robot];
  const bool interior = j > 0 && j < WS_POINTS - 1;

  for (int it = 0; it < smooth_iters; ++it) {
    const float2 a = make_float2(__shfl_up(p.x, 1), __shfl_up(p.y, 1)), b = make_float2(__shfl_down(p.x, 1), __shfl_down(p.y, 1));
    if (interior) {
      const float2 m = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y + b.y));
      const int2 x = seed_texel(g, m);
      const bool clear = tex[(size_t)x.x * g.ny + x.y].x > clearance;
      const bool in_window = x.x >= lo_i && x.x < hi_i && x.y >= lo_j && x.y < hi_j;
      if (clear && in_window) p = m;
    }
  }

  const float2 a = make_float2(__shfl_up(p.x, 1), __shfl_up(p.y, 1)), b = make_float2(__shfl_down(p.x, 1), __shfl_down(p.y, 1));
  const float2 v = interior ? make_float2((b.x - a.x) / two_dt, (b.y - a.y) / two_dt) : make_float2(0.f, 0.f);
  out[j] = make_float4(p.x, p.y, v.x, v.y);
  const int2 x = seed_texel(g, p);
  const int key = wave_min(order_key(__float_as_int(tex[(size_t)x.x * g.ny + x.y].x)));
  if (j == 0) clear_min[robot] = order_key(key);
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_window_seeds(const float* grid_dev, int nx, int ny, const float lo[2], const float hi[2], float clearance, const int32_t* samples_dev,
                     const int32_t* origins_dev, const int32_t* summary_dev, int n_robots, int window, const float* start_points_dev,
                     const float* goal_points_dev, int smooth_iters, float two_dt, float* seeds_dev, float* clear_min_dev, void* stream) {
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "mmd_window_seeds: a grid of %d x %d cells (1 to %d per side)", nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(lo && hi, "mmd_window_seeds: NULL limits");
  const float dim_x = fabsf(hi[0] - lo[0]), dim_y = fabsf(hi[1] - lo[1]);
  MMD_REQUIRE(fabsf(lo[0]) <= FLT_MAX && fabsf(lo[1]) <= FLT_MAX && dim_x > 0.f && dim_x <= FLT_MAX && dim_y > 0.f && dim_y <= FLT_MAX,
              "mmd_window_seeds: limits (%g, %g) .. (%g, %g) (finite, a non-zero extent per axis)", (double)lo[0], (double)lo[1], (double)hi[0],
              (double)hi[1]);
  MMD_REQUIRE(fabsf(clearance) <= FLT_MAX, "mmd_window_seeds: clearance = %g (finite)", (double)clearance);
  MMD_REQUIRE(two_dt > 0.f && two_dt <= FLT_MAX, "mmd_window_seeds: two_dt = %g (finite, > 0)", (double)two_dt);
  MMD_REQUIRE(smooth_iters >= 0, "mmd_window_seeds: smooth_iters = %d (>= 0)", smooth_iters);
  MMD_REQUIRE(n_robots >= 0, "mmd_window_seeds: n_robots = %d (>= 0)", n_robots);
  MMD_REQUIRE(window >= 1, "mmd_window_seeds: window = %d cells (>= 1)", window);
  if (n_robots == 0) return 0;
  MMD_REQUIRE(grid_dev, "mmd_window_seeds: NULL grid");
  MMD_REQUIRE(samples_dev, "mmd_window_seeds: NULL samples");
  MMD_REQUIRE(origins_dev, "mmd_window_seeds: NULL origins");
  MMD_REQUIRE(summary_dev, "mmd_window_seeds: NULL summary");
  MMD_REQUIRE(start_points_dev && goal_points_dev, "mmd_window_seeds: NULL start or goal points");
  MMD_REQUIRE(seeds_dev, "mmd_window_seeds: NULL seeds");
  MMD_REQUIRE(clear_min_dev, "mmd_window_seeds: NULL clear_min");
  const SeedGrid g = {nx, ny, lo[0], lo[1], dim_x, dim_y, dim_x / (float)nx, dim_y / (float)ny};
  hipLaunchKernelGGL(window_seeds_kernel, dim3(n_robots), dim3(WS_POINTS), 0, (hipStream_t)stream, (const float4*)grid_dev, g, clearance,
                     (const int2*)samples_dev, (const int2*)origins_dev, (const int4*)summary_dev, window, (const float2*)start_points_dev,
                     (const float2*)goal_points_dev, smooth_iters, two_dt, (float4*)seeds_dev, (int*)clear_min_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
