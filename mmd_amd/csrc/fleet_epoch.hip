// World fleets: one sampler for a whole run.  Between two epochs its windows move in place (mmd_sdf_grid_windows_moved: sdf_grid.hip's
// clamped gather, which leaves alone every slice whose origin did not change) and its state -- offsets, sub-goal points, hard conditions,
// straight lines -- is written from the sub-goal launch's words on the device (mmd_fleet_epoch_frames), bit for bit what the host
// definitions give (include/mmd_amd.h names them operation by operation).  Plain loads and vector stores; no LDS, no atomics, no scratch,
// nothing that waits on another workgroup.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/mmd_amd.h"
#include "common.h"
// every float operation below is one rounding: no fused multiply-add
#pragma clang fp contract(off)

namespace mmd {

constexpr int FE_WIN_THREADS = 256;
constexpr int FE_POINTS = H;                   // a wave's 64 lanes are a line's 64 points
static_assert(FE_POINTS == 64, "one wave per robot, lane = time step");

// sdf_grid_windows_kernel (sdf_grid.hip) behind one test: the window is blockIdx.y, so its origin and the origin its slice holds are two
// wave-uniform 8-byte loads, and a workgroup of a window that did not move returns before it touches a texel.  The rest is that kernel
// line for line: the origin is device data and is clamped to [-nx, wnx] first, the source index per axis to the world, and the texel
// travels as four 32-bit words.  cell < n_cells = nx * ny and k < n_windows bound the store; the clamps bound the load.
__global__ __launch_bounds__(FE_WIN_THREADS) void sdf_grid_windows_moved_kernel(const uint4* __restrict__ world, int wnx, int wny,
                                                                                const int2* __restrict__ origins,
                                                                                const int2* __restrict__ held, int nx, int ny, int n_cells,
                                                                                uint4* __restrict__ windows) {
  const int k = blockIdx.y;
  const int2 o = origins[k];
  if (held) {
    const int2 h = held[k];
    if (h.x == o.x && h.y == o.y) return;
  }
  const int cell = blockIdx.x * FE_WIN_THREADS + threadIdx.x;
  if (cell >= n_cells) return;
  const int i0 = min(max(o.x, -nx), wnx), j0 = min(max(o.y, -ny), wny);
  const int ix = cell / ny, iy = cell - ix * ny;
  const int sx = min(max(i0 + ix, 0), wnx - 1), sy = min(max(j0 + iy, 0), wny - 1);
  windows[(size_t)k * n_cells + cell] = world[(size_t)sx * wny + sy];
}

struct FrameTerms {
  double cell, world_x, world_y, tile_x, tile_y;          // offsets: origin * cell + world - tile, in float64
  float lo_x, lo_y, pitch_x, pitch_y;                      // cell centres: lo + ((float)cell + 0.5f) * pitch
  float min[4], range[4];                                  // the normaliser: ((x - min) / range) * 2 - 1
};

__device__ __forceinline__ float normalised(float x, float lo, float range) { return ((x - lo) / range) * 2.f - 1.f; }

// One wave per robot, lane = time step.  Every lane computes the robot's few scalars (the loads are wave-uniform); lane t stores the
// line's point t, lane 0 the rest.  Nothing is indexed by a word read from cells, origins or summary.
__global__ __launch_bounds__(FE_POINTS) void fleet_epoch_frames_kernel(const int2* __restrict__ cells, const int2* __restrict__ origins,
                                                                       const int4* __restrict__ summary, const float2* __restrict__ points,
                                                                       int points_stride2, const float2* __restrict__ goal_points, FrameTerms f,
                                                                       const float* __restrict__ line_a, float2* __restrict__ offsets,
                                                                       float2* __restrict__ subgoals, float4* __restrict__ hard_first,
                                                                       float4* __restrict__ hard_last, float2* __restrict__ lines) {
  const int r = blockIdx.x, t = threadIdx.x;
  const int2 c = cells[r], o = origins[r];
  const float2 s = points[(size_t)r * points_stride2];       // (the stride in points: robot r's row, wherever the rows lie)
  const float2 off = make_float2((float)(((double)o.x * f.cell + f.world_x) - f.tile_x), (float)(((double)o.y * f.cell + f.world_y) - f.tile_y));
  float2 g = make_float2(f.lo_x + ((float)c.x + 0.5f) * f.pitch_x, f.lo_y + ((float)c.y + 0.5f) * f.pitch_y);
  if (summary[r].w == 1) g = goal_points[r];
  const float a = line_a[t], b = 1.f - a;
  lines[(size_t)r * FE_POINTS + t] = make_float2(s.x * b + g.x * a, s.y * b + g.y * a);
  if (t == 0) {
    const float vx = normalised(0.f, f.min[2], f.range[2]), vy = normalised(0.f, f.min[3], f.range[3]);
    offsets[r] = off;
    subgoals[r] = g;
    hard_first[r] = make_float4(normalised(s.x - off.x, f.min[0], f.range[0]), normalised(s.y - off.y, f.min[1], f.range[1]), vx, vy);
    hard_last[r] = make_float4(normalised(g.x - off.x, f.min[0], f.range[0]), normalised(g.y - off.y, f.min[1], f.range[1]), vx, vy);
  }
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_sdf_grid_windows_moved(const float* world_grid_dev, int wnx, int wny, const int32_t* origins_dev, const int32_t* held_dev,
                               int n_windows, int nx, int ny, float* windows_dev, void* stream) {
  MMD_REQUIRE(n_windows >= 0 && n_windows <= MMD_SDF_GRID_MAX_WINDOWS,
              "mmd_sdf_grid_windows_moved: n_windows = %d (0 to %d: the window is a block index)", n_windows, MMD_SDF_GRID_MAX_WINDOWS);
  MMD_REQUIRE(wnx >= 1 && wny >= 1, "mmd_sdf_grid_windows_moved: a world of %d x %d texels (at least 1 x 1)", wnx, wny);
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= wnx && ny <= wny,
              "mmd_sdf_grid_windows_moved: windows of %d x %d texels (1 x 1 up to the world's %d x %d)", nx, ny, wnx, wny);
  MMD_REQUIRE((long long)wnx * wny <= INT_MAX - FE_WIN_THREADS,
              "mmd_sdf_grid_windows_moved: a world of %d x %d texels does not fit a 32-bit index", wnx, wny);
  if (n_windows == 0) return 0;
  MMD_REQUIRE(world_grid_dev, "mmd_sdf_grid_windows_moved: NULL world grid");
  MMD_REQUIRE(origins_dev, "mmd_sdf_grid_windows_moved: NULL origins");
  MMD_REQUIRE(windows_dev, "mmd_sdf_grid_windows_moved: NULL windows");
  const int n_cells = nx * ny;                 // (<= wnx * wny)
  hipLaunchKernelGGL(sdf_grid_windows_moved_kernel, dim3((n_cells + FE_WIN_THREADS - 1) / FE_WIN_THREADS, n_windows), dim3(FE_WIN_THREADS),
                     0, (hipStream_t)stream, (const uint4*)world_grid_dev, wnx, wny, (const int2*)origins_dev, (const int2*)held_dev, nx,
                     ny, n_cells, (uint4*)windows_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_fleet_epoch_frames(const int32_t* cells_dev, const int32_t* origins_dev, const int32_t* summary_dev, const float* points_dev,
                           int points_stride, const float* goal_points_dev, int n_robots, const double offset_terms[5],
                           const float centre_terms[4], const float norm_min[4], const float norm_range[4], const float* line_a_dev, float* offsets_dev,
                           float* subgoals_dev, float* hard_first_dev, float* hard_last_dev, float* lines_dev, void* stream) {
  MMD_REQUIRE(n_robots >= 0, "mmd_fleet_epoch_frames: n_robots = %d (>= 0)", n_robots);
  MMD_REQUIRE(points_stride >= 2 && points_stride % 2 == 0, "mmd_fleet_epoch_frames: points_stride = %d floats (even, at least 2)", points_stride);
  MMD_REQUIRE(offset_terms && centre_terms && norm_min && norm_range, "mmd_fleet_epoch_frames: NULL offset_terms, centre_terms, norm_min or norm_range");
  if (n_robots == 0) return 0;
  const auto aligned = [](const void* p, uintptr_t to) { return p && (uintptr_t)p % to == 0; };
  MMD_REQUIRE(aligned(cells_dev, 8) && aligned(origins_dev, 8) && aligned(summary_dev, 16),
              "mmd_fleet_epoch_frames: cells and origins (8-byte aligned) and summary (16-byte aligned), none NULL");
  MMD_REQUIRE(aligned(points_dev, 8) && aligned(goal_points_dev, 8), "mmd_fleet_epoch_frames: points and goal points (8-byte aligned), none NULL");
  MMD_REQUIRE(aligned(line_a_dev, 4), "mmd_fleet_epoch_frames: NULL or misaligned line parameters");
  MMD_REQUIRE(aligned(offsets_dev, 8) && aligned(subgoals_dev, 8) && aligned(lines_dev, 8),
              "mmd_fleet_epoch_frames: offsets, sub-goals and lines (8-byte aligned), none NULL");
  MMD_REQUIRE(aligned(hard_first_dev, 16) && aligned(hard_last_dev, 16), "mmd_fleet_epoch_frames: hard conditions (16-byte aligned), none NULL");
  FrameTerms f;
  f.cell = offset_terms[0], f.world_x = offset_terms[1], f.world_y = offset_terms[2], f.tile_x = offset_terms[3], f.tile_y = offset_terms[4];
  f.lo_x = centre_terms[0], f.lo_y = centre_terms[1], f.pitch_x = centre_terms[2], f.pitch_y = centre_terms[3];
  for (int k = 0; k < 4; ++k) f.min[k] = norm_min[k], f.range[k] = norm_range[k];
  hipLaunchKernelGGL(fleet_epoch_frames_kernel, dim3(n_robots), dim3(FE_POINTS), 0, (hipStream_t)stream, (const int2*)cells_dev,
                     (const int2*)origins_dev, (const int4*)summary_dev, (const float2*)points_dev, points_stride / 2, (const float2*)goal_points_dev, f,
                     line_a_dev, (float2*)offsets_dev, (float2*)subgoals_dev, (float4*)hard_first_dev, (float4*)hard_last_dev,
                     (float2*)lines_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
