// World fleets: the report of a whole run (include/mmd_amd.h: mmd_fleet_run_report).  The paths [n][L][2] of a run against the map they
// were planned on -- every waypoint and n_interp interior points of every segment --, against each other at every column, and against
// their goals, into ONE buffer that the host reads with one copy.  The definition is the numpy function run_report of
// mmd_amd/fleet_report.py: the same integers and the same float32 bits (`length` apart: a float sum, whose order is fixed here and
// is not the definition's).  Two kernels: one wave per robot over its columns, and all pairs of robots over tiles of
// FR_TILE robots x 64 columns staged in LDS.  Integer atomics only: every count is order-independent.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/mmd_amd.h"
#include "collision_dev.h"        // torch_norm2 / rr_hit; sets fp contract(off)
#include "common.h"
#include "seed_dev.h"             // seed_texel (mmd_sdf_grid_lookup's sequence), order_key
#include "wave_dev.h"             // wave_sum / wave_min / wave_max: the fixed order
// every float operation below is one rounding: no fused multiply-add but torch_norm2's own
#pragma clang fp contract(off)

namespace mmd {

constexpr int FR_TILE = 32;                                  // robots per tile of the pair kernel: 2 tiles x 32 rows x 64 float2 = 32 KB of LDS
constexpr int FR_CANONICAL_NAN = 0x7fc00000;
static_assert(MMD_FLEET_REPORT_MAX_ROBOTS <= 1 << 12 && MMD_FLEET_REPORT_MAX_LENGTH < 1 << 16, "the first conflict's key packs (t, i, j) as 16 + 12 + 12 bits");

__device__ __forceinline__ bool finite2(float2 p) { return fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX; }

// ---- per robot: one wave per robot, lanes over 64 consecutive columns, chunk by chunk (agent_stats_kernel's walk) ----
// Lane l of chunk t0 holds waypoint t = t0 + l and segment t (to waypoint t + 1: the lane above's, or for lane 63 the first row of the
// next chunk).  A lane gathers its waypoint's texel and the texels of its segment's interior points; no lane reads another's gathers.
// first_hit and arrival come from one ballot each per chunk: first_hit the first set bit of the first chunk that has one, arrival the
// column behind the last column that is not on the goal.  No LDS; the only atomics are the two per-run robot counts.
__global__ __launch_bounds__(256) void fleet_robot_report_kernel(const float2* __restrict__ paths, int n, int L, const float4* __restrict__ tex,
                                                                  SeedGrid g, float hi_x, float hi_y, const float2* __restrict__ goals,
                                                                  float margin, int n_interp, float goal_tol, int* __restrict__ header,
                                                                  int* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  const int robot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (robot >= n) return;                                      // (whole waves leave together)
  const float2* path = paths + (size_t)robot * L;
  const float2 goal = goals[robot];
  const float parts = (float)(n_interp + 1);
  int points_hit = 0, interp_hit = 0, bad = 0, outside = 0, first_hit = -1, arrival = 0;
  int clear_key = 0x7f800000;                                  // order_key of +inf
  int max_bits = 0;                                            // a segment length is >= 0 and no NaN: its bits order as an int
  float len = 0.f;
  for (int t0 = 0; t0 < L; t0 += 64) {
    const int t = t0 + lane;
    const bool valid = t < L;
    const float2 cur = path[valid ? t : L - 1];
    float2 nxt = make_float2(__shfl_down(cur.x, 1), __shfl_down(cur.y, 1));
    if (lane == 63 && t + 1 < L) nxt = path[t + 1];            // the first row of the next chunk
    const bool fin = valid && finite2(cur);
    bad += valid && !fin ? 1 : 0;
    bool hit = false;
    if (fin) {
      const int2 x = seed_texel(g, cur);
      const float v = tex[(size_t)x.x * g.ny + x.y].x;
      hit = v < margin;
      clear_key = min(clear_key, order_key(__float_as_int(v)));
      outside += cur.x >= g.lo_x && cur.x <= hi_x && cur.y >= g.lo_y && cur.y <= hi_y ? 0 : 1;
    }
    points_hit += hit ? 1 : 0;
    bool seg_hit = hit;
    if (fin && t + 1 < L && finite2(nxt)) {
      const float dx = nxt.x - cur.x, dy = nxt.y - cur.y;
      const float s = torch_norm2(dx, dy);
      len += s;
      max_bits = max(max_bits, __float_as_int(s));
      for (int j = 1; j <= n_interp; ++j) {
        const float f = (float)j / parts;
        const float2 q = make_float2(cur.x + dx * f, cur.y + dy * f);
        if (!finite2(q)) continue;
        const int2 x = seed_texel(g, q);
        const float v = tex[(size_t)x.x * g.ny + x.y].x;
        clear_key = min(clear_key, order_key(__float_as_int(v)));
        if (v < margin) {
          ++interp_hit;
          seg_hit = true;
        }
      }
    }
    const unsigned long long hits = __ballot(seg_hit);
    if (first_hit < 0 && hits) first_hit = t0 + __ffsll((long long)hits) - 1;
    const bool on_goal = fin && torch_norm2(cur.x - goal.x, cur.y - goal.y) <= goal_tol;
    const unsigned long long off_goal = __ballot(valid && !on_goal);
    if (off_goal) arrival = t0 + 64 - __clzll((long long)off_goal);
  }
  points_hit = wave_sum(points_hit);
  interp_hit = wave_sum(interp_hit);
  bad = wave_sum(bad);
  outside = wave_sum(outside);
  clear_key = wave_min(clear_key);
  max_bits = wave_max(max_bits);
  len = wave_sum(len);
  if (lane != 0) return;
  const float2 last = path[L - 1];
  const float end_error = finite2(last) && finite2(goal) ? torch_norm2(last.x - goal.x, last.y - goal.y) : __int_as_float(FR_CANONICAL_NAN);
  int* w = words + robot;
  w[0 * (size_t)n] = points_hit;
  w[1 * (size_t)n] = interp_hit;
  w[2 * (size_t)n] = first_hit;
  w[3 * (size_t)n] = bad;
  w[4 * (size_t)n] = outside;
  w[5 * (size_t)n] = arrival;
  w[6 * (size_t)n] = order_key(clear_key);
  w[7 * (size_t)n] = __float_as_int(len);
  w[8 * (size_t)n] = max_bits;
  w[9 * (size_t)n] = __float_as_int(end_error);
  if (points_hit + interp_hit > 0) atomicAdd(header + MMD_FLEET_REPORT_ROBOTS_HIT, 1);
  if (arrival < L) atomicAdd(header + MMD_FLEET_REPORT_ROBOTS_ARRIVED, 1);
}

// ---- all pairs: a workgroup per (chunk of 64 columns, pair of robot tiles ti <= tj) ----
// Both tiles are staged in LDS as rows of 64 float2, lane = column: the loads from paths [n][L][2] are coalesced along t, and a row
// read by 64 consecutive lanes touches every bank once per half wave.  Rows past n and columns past L are NaN, which collides with
// nothing (so does every non-finite point: the margin is finite).  Wave w tests the rows w, w + 4, .. of tile i against every row of tile
// j (on the diagonal: the rows above it only).  A pair's count over the 64 columns is the population of one ballot, a uniform integer;
// the per-robot, per-column and total counts are added with integer atomics, the first conflict is the atomic minimum of (t, i, j)
// packed into 64 bits.  The robot whose count leaves zero is counted into robots_in_conflict by the adder that saw the zero.
__device__ __forceinline__ void add_conflicts(int* __restrict__ header, int* __restrict__ conflicts, int robot, int c) {
  if (atomicAdd(conflicts + robot, c) == 0) atomicAdd(header + MMD_FLEET_REPORT_ROBOTS_IN_CONFLICT, 1);
}

__global__ __launch_bounds__(256) void fleet_pair_report_kernel(const float2* __restrict__ paths, int n, int L, float rr_margin, int n_tiles,
                                                                 int* __restrict__ header, int* __restrict__ conflicts,
                                                                 int* __restrict__ columns) {
  __shared__ float2 tile_i[FR_TILE][64], tile_j[FR_TILE][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = blockIdx.x * 64, t = t0 + lane;
  int ti = 0, rest = blockIdx.y;                               // blockIdx.y counts the pairs (ti, tj >= ti) row by row
  for (; rest >= n_tiles - ti; ++ti) rest -= n_tiles - ti;
  const int tj = ti + rest;
  const bool diag = ti == tj;
  const float nan = __int_as_float(FR_CANONICAL_NAN);
  for (int r = wave; r < FR_TILE; r += 4) {
    const int i = ti * FR_TILE + r, j = tj * FR_TILE + r;
    tile_i[r][lane] = i < n && t < L ? paths[(size_t)i * L + t] : make_float2(nan, nan);
    if (!diag) tile_j[r][lane] = j < n && t < L ? paths[(size_t)j * L + t] : make_float2(nan, nan);
  }
  __syncthreads();
  const float2(*rows_j)[64] = diag ? tile_i : tile_j;
  int cj[FR_TILE];
#pragma unroll
  for (int s = 0; s < FR_TILE; ++s) cj[s] = 0;
  int col = 0, wave_total = 0;
  unsigned long long key = ~0ull;
  for (int r = wave; r < FR_TILE; r += 4) {
    const float2 a = tile_i[r][lane];
    const int i = ti * FR_TILE + r;
    int ci = 0;
#pragma unroll
    for (int s = 0; s < FR_TILE; ++s) {
      const bool hit = (!diag || s > r) && rr_hit(a, rows_j[s][lane], rr_margin);
      const unsigned long long mask = __ballot(hit);
      if (mask) {                                              // (uniform over the wave)
        const int c = __popcll(mask);
        ci += c;
        cj[s] += c;
        const unsigned long long k = ((unsigned long long)(t0 + __ffsll((long long)mask) - 1) << 24) | ((unsigned long long)i << 12) |
                                     (unsigned long long)(tj * FR_TILE + s);
        key = k < key ? k : key;
      }
      col += hit ? 1 : 0;
    }
    if (lane == 0 && ci) add_conflicts(header, conflicts, i, ci);
    wave_total += ci;
  }
  if (columns && col) atomicAdd(columns + t, col);             // (col > 0 only where t < L)
  if (lane != 0 || wave_total == 0) return;
#pragma unroll
  for (int s = 0; s < FR_TILE; ++s)
    if (cj[s]) add_conflicts(header, conflicts, tj * FR_TILE + s, cj[s]);
  atomicAdd((unsigned long long*)(header + MMD_FLEET_REPORT_CONFLICT_COUNT), (unsigned long long)wave_total);
  atomicMin((unsigned long long*)(header + MMD_FLEET_REPORT_FIRST_KEY), key);
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_fleet_run_report(const float* paths_dev, int n_robots, int length, const float* grid_dev, int nx, int ny, const float lo[2],
                         const float hi[2], const float* goals_dev, float margin, float rr_margin, int n_interp, float goal_tol,
                         int column_conflicts, int32_t* report_dev, void* stream) {
  MMD_REQUIRE(n_robots >= 0 && n_robots <= MMD_FLEET_REPORT_MAX_ROBOTS, "mmd_fleet_run_report: n_robots = %d (0 .. %d)", n_robots,
              MMD_FLEET_REPORT_MAX_ROBOTS);
  MMD_REQUIRE(length >= 2 && length <= MMD_FLEET_REPORT_MAX_LENGTH, "mmd_fleet_run_report: length = %d columns (2 .. %d)", length,
              MMD_FLEET_REPORT_MAX_LENGTH);
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "mmd_fleet_run_report: a grid of %d x %d cells (1 to %d per side)", nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(lo && hi, "mmd_fleet_run_report: NULL limits");
  const float dim_x = fabsf(hi[0] - lo[0]), dim_y = fabsf(hi[1] - lo[1]);
  MMD_REQUIRE(fabsf(lo[0]) <= FLT_MAX && fabsf(lo[1]) <= FLT_MAX && dim_x > 0.f && dim_x <= FLT_MAX && dim_y > 0.f && dim_y <= FLT_MAX,
              "mmd_fleet_run_report: limits (%g, %g) .. (%g, %g) (finite, a non-zero extent per axis)", (double)lo[0], (double)lo[1],
              (double)hi[0], (double)hi[1]);
  MMD_REQUIRE(fabsf(margin) <= FLT_MAX, "mmd_fleet_run_report: margin = %g (finite)", (double)margin);
  MMD_REQUIRE(fabsf(rr_margin) <= FLT_MAX, "mmd_fleet_run_report: rr_margin = %g (finite)", (double)rr_margin);
  MMD_REQUIRE(n_interp >= 0 && n_interp <= MMD_FLEET_REPORT_MAX_INTERP, "mmd_fleet_run_report: n_interp = %d (0 .. %d)", n_interp,
              MMD_FLEET_REPORT_MAX_INTERP);
  MMD_REQUIRE(goal_tol >= 0.f && goal_tol <= FLT_MAX, "mmd_fleet_run_report: goal_tol = %g (finite, >= 0)", (double)goal_tol);
  MMD_REQUIRE(column_conflicts == 0 || column_conflicts == 1, "mmd_fleet_run_report: column_conflicts = %d (0 or 1)", column_conflicts);
  if (n_robots == 0) return 0;
  MMD_REQUIRE(paths_dev && (uintptr_t)paths_dev % 8 == 0, "mmd_fleet_run_report: NULL or misaligned paths (8 bytes)");
  MMD_REQUIRE(grid_dev && (uintptr_t)grid_dev % 16 == 0, "mmd_fleet_run_report: NULL or misaligned grid (16 bytes)");
  MMD_REQUIRE(goals_dev && (uintptr_t)goals_dev % 8 == 0, "mmd_fleet_run_report: NULL or misaligned goals (8 bytes)");
  MMD_REQUIRE(report_dev && (uintptr_t)report_dev % 8 == 0, "mmd_fleet_run_report: NULL or misaligned report (8 bytes)");
  hipStream_t st = (hipStream_t)stream;
  const SeedGrid g = {nx, ny, lo[0], lo[1], dim_x, dim_y, dim_x / (float)nx, dim_y / (float)ny};
  const int n_cols = column_conflicts ? length : 0;
  int* header = report_dev;
  int* conflicts = header + MMD_FLEET_REPORT_HEADER;
  int* columns = conflicts + n_robots;
  int* words = columns + n_cols;
  // what the atomics add into: the header, every robot's conflicts and the columns are zero, the first conflict's key all ones
  MMD_HIP_CHECK(hipMemsetAsync(header, 0, sizeof(int) * (size_t)(MMD_FLEET_REPORT_HEADER + n_robots + n_cols), st));
  MMD_HIP_CHECK(hipMemsetAsync(header + MMD_FLEET_REPORT_FIRST_KEY, 0xff, 8, st));
  hipLaunchKernelGGL(fleet_robot_report_kernel, dim3((n_robots + 3) / 4), dim3(256), 0, st, (const float2*)paths_dev, n_robots, length,
                     (const float4*)grid_dev, g, hi[0], hi[1], (const float2*)goals_dev, margin, n_interp, goal_tol, header, words);
  const int n_tiles = (n_robots + FR_TILE - 1) / FR_TILE;
  hipLaunchKernelGGL(fleet_pair_report_kernel, dim3((length + 63) / 64, n_tiles * (n_tiles + 1) / 2), dim3(256), 0, st,
                     (const float2*)paths_dev, n_robots, length, rr_margin, n_tiles, header, conflicts, column_conflicts ? columns : nullptr);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
