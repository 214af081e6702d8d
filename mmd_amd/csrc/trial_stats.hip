// The statistics of a multi-agent solution (scripts/inference/inference_multi_agent.py:285-342) in one launch sequence and one output
// buffer, so that a trial reads them back with one device -> host copy:
//   * agent pairs in collision: the loop of inference_multi_agent.py:288-294 over the globally padded paths;
//   * the data-adherence score of every (agent, skeleton step) tile by the rule of the tile's environment
//     (compute_traj_data_adherence of deps/torch_robotics/torch_robotics/environments/env_empty_2d.py:132-146, env_highways_2d.py:255-273,
//     env_conveyor_2d.py:161-185, env_drop_region_2d.py:183-196);
//   * path length and mean acceleration per agent (deps/torch_robotics/torch_robotics/trajectory/metrics.py:13-16, :52-65).
// A tile is 64 rows = one wave64, lane = support point.  Every decision (collision, waypoint visit, inside-disc, within-fraction) is the
// reference's fp32 arithmetic operation for operation (torch.norm over two components = sqrt(fma(dy, dy, dx * dx)), collision_dev.h).
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"
#include "collision_dev.h"        // torch_norm2 / rr_hit; sets fp contract(off): every fp32 operation below is the one written out
#include "common.h"
#include "wave_dev.h"             // wave_sum (fixed order: a float sum does not depend on scheduling) / block_sum

namespace mmd {

// first set bit of `mask` strictly above bit `prev` (prev = -1: any bit), or 64
__device__ __forceinline__ int first_above(unsigned long long mask, int prev) {
  const unsigned long long m = prev >= 63 ? 0ull : mask & (~0ull << (prev + 1));
  return m ? __ffsll((long long)m) - 1 : 64;
}

// env_empty_2d.py:132-146: the fraction of points closer than 0.1 (mmd_params.py:57) to the first-to-last-point line.
// torch.cross((g, 0), (p, 0)).z = fma(g_x, p_y, -(g_y * p_x)); torch.norm of (0, 0, z) = |z|; length = torch.norm(g).
// length == 0: |z| / length is NaN for every point, no point counts.
__device__ __forceinline__ float adherence_line(float2 p) {
  const float2 first = make_float2(__shfl(p.x, 0), __shfl(p.y, 0)), last = make_float2(__shfl(p.x, 63), __shfl(p.y, 63));
  const float gx = last.x - first.x, gy = last.y - first.y;
  const float length = torch_norm2(gx, gy);
  const float px = p.x - first.x, py = p.y - first.y;
  const float z = __builtin_fmaf(gx, py, -(gy * px));
  const float deviation = fabsf(z) / length;
  return (float)__popcll(__ballot(deviation < 0.1f)) / 64.f;
}

// env_highways_2d.py:255-273: position VECTORS normalised, the 2-D cross product of consecutive ones (each product and the difference
// rounded on their own), 1 iff the sum of the 63 products is > 0.  A point at the origin makes the sum NaN -> 0.
__device__ __forceinline__ float adherence_highways(float2 p, int lane) {
  const float norm = torch_norm2(p.x, p.y);
  const float vx = p.x / norm, vy = p.y / norm;
  const float nx = __shfl_down(vx, 1), ny = __shfl_down(vy, 1);
  const float a = vx * ny, b = vy * nx;
  const float cross = lane < 63 ? a - b : 0.f;
  return wave_sum(cross) > 0.f ? 1.f : 0.f;
}

// env_conveyor_2d.py:161-185: per corridor three waypoints visited greedily in order (radius 0.2), at most one per time step, so each visit
// is strictly later than the one before; 1 iff either corridor's third waypoint gets visited.  (After the third visit the reference's
// argmin goes round again and overwrites visit times with later ones: no entry returns to -1.)
__device__ __forceinline__ bool corridor_passed(float2 p, float x0, float x2, float y) {
  const unsigned long long m0 = __ballot(torch_norm2(p.x - x0, p.y - y) < 0.2f);
  const unsigned long long m1 = __ballot(torch_norm2(p.x - 0.0f, p.y - y) < 0.2f);
  const unsigned long long m2 = __ballot(torch_norm2(p.x - x2, p.y - y) < 0.2f);
  const int t0 = first_above(m0, -1);
  const int t1 = t0 < 64 ? first_above(m1, t0) : 64;
  const int t2 = t1 < 64 ? first_above(m2, t1) : 64;
  return t2 < 64;
}

__device__ __forceinline__ float adherence_conveyor(float2 p) {
  const bool top = corridor_passed(p, 0.6f, -0.6f, 0.2f);         // entered from the right, left to the left
  const bool bottom = corridor_passed(p, -0.6f, 0.6f, -0.2f);     // entered from the left, left to the right
  return top || bottom ? 1.f : 0.f;
}

// env_drop_region_2d.py:183-196: 1 iff for one of the 16 centres (:80-97) 16 consecutive points lie within 0.15 -- among rows 0 .. 62:
// range(16, 64) with mask[i - 16 : i] never reads row 63.
__constant__ float2 DROP_REGION_CENTERS[16] = {
    {0.4f, 0.75f},  {0.4f, 0.05f},  {0.4f, -0.05f},  {0.4f, -0.75f},  {-0.4f, 0.75f},  {-0.4f, 0.05f},  {-0.4f, -0.05f},  {-0.4f, -0.75f},
    {0.75f, 0.4f},  {0.05f, 0.4f},  {-0.05f, 0.4f},  {-0.75f, 0.4f},  {0.75f, -0.4f},  {0.05f, -0.4f},  {-0.05f, -0.4f},  {-0.75f, -0.4f}};

__device__ __forceinline__ float adherence_drop_region(float2 p) {
  bool found = false;
#pragma unroll 4
  for (int c = 0; c < 16; ++c) {
    const float2 q = DROP_REGION_CENTERS[c];
    unsigned long long m = __ballot(torch_norm2(p.x - q.x, p.y - q.y) < 0.15f) & ~(1ull << 63);
    m &= m >> 1;           // bit s: rows s, s + 1 inside
    m &= m >> 2;           // rows s .. s + 3
    m &= m >> 4;           // rows s .. s + 7
    m &= m >> 8;           // rows s .. s + 15
    found |= m != 0ull;
  }
  return found ? 1.f : 0.f;
}

// one wave per tile reference, lane = support point
__global__ __launch_bounds__(256) void tile_adherence_kernel(const float4* __restrict__ paths, int Tg, const mmd_tile_ref* __restrict__ tiles,
                                                              int n_tiles, float* __restrict__ adherence) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;                                  // (whole waves leave together)
  const mmd_tile_ref ref = tiles[tile];
  const float4 s = paths[(size_t)ref.agent * Tg + ref.t0 + lane];
  const float2 p = make_float2(s.x - ref.offset[0], s.y - ref.offset[1]);          // inference_multi_agent.py:310-313
  float score;
  switch (ref.rule) {                                            // (uniform over the wave)
    case MMD_ADHERENCE_LINE: score = adherence_line(p); break;
    case MMD_ADHERENCE_HIGHWAYS: score = adherence_highways(p, lane); break;
    case MMD_ADHERENCE_CONVEYOR: score = adherence_conveyor(p); break;
    default: score = adherence_drop_region(p); break;           // MMD_ADHERENCE_DROP_REGION (rules are checked on the host)
  }
  if (lane == 0) adherence[tile] = score;
}

// one wave per agent over its Tg rows in chunks of 64: sum_t ||p_{t+1} - p_t|| and mean_t ||v_{t+1} - v_t|| (Tg - 1 terms each)
__global__ __launch_bounds__(256) void agent_stats_kernel(const float4* __restrict__ paths, int n_agents, int Tg,
                                                           float* __restrict__ path_length, float* __restrict__ mean_accel) {
  const int lane = threadIdx.x & 63;
  const int agent = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (agent >= n_agents) return;
  const float4* path = paths + (size_t)agent * Tg;
  float len = 0.f, acc = 0.f;
  for (int t0 = 0; t0 < Tg - 1; t0 += 64) {
    const int t = t0 + lane;
    const float4 cur = path[t < Tg ? t : Tg - 1];
    float4 nxt = make_float4(__shfl_down(cur.x, 1), __shfl_down(cur.y, 1), __shfl_down(cur.z, 1), __shfl_down(cur.w, 1));
    if (lane == 63 && t + 1 < Tg) nxt = path[t + 1];            // the first row of the next chunk
    if (t + 1 < Tg) {
      len += torch_norm2(nxt.x - cur.x, nxt.y - cur.y);
      acc += torch_norm2(nxt.z - cur.z, nxt.w - cur.w);
    }
  }
  len = wave_sum(len);
  acc = wave_sum(acc);
  if (lane == 0) {
    path_length[agent] = len;
    mean_accel[agent] = acc / (float)(Tg - 1);                   // Tg == 1: 0 / 0, the mean of an empty tensor
  }
}

// one workgroup per time step: the pairs (i < j) of row t in collision, added to *count (an integer atomic: order-independent)
__global__ __launch_bounds__(256) void pair_collisions_kernel(const float4* __restrict__ paths, int n, int Tg, float dist,
                                                               int* __restrict__ count) {
  __shared__ int lds4[4];
  const int t = blockIdx.x;
  int c = 0;
  for (int cell = threadIdx.x; cell < n * n; cell += 256) {
    const int i = cell / n, j = cell % n;
    if (i < j) {
      const float4 a = paths[(size_t)i * Tg + t], b = paths[(size_t)j * Tg + t];
      c += rr_hit(make_float2(a.x, a.y), make_float2(b.x, b.y), dist) ? 1 : 0;
    }
  }
  c = block_sum<true>(c, lds4);                               // (the last use of lds4: no barrier behind the read)
  if (threadIdx.x == 0 && c) atomicAdd(count, c);
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_solution_stats(const float* paths_dev, int n_agents, int horizon_global, float collision_dist, const mmd_tile_ref* tiles,
                       int n_tiles, const mmd_tile_ref* tiles_dev, float* stats_dev, void* stream) {
  MMD_REQUIRE(n_agents >= 1 && n_agents <= 4096, "mmd_solution_stats: n_agents = %d (1 .. 4096)", n_agents);
  MMD_REQUIRE(paths_dev && stats_dev, "mmd_solution_stats: NULL argument");
  MMD_REQUIRE(horizon_global >= 1 && horizon_global <= 65535, "mmd_solution_stats: horizon_global = %d (1 .. 65535)", horizon_global);
  MMD_REQUIRE(n_tiles >= 0 && (n_tiles == 0 || (tiles && tiles_dev)), "mmd_solution_stats: n_tiles = %d without a tile table", n_tiles);
  for (int k = 0; k < n_tiles; ++k) {
    const mmd_tile_ref& r = tiles[k];
    MMD_REQUIRE(r.rule >= MMD_ADHERENCE_LINE && r.rule <= MMD_ADHERENCE_DROP_REGION, "mmd_solution_stats: tile %d has unknown adherence rule %d",
                k, r.rule);
    MMD_REQUIRE(r.agent >= 0 && r.agent < n_agents, "mmd_solution_stats: tile %d names agent %d of %d", k, r.agent, n_agents);
    MMD_REQUIRE(r.t0 >= 0 && r.t0 <= horizon_global - MMD_HORIZON,
                "mmd_solution_stats: the %d rows of tile %d from row %d do not fit in horizon_global = %d", MMD_HORIZON, k, r.t0, horizon_global);
  }
  hipStream_t st = (hipStream_t)stream;
  const float4* paths = (const float4*)paths_dev;
  int* count = (int*)stats_dev;
  float* path_length = stats_dev + 1;
  float* mean_accel = path_length + n_agents;
  float* adherence = mean_accel + n_agents;
  MMD_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int), st));
  hipLaunchKernelGGL(pair_collisions_kernel, dim3(horizon_global), dim3(256), 0, st, paths, n_agents, horizon_global, collision_dist, count);
  hipLaunchKernelGGL(agent_stats_kernel, dim3((n_agents + 3) / 4), dim3(256), 0, st, paths, n_agents, horizon_global, path_length, mean_accel);
  if (n_tiles > 0)
    hipLaunchKernelGGL(tile_adherence_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, st, paths, horizon_global, tiles_dev, n_tiles, adherence);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
