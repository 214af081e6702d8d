// World routes: the seed trajectory of a route.  From a converged distance field and a start, the 64 support cells of every tile visit
// of the cell path (include/mmd_amd.h: mmd_grid_descend_samples), and from those the smoothed chain of support points with velocities, in
// trajs_final's format (mmd_route_seeds).  The definitions are the numpy functions descend_samples and seed_trajectory of
// mmd_amd/world_routes.py: the same integers and the same float32 bits.  Plain loads and vector stores; no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/mmd_amd.h"
#include "common.h"
#include "grid_route_dev.h"
#include "seed_dev.h"
#include "walk_args.h"
#include "wave_dev.h"
// every float operation below is one rounding: no fused multiply-add
#pragma clang fp contract(off)

namespace mmd {

constexpr int RS_POINTS = MMD_ROUTE_SEED_POINTS;            // support points of a tile visit
constexpr int RS_MAX_TILES = MMD_ROUTE_SEED_MAX_TILES;
constexpr int RS_CHAIN = RS_POINTS * RS_MAX_TILES;          // the longest chain: 1024 points
constexpr int RS_THREADS = 256;
constexpr int RS_PER_THREAD = RS_CHAIN / RS_THREADS;        // a thread owns the points t, t + 256, t + 512, t + 768
static_assert(RS_POINTS == 64 && RS_CHAIN == RS_THREADS * RS_PER_THREAD, "a wave's 64 points are one tile visit");

// ---- the samples of a descent: one lane per query (walk_entry, descend_step: grid_route_dev.h; emit_samples: seed_dev.h) ----
// The lane walks the field twice, with no buffer proportional to the path: the first walk is mmd_grid_descend's and counts the cells of
// every visit; the second, only for status 0, repeats it and emits each visit's 64 samples as it passes them.  Each walk's loop runs at
// most dist[start] times, whatever the field holds (d falls by one per step), and emit_samples at most 64 times per visit in all (j only
// grows).  Every row of visit_cells and cells of the query is written: zero behind n_tiles and for a status other than 0.
__global__ __launch_bounds__(WALK_THREADS) void grid_descend_samples_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                            const int2* __restrict__ starts, const int* __restrict__ field,
                                                                            int n_queries, int tile, int o_i, int o_j, int max_tiles,
                                                                            int2* __restrict__ tiles, int4* __restrict__ summary,
                                                                            int* visit_cells, int2* __restrict__ cells) {
  const int q = blockIdx.x * WALK_THREADS + threadIdx.x;
  if (q >= n_queries) return;
  const WalkEntry e = walk_entry(dist_all, nx, ny, n_fields, starts, field, q);
  int* vc = visit_cells + (size_t)q * max_tiles;
  int2* rows = cells + (size_t)q * max_tiles * RS_POINTS;
  int4 sum = make_int4(-1, 0, e.no_walk, 0);
  int n_visits = 0;
  if (e.d0 != GRID_UNREACHED) {
    int2* out = tiles + (size_t)q * max_tiles;
    int ix = e.s.x, iy = e.s.y;
    long long ta = floor_div((long long)ix - o_i, tile), tb = floor_div((long long)iy - o_j, tile);
    int n_tiles = 1, steps = 0, status = WALK_OK, m = 1;
    out[0] = make_int2((int)ta, (int)tb);
    for (int d = e.d0; d > 0; --d) {
      const int r = descend_step(e.dist, nx, ny, tile, o_i, o_j, d, ix, iy, ta, tb);
      if (r < 0) { status = WALK_STUCK; break; }
      ++steps;
      if (r) { ++m; continue; }
      if (n_tiles <= max_tiles) vc[n_tiles - 1] = m;
      if (n_tiles < max_tiles) out[n_tiles] = make_int2((int)ta, (int)tb);
      ++n_tiles;
      m = 1;
    }
    if (n_tiles <= max_tiles) vc[n_tiles - 1] = m;
    if (status == WALK_OK && n_tiles > max_tiles) status = WALK_TILES;
    sum = make_int4(steps, n_tiles, status, 0);
    if (status == WALK_OK) n_visits = n_tiles;
  }
  summary[q] = sum;
  for (int k = n_visits; k < max_tiles; ++k) {
    vc[k] = 0;
    for (int j = 0; j < RS_POINTS; ++j) rows[(size_t)k * RS_POINTS + j] = make_int2(0, 0);
  }
  if (n_visits == 0) return;

  int ix = e.s.x, iy = e.s.y;
  long long ta = floor_div((long long)ix - o_i, tile), tb = floor_div((long long)iy - o_j, tile);
  int k = 0, m = vc[0], t = 0, j = 0;
  emit_samples(rows, j, m, t, ix, iy);
  for (int d = e.d0; d > 0; --d) {
    const int r = descend_step(e.dist, nx, ny, tile, o_i, o_j, d, ix, iy, ta, tb);
    if (r < 0) break;                                      // (the first walk passed here)
    if (r) {
      ++t;
    } else {
      if (++k >= n_visits) break;                          // (the first walk counted n_visits)
      m = vc[k];
      t = j = 0;
    }
    emit_samples(rows + (size_t)k * RS_POINTS, j, m, t, ix, iy);
  }
}

// ---- the seed: one workgroup per route ----
// Workgroup = route, 256 threads x 4 points (point i = t + 256 r: a wave's 64 points are one tile visit, so a wave behind the route's K
// visits only meets the barriers).  The chain lives in LDS as two float2 buffers; iteration `it` reads buffer it & 1 and writes the other,
// every interior point from its two neighbours of the iteration before (Jacobi: no order within an iteration matters, so the result does
// not depend on the launch shape).  Per iteration and point: two 8-byte LDS reads, the candidate, one 4-byte texel gather (the four of a
// thread are independent and in flight together), the two tests, one 8-byte LDS write; one barrier per iteration.  The loop runs
// smooth_iters times.  The point's own value stays in a register.
__global__ __launch_bounds__(RS_THREADS) void route_seeds_kernel(const float4* __restrict__ tex, SeedGrid g, float clearance,
                                                                 const int2* __restrict__ cells, const int2* __restrict__ tiles,
                                                                 const int4* __restrict__ summary, int tile, int o_i, int o_j, int max_tiles,
                                                                 const float2* __restrict__ start_points, const float2* __restrict__ goal_points,
                                                                 int smooth_iters, float two_dt, float4* __restrict__ seeds,
                                                                 int* __restrict__ clear_min) {
  __shared__ float2 chain[2][RS_CHAIN];
  __shared__ int lds4[4];
  const int route = blockIdx.x, t = threadIdx.x;
  const int4 sum = summary[route];
  const int n_visits = sum.z == 0 ? min(max(sum.y, 0), max_tiles) : 0;
  const int n = n_visits * RS_POINTS, n_rows = max_tiles * RS_POINTS;
  float4* out = seeds + (size_t)route * n_rows;
  if (n == 0) {                                            // one decision per workgroup: no chain, no texture read
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; ++r)
      if (t + RS_THREADS * r < n_rows) out[t + RS_THREADS * r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t == 0) clear_min[route] = 0;
    return;
  }

  float2 mine[RS_PER_THREAD];
  long long tile_i[RS_PER_THREAD], tile_j[RS_PER_THREAD];  // the first cell of the point's lattice tile
#pragma unroll
  for (int r = 0; r < RS_PER_THREAD; ++r) {
    const int i = t + RS_THREADS * r;
    mine[r] = make_float2(0.f, 0.f);
    tile_i[r] = tile_j[r] = 0;
    if (i >= n) continue;
    const int2 c = cells[(size_t)route * n_rows + i];
    const int2 ab = tiles[(size_t)route * max_tiles + i / RS_POINTS];
    tile_i[r] = (long long)o_i + (long long)ab.x * tile;
    tile_j[r] = (long long)o_j + (long long)ab.y * tile;
    mine[r] = make_float2(g.lo_x + ((float)c.x + 0.5f) * g.pitch_x, g.lo_y + ((float)c.y + 0.5f) * g.pitch_y);
    if (i == 0) mine[r] = start_points[route];
    if (i == n - 1) mine[r] = goal_points[route];
    chain[0][i] = mine[r];
  }
  __syncthreads();

  for (int it = 0; it < smooth_iters; ++it) {
    const float2* src = chain[it & 1];
    float2* dst = chain[(it & 1) ^ 1];
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; ++r) {
      const int i = t + RS_THREADS * r;
      if (i >= n) continue;
      if (i > 0 && i < n - 1) {
        const float2 a = src[i - 1], b = src[i + 1];
        const float2 c = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y + b.y));
        const int2 x = seed_texel(g, c);
        const bool clear = tex[(size_t)x.x * g.ny + x.y].x > clearance;
        const bool in_tile = x.x >= tile_i[r] && x.x < tile_i[r] + tile && x.y >= tile_j[r] && x.y < tile_j[r] + tile;
        if (clear && in_tile) mine[r] = c;
      }
      dst[i] = mine[r];
    }
    __syncthreads();
  }

  const float2* fin = chain[smooth_iters & 1];
  int key = INT_MAX;
#pragma unroll
  for (int r = 0; r < RS_PER_THREAD; ++r) {
    const int i = t + RS_THREADS * r;
    if (i >= n_rows) continue;
    float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
      float2 v = make_float2(0.f, 0.f);
      if (i > 0 && i < n - 1) {
        const float2 a = fin[i - 1], b = fin[i + 1];
        v = make_float2((b.x - a.x) / two_dt, (b.y - a.y) / two_dt);
      }
      row = make_float4(mine[r].x, mine[r].y, v.x, v.y);
      const int2 x = seed_texel(g, mine[r]);
      key = min(key, order_key(__float_as_int(tex[(size_t)x.x * g.ny + x.y].x)));
    }
    out[i] = row;
  }
  key = wave_min(key);
  if ((t & 63) == 0) lds4[t >> 6] = key;
  __syncthreads();
  if (t == 0) clear_min[route] = order_key(min(min(lds4[0], lds4[1]), min(lds4[2], lds4[3])));
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_grid_descend_samples(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev, const int32_t* field_dev,
                             int n_queries, int tile, const int32_t lattice_origin[2], int max_tiles, int32_t* tiles_dev, int32_t* summary_dev,
                             int32_t* visit_cells_dev, int32_t* cells_dev, void* stream) {
  if (const int refused = descend_args("mmd_grid_descend_samples", dist_dev, nx, ny, n_fields, starts_dev, field_dev, n_queries, tile,
                                       lattice_origin, max_tiles, RS_MAX_TILES, tiles_dev, summary_dev))
    return refused;
  if (n_queries == 0) return 0;
  MMD_REQUIRE(visit_cells_dev, "mmd_grid_descend_samples: NULL visit_cells");
  MMD_REQUIRE(cells_dev, "mmd_grid_descend_samples: NULL cells");
  hipLaunchKernelGGL(grid_descend_samples_kernel, dim3((n_queries + WALK_THREADS - 1) / WALK_THREADS), dim3(WALK_THREADS), 0, (hipStream_t)stream,
                     (const int*)dist_dev, nx, ny, n_fields, (const int2*)starts_dev, (const int*)field_dev, n_queries, tile, lattice_origin[0],
                     lattice_origin[1], max_tiles, (int2*)tiles_dev, (int4*)summary_dev, (int*)visit_cells_dev, (int2*)cells_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_route_seeds(const float* grid_dev, int nx, int ny, const float lo[2], const float hi[2], float clearance, const int32_t* cells_dev,
                    const int32_t* tiles_dev, const int32_t* summary_dev, int n_routes, int tile, const int32_t lattice_origin[2], int max_tiles,
                    const float* start_points_dev, const float* goal_points_dev, int smooth_iters, float two_dt, float* seeds_dev,
                    float* clear_min_dev, void* stream) {
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "mmd_route_seeds: a grid of %d x %d cells (1 to %d per side)", nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(lo && hi, "mmd_route_seeds: NULL limits");
  const float dim_x = fabsf(hi[0] - lo[0]), dim_y = fabsf(hi[1] - lo[1]);
  MMD_REQUIRE(fabsf(lo[0]) <= FLT_MAX && fabsf(lo[1]) <= FLT_MAX && dim_x > 0.f && dim_x <= FLT_MAX && dim_y > 0.f && dim_y <= FLT_MAX,
              "mmd_route_seeds: limits (%g, %g) .. (%g, %g) (finite, a non-zero extent per axis)", (double)lo[0], (double)lo[1], (double)hi[0],
              (double)hi[1]);
  MMD_REQUIRE(fabsf(clearance) <= FLT_MAX, "mmd_route_seeds: clearance = %g (finite)", (double)clearance);
  MMD_REQUIRE(two_dt > 0.f && two_dt <= FLT_MAX, "mmd_route_seeds: two_dt = %g (finite, > 0)", (double)two_dt);
  MMD_REQUIRE(smooth_iters >= 0, "mmd_route_seeds: smooth_iters = %d (>= 0)", smooth_iters);
  MMD_REQUIRE(n_routes >= 0, "mmd_route_seeds: n_routes = %d (>= 0)", n_routes);
  MMD_REQUIRE(tile >= 1, "mmd_route_seeds: tile = %d cells (>= 1)", tile);
  MMD_REQUIRE(max_tiles >= 1 && max_tiles <= RS_MAX_TILES, "mmd_route_seeds: max_tiles = %d (1 to %d: the chain lives in LDS)", max_tiles,
              RS_MAX_TILES);
  MMD_REQUIRE(lattice_origin, "mmd_route_seeds: NULL lattice_origin");
  MMD_REQUIRE(origin_ok(lattice_origin), "mmd_route_seeds: lattice_origin = (%d, %d) (each within +-2^30)", lattice_origin[0],
              lattice_origin[1]);
  if (n_routes == 0) return 0;
  MMD_REQUIRE(grid_dev, "mmd_route_seeds: NULL grid");
  MMD_REQUIRE(cells_dev, "mmd_route_seeds: NULL cells");
  MMD_REQUIRE(tiles_dev, "mmd_route_seeds: NULL tiles");
  MMD_REQUIRE(summary_dev, "mmd_route_seeds: NULL summary");
  MMD_REQUIRE(start_points_dev && goal_points_dev, "mmd_route_seeds: NULL start or goal points");
  MMD_REQUIRE(seeds_dev, "mmd_route_seeds: NULL seeds");
  MMD_REQUIRE(clear_min_dev, "mmd_route_seeds: NULL clear_min");
  const SeedGrid g = {nx, ny, lo[0], lo[1], dim_x, dim_y, dim_x / (float)nx, dim_y / (float)ny};
  hipLaunchKernelGGL(route_seeds_kernel, dim3(n_routes), dim3(RS_THREADS), 0, (hipStream_t)stream, (const float4*)grid_dev, g, clearance,
                     (const int2*)cells_dev, (const int2*)tiles_dev, (const int4*)summary_dev, tile, lattice_origin[0], lattice_origin[1],
                     max_tiles, (const float2*)start_points_dev, (const float2*)goal_points_dev, smooth_iters, two_dt, (float4*)seeds_dev,
                     (int*)clear_min_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
