// World routes: the geodesic distance field of an SDF texture's routable cells, one field per goal, and the descent from a start cell that
// yields the sequence of lattice tiles a route crosses (include/mmd_amd.h: mmd_grid_distance_field, mmd_grid_descend).  The definitions
// are the numpy functions of mmd_amd/world_routes.py (routable_cells, grid_distance_field, descend); every value here is an exact integer.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/mmd_amd.h"
#include "common.h"
#include "grid_route_dev.h"
#include "walk_args.h"

namespace mmd {

constexpr int GD_BLOCK = MMD_GRID_DIST_BLOCK;        // a workgroup's block of cells, per side
constexpr int GD_LDS = GD_BLOCK + 2;                 // with a one-cell halo
constexpr int GD_THREADS = 256;
constexpr int GD_ROWS = GD_BLOCK * GD_BLOCK / GD_THREADS;      // rows of one column that a thread owns: 16 consecutive ones
constexpr int GD_MAX_ITERS = GD_BLOCK * GD_BLOCK + 1;
constexpr int GD_NEVER = -1;                         // a block flag: "has not lowered a value since the restart"
static_assert(GD_THREADS == 4 * GD_BLOCK && GD_ROWS * 4 == GD_BLOCK, "a thread owns one column of a quarter of the block's rows");

#define GD_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define GD_RELAXED_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// routable[ix][iy] = tex[ix][iy][0] > clearance (a strict fp32 compare: a NaN texel is not routable) inside the region, upper bounds exclusive
struct GridRegion { int i_lo, j_lo, i_hi, j_hi; };
__device__ __forceinline__ bool gd_routable(const float4* __restrict__ tex, int ny, float clearance, GridRegion rg, int ix, int iy) {
  return ix >= rg.i_lo && ix < rg.i_hi && iy >= rg.j_lo && iy < rg.j_hi && tex[(size_t)ix * ny + iy].x > clearance;
}

// The workspace: int32 sweep[n_fields], the number of sweeps field f has run since its restart, then int32 flag[n_fields][nbx * nby], the
// number of the last sweep (1-based) in which the block lowered a value; the goal's block holds 0 after a restart, every other GD_NEVER.
__device__ __forceinline__ int* gd_flags(int* work, int n_fields, int f, int n_blocks) { return work + n_fields + (size_t)f * n_blocks; }

// Restart: one thread per cell of one field (blockIdx.y).  The goal is device data and may be anything: outside the grid, or not routable,
// gives the field that is UNREACHED everywhere with no block flagged.
__global__ __launch_bounds__(GD_THREADS) void grid_distance_init_kernel(const float4* __restrict__ tex, int nx, int ny, float clearance,
                                                                        GridRegion rg, const int2* __restrict__ goals, int n_fields,
                                                                        int nby, int n_blocks, int* __restrict__ dist, int* __restrict__ work) {
  const int cell = blockIdx.x * GD_THREADS + threadIdx.x;
  if (cell >= nx * ny) return;
  const int f = blockIdx.y;
  const int2 g = goals[f];
  const bool seeded = g.x >= 0 && g.x < nx && g.y >= 0 && g.y < ny && gd_routable(tex, ny, clearance, rg, g.x, g.y);
  dist[(size_t)f * nx * ny + cell] = (seeded && cell == g.x * ny + g.y) ? 0 : GRID_UNREACHED;
  if (cell < n_blocks)          // (a block holds at least one cell: n_blocks <= nx * ny)
    gd_flags(work, n_fields, f, n_blocks)[cell] = (seeded && cell == (g.x / GD_BLOCK) * nby + g.y / GD_BLOCK) ? 0 : GD_NEVER;
  if (cell == 0) work[f] = 0;
}

// One sweep of the block-tiled Bellman-Ford.  Workgroup (blockIdx.y, blockIdx.x, blockIdx.z) = (block row bi, block column bj, field).
//
// Why the fixed point is the exact field, whatever the order in which the workgroups of a sweep run and wherever they are placed:
//   (1) Every value ever stored is UNREACHED or the length of a real path over routable cells from the goal: the restart stores 0 at the
//       goal, and a relaxation stores a neighbour's value + 1 on a routable cell.  So no value is ever below the true distance.
//   (2) Values only fall: a cell is stored only with a value below the one it held.
//   (3) A halo cell read during a sweep is its owner's value from before or from within this sweep (a relaxed agent-scope load of a word
//       that the owner stores whole with a relaxed agent-scope store: never torn, and by the kernel boundary never older than the end of
//       the previous sweep).  Either is covered by (1).
//   (4) A block that lowers a value in sweep s stores s in its flag.  In sweep s + 1 the flag reads s, or s + 1 if the owner has already
//       lowered a value again: a block runs iff its own or a neighbour's flag is >= s, so every reader of the lowered value runs in sweep
//       s + 1, behind the kernel boundary, where the value is visible.  Nothing in a sweep waits on another workgroup.
//   (5) When a sweep ends with no flag set to its number, every block's last run saw the halo as it now stands (a later change of it
//       would have set a flag and run the block again, by 4) and ended with no cell of the block improvable: d <= min(neighbours) + 1
//       holds on every routable cell of the grid.  With (1), by induction over the true distance k: a cell at true distance k has a
//       neighbour at k - 1 that holds exactly k - 1, so it holds at most k, and by (1) at least k.
// A workgroup-scope fence would add nothing: another CU cannot observe it, and (3) needs no ordering between the words of a block.
//
// Thread t owns column t % 64 of rows (t / 64) * 16 .. + 16: a wave loads and stores 64 consecutive cells of a row.  The block sits in LDS
// with its halo; an iteration relaxes the thread's 16 cells top to bottom and bottom to top, in place (relaxed workgroup-scope accesses:
// a neighbour's older or newer value, both covered by 1), so a fall travels a thread's strip in one iteration; the block votes after
// each.  At most 64 * 64 + 1 iterations: with the halo fixed, iteration k settles every cell whose shortest path inside the block from a
// settled source has k cells, a path has at most 64 * 64, and one more iteration sees no change.  If the bound ever cut a block short it
// would have lowered a value in its last iteration, flagged itself, and run again in the next sweep.
__global__ __launch_bounds__(GD_THREADS) void grid_distance_sweep_kernel(const float4* __restrict__ tex, int nx, int ny, float clearance,
                                                                         GridRegion rg, int n_fields, int sweep_in_call,
                                                                         int* __restrict__ dist_all, int* __restrict__ work) {
  __shared__ int lds[GD_LDS * GD_LDS];
  __shared__ int active;
  const int bi = blockIdx.y, bj = blockIdx.x, f = blockIdx.z;
  const int nbx = gridDim.y, nby = gridDim.x;
  int* flags = gd_flags(work, n_fields, f, nbx * nby);
  const int sweep = work[f] + sweep_in_call + 1;          // this sweep's number (work[f] moves only in the call's last kernel)
  if (threadIdx.x == 0) {
    int newest = __hip_atomic_load(&flags[bi * nby + bj], GD_RELAXED_AGENT);
    if (bi > 0) newest = max(newest, __hip_atomic_load(&flags[(bi - 1) * nby + bj], GD_RELAXED_AGENT));
    if (bi + 1 < nbx) newest = max(newest, __hip_atomic_load(&flags[(bi + 1) * nby + bj], GD_RELAXED_AGENT));
    if (bj > 0) newest = max(newest, __hip_atomic_load(&flags[bi * nby + bj - 1], GD_RELAXED_AGENT));
    if (bj + 1 < nby) newest = max(newest, __hip_atomic_load(&flags[bi * nby + bj + 1], GD_RELAXED_AGENT));
    active = newest >= sweep - 1;
  }
  __syncthreads();
  if (!active) return;                                     // one decision per workgroup: every thread leaves, or none

  int* dist = dist_all + (size_t)f * nx * ny;
  const int col = threadIdx.x % GD_BLOCK, row0 = (threadIdx.x / GD_BLOCK) * GD_ROWS;
  const int i0 = bi * GD_BLOCK, j0 = bj * GD_BLOCK;
  const int iy = j0 + col;
  // own cells: plain loads (only this block ever stores them, in earlier launches); a cell outside the grid or not routable holds
  // UNREACHED and is never relaxed
  int loaded[GD_ROWS];
  unsigned routable = 0;
#pragma unroll
  for (int k = 0; k < GD_ROWS; ++k) {
    const int ix = i0 + row0 + k;
    const bool inside = ix < nx && iy < ny;
    loaded[k] = inside ? dist[(size_t)ix * ny + iy] : GRID_UNREACHED;
    if (inside && gd_routable(tex, ny, clearance, rg, ix, iy)) routable |= 1u << k;
    lds[(row0 + k + 1) * GD_LDS + col + 1] = loaded[k];
  }
  // the halo: 4 x 64 cells of the neighbours' outer rings, one per thread (the corners are never read)
  {
    const int side = threadIdx.x / GD_BLOCK, k = threadIdx.x % GD_BLOCK;
    const int hr = side == 0 ? -1 : side == 1 ? GD_BLOCK : k;            // row, column in block coordinates
    const int hc = side == 2 ? -1 : side == 3 ? GD_BLOCK : k;
    const int ix = i0 + hr, jy = j0 + hc;
    int v = GRID_UNREACHED;
    if (ix >= 0 && ix < nx && jy >= 0 && jy < ny) v = __hip_atomic_load(&dist[(size_t)ix * ny + jy], GD_RELAXED_AGENT);
    lds[(hr + 1) * GD_LDS + hc + 1] = v;
  }
  __syncthreads();

  for (int it = 0; it < GD_MAX_ITERS; ++it) {
    int fell = 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int kk = 0; kk < GD_ROWS; ++kk) {
        const int k = pass == 0 ? kk : GD_ROWS - 1 - kk;
        if (!(routable >> k & 1u)) continue;
        int* c = &lds[(row0 + k + 1) * GD_LDS + col + 1];
        const int m = min(min(__hip_atomic_load(c + GD_LDS, GD_RELAXED_WG), __hip_atomic_load(c - GD_LDS, GD_RELAXED_WG)),
                          min(__hip_atomic_load(c + 1, GD_RELAXED_WG), __hip_atomic_load(c - 1, GD_RELAXED_WG)));
        if (m < __hip_atomic_load(c, GD_RELAXED_WG) - 1) {              // (m < UNREACHED here, so m + 1 does not overflow)
          __hip_atomic_store(c, m + 1, GD_RELAXED_WG);
          fell = 1;
        }
      }
    }
    if (!__syncthreads_or(fell)) break;
  }

  // write back what fell: the outer ring, which the neighbours read as their halo, with relaxed agent-scope stores; the rest plainly
  int lowered = 0;
#pragma unroll
  for (int k = 0; k < GD_ROWS; ++k) {
    const int r = row0 + k;
    const int v = lds[(r + 1) * GD_LDS + col + 1];
    if (v < loaded[k]) {                                   // (only a routable cell inside the grid can have fallen)
      int* p = &dist[(size_t)(i0 + r) * ny + iy];
      if (r == 0 || r == GD_BLOCK - 1 || col == 0 || col == GD_BLOCK - 1) __hip_atomic_store(p, v, GD_RELAXED_AGENT);
      else *p = v;
      lowered = 1;
    }
  }
  lowered = __syncthreads_or(lowered);
  if (lowered && threadIdx.x == 0) __hip_atomic_store(&flags[bi * nby + bj], sweep, GD_RELAXED_AGENT);
}

// The call's last kernel, one workgroup per field: the number of blocks that lowered a value in the call's last sweep, and the field's
// sweep count moved on.  Only this workgroup reads or writes work[f] in this launch.
__global__ __launch_bounds__(GD_THREADS) void grid_distance_count_kernel(int n_fields, int n_blocks, int n_sweeps, int* __restrict__ work,
                                                                         int* __restrict__ changed) {
  const int f = blockIdx.x;
  const int last = work[f] + n_sweeps;
  const int* flags = gd_flags(work, n_fields, f, n_blocks);
  int n = 0;
  for (int b = threadIdx.x; b < n_blocks; b += GD_THREADS) n += flags[b] == last;
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  if (n) atomicAdd(&total, n);
  __syncthreads();
  if (threadIdx.x == 0) {
    changed[f] = total;
    work[f] = last;
  }
}

// ---- the descent: one lane per query (include/mmd_amd.h: mmd_grid_descend; descend_step: grid_route_dev.h) ----
// From the start cell, while d > 0: one step of the rule.  The loop runs at most dist[start] times, whatever the field holds: d falls
// by one per step.  The lanes of a wave walk unrelated cells: four scattered 4-byte loads per step and lane, no LDS, no atomics.
// The entry is walk_entry's, written out with its two exits: through walk_entry the compiler merges them, fetches every argument in front
// of the first and shares one reciprocal of `tile`, which moves the kernel's scalar-load and v_rcp counts off the figures on record.
__global__ __launch_bounds__(WALK_THREADS) void grid_descend_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                    const int2* __restrict__ starts, const int* __restrict__ field,
                                                                    int n_queries, int tile, int o_i, int o_j, int max_tiles,
                                                                    int2* __restrict__ tiles, int4* __restrict__ summary) {
  const int q = blockIdx.x * WALK_THREADS + threadIdx.x;
  if (q >= n_queries) return;
  const int2 s = starts[q];
  const int f = field[q];
  if (f < 0 || f >= n_fields || s.x < 0 || s.x >= nx || s.y < 0 || s.y >= ny) {
    summary[q] = make_int4(-1, 0, WALK_OUTSIDE, 0);
    return;
  }
  const int* dist = dist_all + (size_t)f * nx * ny;
  int ix = s.x, iy = s.y;
  const int d0 = dist[(size_t)ix * ny + iy];
  if (d0 == GRID_UNREACHED) {
    summary[q] = make_int4(-1, 0, WALK_UNREACHED_START, 0);
    return;
  }
  int2* out = tiles + (size_t)q * max_tiles;
  long long ta = floor_div((long long)ix - o_i, tile), tb = floor_div((long long)iy - o_j, tile);
  int n_tiles = 1, steps = 0, status = WALK_OK;
  out[0] = make_int2((int)ta, (int)tb);
  for (int d = d0; d > 0; --d) {
    const int r = descend_step(dist, nx, ny, tile, o_i, o_j, d, ix, iy, ta, tb);
    if (r < 0) { status = WALK_STUCK; break; }
    ++steps;
    if (r == 0) {
      if (n_tiles < max_tiles) out[n_tiles] = make_int2((int)ta, (int)tb);
      ++n_tiles;
    }
  }
  if (status == WALK_OK && n_tiles > max_tiles) status = WALK_TILES;
  summary[q] = make_int4(steps, n_tiles, status, 0);
}

static bool region_ok(const int32_t r[4], int nx, int ny) {
  return r[0] >= 0 && r[0] <= r[2] && r[2] <= nx && r[1] >= 0 && r[1] <= r[3] && r[3] <= ny;
}

}  // namespace mmd

using namespace mmd;

extern "C" {

size_t mmd_grid_distance_work_bytes(int nx, int ny, int n_fields) {
  if (nx < 1 || ny < 1 || nx > MMD_OCCUPANCY_MAX_SIDE || ny > MMD_OCCUPANCY_MAX_SIDE || n_fields < 0 || n_fields > MMD_GRID_DIST_MAX_FIELDS)
    return 0;
  const size_t n_blocks = (size_t)((nx + GD_BLOCK - 1) / GD_BLOCK) * ((ny + GD_BLOCK - 1) / GD_BLOCK);
  return (size_t)n_fields * (1 + n_blocks) * sizeof(int32_t);
}

int mmd_grid_distance_field(const float* grid_dev, int nx, int ny, float clearance, const int32_t region[4], const int32_t* goals_dev,
                            int n_fields, int restart, int n_sweeps, int32_t* dist_dev, void* work_dev, size_t work_bytes,
                            int32_t* changed_dev, void* stream) {
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "mmd_grid_distance_field: a grid of %d x %d cells (1 to %d per side)", nx, ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(n_fields >= 0 && n_fields <= MMD_GRID_DIST_MAX_FIELDS, "mmd_grid_distance_field: n_fields = %d (0 to %d: the field is a block index)",
              n_fields, MMD_GRID_DIST_MAX_FIELDS);
  MMD_REQUIRE(n_sweeps >= 0, "mmd_grid_distance_field: n_sweeps = %d (>= 0)", n_sweeps);
  MMD_REQUIRE(fabsf(clearance) <= FLT_MAX, "mmd_grid_distance_field: clearance = %g (finite)", (double)clearance);
  MMD_REQUIRE(region, "mmd_grid_distance_field: NULL region");
  MMD_REQUIRE(region_ok(region, nx, ny), "mmd_grid_distance_field: region (%d, %d) .. (%d, %d) (lo <= hi, inside 0 .. %d and 0 .. %d)",
              region[0], region[1], region[2], region[3], nx, ny);
  if (n_fields == 0) return 0;
  MMD_REQUIRE(grid_dev, "mmd_grid_distance_field: NULL grid");
  MMD_REQUIRE(goals_dev, "mmd_grid_distance_field: NULL goals");
  MMD_REQUIRE(dist_dev, "mmd_grid_distance_field: NULL dist");
  MMD_REQUIRE(work_dev, "mmd_grid_distance_field: NULL workspace");
  MMD_REQUIRE(changed_dev, "mmd_grid_distance_field: NULL changed");
  MMD_REQUIRE(work_bytes >= mmd_grid_distance_work_bytes(nx, ny, n_fields),
              "mmd_grid_distance_field: work_bytes = %zu, below mmd_grid_distance_work_bytes(%d, %d, %d) = %zu", work_bytes, nx, ny, n_fields,
              mmd_grid_distance_work_bytes(nx, ny, n_fields));
  if (n_sweeps == 0 && !restart) return 0;
  const int nbx = (nx + GD_BLOCK - 1) / GD_BLOCK, nby = (ny + GD_BLOCK - 1) / GD_BLOCK, n_blocks = nbx * nby;
  const GridRegion rg = {region[0], region[1], region[2], region[3]};
  const float4* tex = (const float4*)grid_dev;
  int* work = (int*)work_dev;
  hipStream_t st = (hipStream_t)stream;
  if (restart) {
    hipLaunchKernelGGL(grid_distance_init_kernel, dim3((nx * ny + GD_THREADS - 1) / GD_THREADS, n_fields), dim3(GD_THREADS), 0, st, tex, nx, ny,
                       clearance, rg, (const int2*)goals_dev, n_fields, nby, n_blocks, dist_dev, work);
    MMD_HIP_CHECK(hipGetLastError());
  }
  for (int k = 0; k < n_sweeps; ++k) {
    hipLaunchKernelGGL(grid_distance_sweep_kernel, dim3(nby, nbx, n_fields), dim3(GD_THREADS), 0, st, tex, nx, ny, clearance, rg, n_fields, k,
                       dist_dev, work);
    MMD_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(grid_distance_count_kernel, dim3(n_fields), dim3(GD_THREADS), 0, st, n_fields, n_blocks, n_sweeps, work, changed_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_grid_descend(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev, const int32_t* field_dev, int n_queries,
                     int tile, const int32_t lattice_origin[2], int max_tiles, int32_t* tiles_dev, int32_t* summary_dev, void* stream) {
  if (const int refused = descend_args("mmd_grid_descend", dist_dev, nx, ny, n_fields, starts_dev, field_dev, n_queries, tile, lattice_origin,
                                       max_tiles, 0, tiles_dev, summary_dev))
    return refused;
  if (n_queries == 0) return 0;
  hipLaunchKernelGGL(grid_descend_kernel, dim3((n_queries + WALK_THREADS - 1) / WALK_THREADS), dim3(WALK_THREADS), 0, (hipStream_t)stream,
                     (const int*)dist_dev, nx, ny, n_fields, (const int2*)starts_dev, (const int*)field_dev, n_queries, tile,
                     lattice_origin[0], lattice_origin[1], max_tiles, (int2*)tiles_dev, (int4*)summary_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
