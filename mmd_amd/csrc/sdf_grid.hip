// The SDF grid of a custom map, built on the device.  From an occupancy bitmap: the second half of this file.  From primitives
// (include/mmd_amd.h: mmd_sdf_grid_build): GridMapSDF.precompute_sdf
// (grid_map_sdf.py:34-63) for one ObjectField([MultiSphereField, MultiBoxField]), value and torch-autograd gradient per node, bit for bit
// (but for the sign of a zero) what mmd_amd/environments.py::sdf_grid_texture computes on the host (tests/sdf_grid_model.py is the same operation sequence in numpy).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/mmd_amd.h"
#include "common.h"
// before guide_dev.h: its extra_sdf<true> is the grid's arithmetic, operation for operation
#pragma clang fp contract(off)
#include "guide_dev.h"

namespace mmd {

// One thread per node, node = ix * ny + iy: a wave stores 64 consecutive float4.  The primitive tables are read at a wave-uniform index
// (every lane walks the same list), so their loads are scalar and a primitive costs each lane its arithmetic alone: no LDS, no atomics.
// extra_sdf<true> is the sphere-then-box first minimum with torch's sub-gradients (guide_dev.h); on top of it
//   - an empty sphere field is the constant 1 with gradient 0, FIRST in ObjectField's min (primitives.py:109-110, :569-572): it keeps a
//     node whose box distance is not below 1;
//   - a zero gradient component is +0 (extra_sdf's 0 / n * -1 is -0; autograd leaves either sign, by how many primitives it sums
//     over): x + 0 in round-to-nearest.
constexpr int SDF_GRID_THREADS = 256;
__global__ __launch_bounds__(SDF_GRID_THREADS) void sdf_grid_kernel(const float4* __restrict__ spheres, int n_spheres,
                                                                    const float4* __restrict__ boxes, int n_boxes,
                                                                    const float* __restrict__ xs, const float* __restrict__ ys, int ny,
                                                                    int n_nodes, float4* __restrict__ grid) {
  const int node = blockIdx.x * SDF_GRID_THREADS + threadIdx.x;
  if (node >= n_nodes) return;
  const int ix = node / ny, iy = node - ix * ny;
  float gx, gy;
  float d = extra_sdf<true>(spheres, n_spheres, boxes, n_boxes, xs[ix], ys[iy], gx, gy);
  if (n_spheres == 0 && !(d < 1.f)) { d = 1.f; gx = 0.f; gy = 0.f; }
  grid[node] = make_float4(d, gx + 0.f, gy + 0.f, 0.f);
}

// ---- occupancy bitmaps: exact Euclidean distance transform with nearest-site tracking (include/mmd_amd.h: mmd_sdf_grid_from_occupancy) ----
// For a cell, the site is the nearest cell of the OTHER class (a free cell's: occupied; an occupied cell's: free), by the integer
// D2 = dx^2 + dy^2, the lexicographically smallest (jx, jy) among equal D2.  Two passes over the separable form: pass 1 finds, per ix
// row, the signed iy offset to the row's nearest cell of each class (a tie to the smaller jy); pass 2 takes the first minimum over jx,
// ascending with a strict <, of (ix - jx)^2 + offset[jx][iy]^2 -- the smallest jx among equal D2 and, within that row, the smaller jy.
// Every decision is integer arithmetic on values that do not depend on the launch shape: no atomics, no LDS, no scratch.
constexpr int OCC_THREADS = 256;
constexpr int OCC_NONE = 1 << 14;            // the offset of "this row holds no such cell": its square, 2^28, is above every real D2
                                             // (< 2^23 for n <= 2048) and (ix - jx)^2 + 2^28 stays inside an int

// Pass 1, one thread per cell: walk outwards in the row, the smaller jy first at each distance, until both classes are found or the row
// ends.  The lanes of a wave read neighbouring bytes of one row (or two, at a row's end); a row without occupied (free) cells costs its
// lanes ny steps, what pass 2 spends per cell anyway.  No scan, no LDS staging: the build runs once per map, not per step.
__global__ __launch_bounds__(OCC_THREADS) void occupancy_rows_kernel(const unsigned char* __restrict__ occ, int ny, int n_nodes,
                                                                     short* __restrict__ to_occ, short* __restrict__ to_free) {
  const int node = blockIdx.x * OCC_THREADS + threadIdx.x;
  if (node >= n_nodes) return;
  const int ix = node / ny, iy = node - ix * ny;
  const unsigned char* row = occ + (size_t)ix * ny;
  int d_occ = OCC_NONE, d_free = OCC_NONE;
  for (int d = 0; d < ny && (d_occ == OCC_NONE || d_free == OCC_NONE); ++d) {
    if (iy - d >= 0) {
      const bool o = row[iy - d] != 0;
      if (o && d_occ == OCC_NONE) d_occ = -d;
      if (!o && d_free == OCC_NONE) d_free = -d;
    }
    if (iy + d < ny) {
      const bool o = row[iy + d] != 0;
      if (o && d_occ == OCC_NONE) d_occ = d;
      if (!o && d_free == OCC_NONE) d_free = d;
    }
  }
  to_occ[node] = (short)d_occ;
  to_free[node] = (short)d_free;
}

// Pass 2, one thread per cell, node = ix * ny + iy: at each jx a wave reads 64 consecutive int16 of table[jx][iy...] (the table of the
// other class, chosen per lane) and at the end stores 64 consecutive float4.  The jx loop is wave-uniform.  No site at all (the grid is
// all free, or all occupied) shows as a D2 that is still >= OCC_NONE^2: the constant field, decided here without a host round trip.
// fp32 sequence of the definition (environments.occupancy_sdf_texture), one rounding per operation: s = sqrt(float(D2)),
// v = cell * s - 0.5 * cell, gradient = float(integer offset) / s; a zero offset is the integer 0, so its component is +0.
__global__ __launch_bounds__(OCC_THREADS) void occupancy_sdf_kernel(const unsigned char* __restrict__ occ, const short* __restrict__ to_occ,
                                                                    const short* __restrict__ to_free, int nx, int ny, int n_nodes,
                                                                    float cell, float4* __restrict__ grid) {
  const int node = blockIdx.x * OCC_THREADS + threadIdx.x;
  if (node >= n_nodes) return;
  const int ix = node / ny, iy = node - ix * ny;
  const bool occupied = occ[node] != 0;
  const short* col = (occupied ? to_free : to_occ) + iy;
  int best = INT_MAX, best_dx = 0, best_dy = 0;
  for (int jx = 0; jx < nx; ++jx) {
    const int dy = col[(size_t)jx * ny], dx = jx - ix;
    const int d2 = dx * dx + dy * dy;
    if (d2 < best) { best = d2; best_dx = dx; best_dy = dy; }
  }
  float4 out;
  if (best >= OCC_NONE * OCC_NONE) {
    out = make_float4(occupied ? -1.f : 1.f, 0.f, 0.f, 0.f);
  } else {
    const float s = sqrtf((float)best);
    const float v = cell * s - 0.5f * cell;
    if (occupied) out = make_float4(-v, (float)best_dx / s, (float)best_dy / s, 0.f);         // towards the free site
    else if (!(v < 1.f)) out = make_float4(1.f, 0.f, 0.f, 0.f);                                // the primitive maps' constant-1 cap
    else out = make_float4(v, (float)-best_dx / s, (float)-best_dy / s, 0.f);                  // away from the occupied site
  }
  grid[node] = out;
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_sdf_grid_build(const float* spheres_dev, int n_spheres, const float* boxes_dev, int n_boxes, const float* xs_dev, int nx,
                       const float* ys_dev, int ny, float* grid_dev, void* stream) {
  MMD_REQUIRE(n_spheres >= 0 && (n_spheres == 0 || spheres_dev), "mmd_sdf_grid_build: n_spheres = %d %s", n_spheres,
              n_spheres < 0 ? "(>= 0)" : "without a sphere table");
  MMD_REQUIRE(n_boxes >= 0 && (n_boxes == 0 || boxes_dev), "mmd_sdf_grid_build: n_boxes = %d %s", n_boxes,
              n_boxes < 0 ? "(>= 0)" : "without a box table");
  MMD_REQUIRE(nx >= 1 && ny >= 1, "mmd_sdf_grid_build: a grid of %d x %d nodes (at least 1 x 1)", nx, ny);
  MMD_REQUIRE((long long)nx * ny <= INT_MAX - SDF_GRID_THREADS, "mmd_sdf_grid_build: %d x %d nodes do not fit a 32-bit index", nx, ny);
  MMD_REQUIRE(xs_dev && ys_dev, "mmd_sdf_grid_build: NULL node coordinates");
  MMD_REQUIRE(grid_dev, "mmd_sdf_grid_build: NULL grid");
  const int n_nodes = nx * ny;
  hipLaunchKernelGGL(sdf_grid_kernel, dim3((n_nodes + SDF_GRID_THREADS - 1) / SDF_GRID_THREADS), dim3(SDF_GRID_THREADS), 0,
                     (hipStream_t)stream, (const float4*)spheres_dev, n_spheres, (const float4*)boxes_dev, n_boxes, xs_dev, ys_dev, ny,
                     n_nodes, (float4*)grid_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

size_t mmd_sdf_grid_occupancy_work_bytes(int nx, int ny) {
  if (nx < 1 || ny < 1 || nx > MMD_OCCUPANCY_MAX_SIDE || ny > MMD_OCCUPANCY_MAX_SIDE) return 0;
  return (size_t)2 * nx * ny * sizeof(short);
}

int mmd_sdf_grid_from_occupancy(const unsigned char* occ_dev, int nx, int ny, float cell, float* grid_dev, void* work_dev,
                                size_t work_bytes, void* stream) {
  MMD_REQUIRE(occ_dev, "mmd_sdf_grid_from_occupancy: NULL occupancy");
  MMD_REQUIRE(grid_dev, "mmd_sdf_grid_from_occupancy: NULL grid");
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= MMD_OCCUPANCY_MAX_SIDE && ny <= MMD_OCCUPANCY_MAX_SIDE,
              "mmd_sdf_grid_from_occupancy: a grid of %d x %d cells (1 to %d per side: every squared distance is then an exact float)", nx,
              ny, MMD_OCCUPANCY_MAX_SIDE);
  MMD_REQUIRE(cell > 0.f && cell <= FLT_MAX, "mmd_sdf_grid_from_occupancy: cell = %g (finite and positive)", (double)cell);
  MMD_REQUIRE(work_dev, "mmd_sdf_grid_from_occupancy: NULL workspace");
  MMD_REQUIRE(work_bytes >= mmd_sdf_grid_occupancy_work_bytes(nx, ny),
              "mmd_sdf_grid_from_occupancy: work_bytes = %zu, below mmd_sdf_grid_occupancy_work_bytes(%d, %d) = %zu", work_bytes, nx, ny,
              mmd_sdf_grid_occupancy_work_bytes(nx, ny));
  const int n_nodes = nx * ny;
  short* to_occ = (short*)work_dev;
  short* to_free = to_occ + n_nodes;
  const dim3 blocks((n_nodes + OCC_THREADS - 1) / OCC_THREADS), threads(OCC_THREADS);
  hipLaunchKernelGGL(occupancy_rows_kernel, blocks, threads, 0, (hipStream_t)stream, occ_dev, ny, n_nodes, to_occ, to_free);
  MMD_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(occupancy_sdf_kernel, blocks, threads, 0, (hipStream_t)stream, occ_dev, (const short*)to_occ, (const short*)to_free,
                     nx, ny, n_nodes, cell, (float4*)grid_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
