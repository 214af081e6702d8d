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

// ---- world maps: robot windows cut from one resident world texture, and the texel of a point (include/mmd_amd.h: mmd_sdf_grid_windows,
// ---- mmd_sdf_grid_lookup).  Two memory-bound kernels: no LDS, no atomics, no scratch.
constexpr int WIN_THREADS = 256;

// The clamped gather windows[k][ix][iy] = world[clamp(i0_k + ix)][clamp(j0_k + iy)], one thread per output texel, cell = ix * ny + iy: a
// wave stores 64 consecutive 16-byte texels and, off the world's border, loads 64 consecutive ones of a world row (two row segments where
// the wave crosses a window row's end).  The window is blockIdx.y, so the origin is one wave-uniform 8-byte scalar load.  The texel
// travels as four 32-bit words: NaN payloads and the sign of a zero survive.  The origin is device data and may be anything: it is
// clamped to [-nx, wnx] first (the same texel as without, and i0 + ix then cannot overflow).
__global__ __launch_bounds__(WIN_THREADS) void sdf_grid_windows_kernel(const uint4* __restrict__ world, int wnx, int wny,
                                                                       const int2* __restrict__ origins, int nx, int ny, int n_cells,
                                                                       uint4* __restrict__ windows) {
  const int cell = blockIdx.x * WIN_THREADS + threadIdx.x;
  if (cell >= n_cells) return;
  const int k = blockIdx.y;
  const int2 o = origins[k];
  const int i0 = min(max(o.x, -nx), wnx), j0 = min(max(o.y, -ny), wny);
  const int ix = cell / ny, iy = cell - ix * ny;
  const int sx = min(max(i0 + ix, 0), wnx - 1), sy = min(max(j0 + iy, 0), wny - 1);
  windows[(size_t)k * n_cells + cell] = world[(size_t)sx * wny + sy];
}

// The texel every consumer of a texture reads for a point (guide.hip's gather, postprocess.hip: point_collides): per axis
// floor((p - lo) / |hi - lo| * n) in fp32, clamped to [0, n - 1] -- clamped as a float and then converted, the same integer as
// clamp((int)floorf(..)) wherever that conversion is defined, and defined for every finite p.  One thread per point: an 8-byte load, one
// 16-byte gather, one 16-byte store.  A point with a non-finite coordinate: four NaNs and no gather.
__global__ __launch_bounds__(WIN_THREADS) void sdf_grid_lookup_kernel(const float4* __restrict__ grid, int nx, int ny, float lo_x, float lo_y,
                                                                      float dim_x, float dim_y, const float2* __restrict__ points,
                                                                      int n_points, float4* __restrict__ out) {
  const int i = blockIdx.x * WIN_THREADS + threadIdx.x;
  if (i >= n_points) return;
  const float2 p = points[i];
  if (!(fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX)) {
    const float nan = __builtin_nanf("");
    out[i] = make_float4(nan, nan, nan, nan);
    return;
  }
  const int ix = (int)fminf(fmaxf(floorf((p.x - lo_x) / dim_x * (float)nx), 0.f), (float)(nx - 1));
  const int iy = (int)fminf(fmaxf(floorf((p.y - lo_y) / dim_y * (float)ny), 0.f), (float)(ny - 1));
  out[i] = grid[(size_t)ix * ny + iy];
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

int mmd_sdf_grid_windows(const float* world_grid_dev, int wnx, int wny, const int32_t* origins_dev, int n_windows, int nx, int ny,
                         float* windows_dev, void* stream) {
  MMD_REQUIRE(n_windows >= 0 && n_windows <= MMD_SDF_GRID_MAX_WINDOWS, "mmd_sdf_grid_windows: n_windows = %d (0 to %d: the window is a block index)",
              n_windows, MMD_SDF_GRID_MAX_WINDOWS);
  MMD_REQUIRE(wnx >= 1 && wny >= 1, "mmd_sdf_grid_windows: a world of %d x %d texels (at least 1 x 1)", wnx, wny);
  MMD_REQUIRE(nx >= 1 && ny >= 1 && nx <= wnx && ny <= wny, "mmd_sdf_grid_windows: windows of %d x %d texels (1 x 1 up to the world's %d x %d)",
              nx, ny, wnx, wny);
  MMD_REQUIRE((long long)wnx * wny <= INT_MAX - WIN_THREADS, "mmd_sdf_grid_windows: a world of %d x %d texels does not fit a 32-bit index", wnx,
              wny);
  if (n_windows == 0) return 0;
  MMD_REQUIRE(world_grid_dev, "mmd_sdf_grid_windows: NULL world grid");
  MMD_REQUIRE(origins_dev, "mmd_sdf_grid_windows: NULL origins");
  MMD_REQUIRE(windows_dev, "mmd_sdf_grid_windows: NULL windows");
  const int n_cells = nx * ny;                 // (<= wnx * wny)
  hipLaunchKernelGGL(sdf_grid_windows_kernel, dim3((n_cells + WIN_THREADS - 1) / WIN_THREADS, n_windows), dim3(WIN_THREADS), 0,
                     (hipStream_t)stream, (const uint4*)world_grid_dev, wnx, wny, (const int2*)origins_dev, nx, ny, n_cells,
                     (uint4*)windows_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_sdf_grid_lookup(const float* grid_dev, int nx, int ny, const float lo[2], const float hi[2], const float* points_dev, int n_points,
                        float* out_dev, void* stream) {
  MMD_REQUIRE(n_points >= 0 && n_points <= INT_MAX - WIN_THREADS, "mmd_sdf_grid_lookup: n_points = %d (0 to 2^31 - 257)", n_points);
  MMD_REQUIRE(nx >= 1 && ny >= 1, "mmd_sdf_grid_lookup: a grid of %d x %d texels (at least 1 x 1)", nx, ny);
  MMD_REQUIRE((long long)nx * ny <= INT_MAX, "mmd_sdf_grid_lookup: a grid of %d x %d texels does not fit a 32-bit index", nx, ny);
  MMD_REQUIRE(lo && hi, "mmd_sdf_grid_lookup: NULL limits");
  const float dim_x = fabsf(hi[0] - lo[0]), dim_y = fabsf(hi[1] - lo[1]);
  MMD_REQUIRE(fabsf(lo[0]) <= FLT_MAX && fabsf(lo[1]) <= FLT_MAX && dim_x > 0.f && dim_x <= FLT_MAX && dim_y > 0.f && dim_y <= FLT_MAX,
              "mmd_sdf_grid_lookup: limits (%g, %g) .. (%g, %g) (finite, a non-zero extent per axis)", (double)lo[0], (double)lo[1],
              (double)hi[0], (double)hi[1]);
  if (n_points == 0) return 0;
  MMD_REQUIRE(grid_dev, "mmd_sdf_grid_lookup: NULL grid");
  MMD_REQUIRE(points_dev, "mmd_sdf_grid_lookup: NULL points");
  MMD_REQUIRE(out_dev, "mmd_sdf_grid_lookup: NULL out");
  hipLaunchKernelGGL(sdf_grid_lookup_kernel, dim3((n_points + WIN_THREADS - 1) / WIN_THREADS), dim3(WIN_THREADS), 0, (hipStream_t)stream,
                     (const float4*)grid_dev, nx, ny, lo[0], lo[1], dim_x, dim_y, (const float2*)points_dev, n_points, (float4*)out_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
