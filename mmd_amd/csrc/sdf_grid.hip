// The SDF grid of a custom map, built on the device (include/mmd_amd.h: mmd_sdf_grid_build): GridMapSDF.precompute_sdf
// (grid_map_sdf.py:34-63) for one ObjectField([MultiSphereField, MultiBoxField]), value and torch-autograd gradient per node, bit for bit
// (but for the sign of a zero) what mmd_amd/environments.py::sdf_grid_texture computes on the host (tests/sdf_grid_model.py is the same operation sequence in numpy).
#include <hip/hip_runtime.h>

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

}  // extern "C"
