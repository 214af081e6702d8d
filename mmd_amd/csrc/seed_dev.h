// What the seed kernels of route_seeds.hip and window_seeds.hip share: the texel of a point and the order of texel values.
#pragma once
#include <hip/hip_runtime.h>
// every float operation below is one rounding, as in the files that include this: no fused multiply-add
#pragma clang fp contract(off)

namespace mmd {

// The texel of a point: sdf_grid.hip's sdf_grid_lookup_kernel, operation for operation (fmaxf drops a NaN: index 0)
struct SeedGrid { int nx, ny; float lo_x, lo_y, dim_x, dim_y, pitch_x, pitch_y; };
__device__ __forceinline__ int2 seed_texel(const SeedGrid& g, float2 p) {
  return make_int2((int)fminf(fmaxf(floorf((p.x - g.lo_x) / g.dim_x * (float)g.nx), 0.f), (float)(g.nx - 1)),
                   (int)fminf(fmaxf(floorf((p.y - g.lo_y) / g.dim_y * (float)g.ny), 0.f), (float)(g.ny - 1)));
}

// a float's bits as an int32 that orders like the float (-0 below +0, a NaN beyond the infinity of its sign); its own inverse
__device__ __forceinline__ int order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

}  // namespace mmd
