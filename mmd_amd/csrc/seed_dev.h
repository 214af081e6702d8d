// What the seed kernels of route_seeds.hip and window_seeds.hip and the sample kernels of route_seeds.hip and window_goals.hip share: the
// texel of a point, the order of texel values, and the cursor over a path's 64 support cells.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"
// every float operation below is one rounding, as in the files that include this: no fused multiply-add
#pragma clang fp contract(off)

namespace mmd {

// The texel of a point: sdf_grid.hip's sdf_grid_lookup_kernel, operation for operation (fmaxf drops a NaN: index 0)
struct SeedGrid { int nx, ny; float lo_x, lo_y, dim_x, dim_y, pitch_x, pitch_y; };
__device__ __forceinline__ int2 seed_texel(const SeedGrid& g, float2 p) {
  return make_int2((int)fminf(fmaxf(floorf((p.x - g.lo_x) / g.dim_x * (float)g.nx), 0.f), (float)(g.nx - 1)),
                   (int)fminf(fmaxf(floorf((p.y - g.lo_y) / g.dim_y * (float)g.ny), 0.f), (float)(g.ny - 1)));
}

// The 64 support cells of a cell path, emitted by the walk that passes them.  Support point j of a path of m cells is the path's cell
// number off(j) = (j * (m - 1) + 31) / 63, monotone in j.  The walk stands on cell number t, at (ix, iy), and has emitted every j with
// off(j) < t: the next j belongs to t iff j * (m - 1) + 31 < (t + 1) * 63 (in 64 bits: m and t are device data).  j only grows: at most
// 64 emissions per row in all.
__device__ __forceinline__ void emit_samples(int2* __restrict__ row, int& j, int m, int t, int ix, int iy) {
  while (j < MMD_ROUTE_SEED_POINTS && (long long)j * (m - 1) + 31 < ((long long)t + 1) * 63) row[j++] = make_int2(ix, iy);
}

// a float's bits as an int32 that orders like the float (-0 below +0, a NaN beyond the infinity of its sign); its own inverse
__device__ __forceinline__ int order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

}  // namespace mmd
