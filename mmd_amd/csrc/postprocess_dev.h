// The device fragments of the post-sampling selection that more than one kernel uses (postprocess.hip: postprocess_kernel, select_best_kernel,
// unnormalize_kernel; round_pick.hip: the round's pick in two kernels): the map / workspace occupancy of a point, a segment's interpolated points,
// the joint limits, a segment's length and smoothness terms, the un-normalisation, and the order and the scan of the per-robot pick.  One text
// each, so a decision or a rounding made twice is made the same way twice.  Every fp32 operation is the one written out (no FMA contraction).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mmd_amd.h"
#include "common.h"

// before guide_dev.h: its extra_sdf decides occupancy here, operation for operation (guide.hip keeps its own contraction)
#pragma clang fp contract(off)

#include "guide_dev.h"
#include "wave_dev.h"             // wave_sum

namespace mmd {

constexpr int MAX_INTERP = 16;

struct EnvDev {
  float lo[2], dim[2];
  int nx, ny, n_grids;
  const float4* grids;        // [n_maps][n_grids][nx][ny]
  const int* robot_map;       // per-robot map index or null
  float ws_min[2], ws_max[2];
  const float4* xs;           // the env's extra objects (mmd_guide_desc.extra_spheres_dev / extra_boxes_dev)
  const float4* xb;
  int n_xs, n_xb;
};

static int fill_env(const mmd_guide_desc* d, EnvDev& e) {
  MMD_REQUIRE(d->n_grids == 0 || (d->sdf_grids_dev && d->grid_nx >= 1 && d->grid_ny >= 1), "postprocess: SDF grid missing");
  for (int k = 0; k < 2; ++k) {
    e.lo[k] = d->limits_lo[k];
    e.dim[k] = fabsf(d->limits_hi[k] - d->limits_lo[k]);
    e.ws_min[k] = d->ws_min[k];
    e.ws_max[k] = d->ws_max[k];
  }
  e.nx = d->grid_nx; e.ny = d->grid_ny; e.n_grids = d->n_grids;
  e.grids = reinterpret_cast<const float4*>(d->sdf_grids_dev);
  e.robot_map = d->robot_map_dev;
  e.xs = reinterpret_cast<const float4*>(d->extra_spheres_dev); e.n_xs = d->extra_spheres_dev ? d->n_extra_spheres : 0;
  e.xb = reinterpret_cast<const float4*>(d->extra_boxes_dev); e.n_xb = d->extra_boxes_dev ? d->n_extra_boxes : 0;
  return 0;
}

// the SDF grids of `robot`'s map
__device__ __forceinline__ const float4* robot_grid(const EnvDev& e, int robot) {
  const int map = e.robot_map ? e.robot_map[robot] : 0;
  return e.grids + (size_t)map * e.n_grids * e.nx * e.ny;
}

// occupancy of one point: any fixed-object SDF (nearest cell) or any of the 4 workspace-boundary distances below `margin`
__device__ __forceinline__ bool point_collides(const EnvDev& e, const float4* __restrict__ grid, float px, float py,
                                               float margin) {
  bool c = false;
  if (e.n_grids > 0) {
    int ix = (int)floorf((px - e.lo[0]) / e.dim[0] * (float)e.nx);
    int iy = (int)floorf((py - e.lo[1]) / e.dim[1] * (float)e.ny);
    ix = min(max(ix, 0), e.nx - 1);
    iy = min(max(iy, 0), e.ny - 1);
    for (int k = 0; k < e.n_grids; ++k) c = c || grid[((size_t)k * e.nx + ix) * e.ny + iy].x < margin;
  }
  if (e.n_xs + e.n_xb > 0) {                                // env.get_df_obj_list(): the fixed grid + obj_extra_list
    float gx, gy;
    c = c || extra_sdf<true>(e.xs, e.n_xs, e.xb, e.n_xb, px, py, gx, gy) < margin;
  }
  c = c || (px - e.ws_min[0] < margin) || (py - e.ws_min[1] < margin) || (e.ws_max[0] - px < margin) ||
      (e.ws_max[1] - py < margin);
  return c;
}

__device__ __forceinline__ float lane_next_f(float v) {   // lane t reads lane t + 1 (wave_shl:1)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

// interpolated point j of the segment a -> b, one coordinate: a * alpha + b * (1 - alpha)   (trajectory/utils.py:80-81)
__device__ __forceinline__ float interp_coord(float a, float b, float alpha, float one_minus_alpha) { return a * alpha + b * one_minus_alpha; }

// joint limits of a support point (tasks.py:270-276)
__device__ __forceinline__ bool inside_limits(float x, float y, const float* q_min, const float* q_max) {
  return x >= q_min[0] && x <= q_max[0] && y >= q_min[1] && y <= q_max[1];
}

// a segment's terms of the path length and of the smoothness: || diff ||  (metrics.py:13-14, :36-38)
__device__ __forceinline__ void segment_costs(const float4& x, float nx, float ny, float nz, float nw, float& pl, float& sm) {
  const float dx = nx - x.x, dy = ny - x.y, dvx = nz - x.z, dvy = nw - x.w;
  pl = sqrtf(dx * dx + dy * dy);
  sm = sqrtf(dvx * dvx + dvy * dvy);
}

// x_u = (x + 1) / 2 * (max - min) + min, every operation rounded on its own as torch does
struct UnnormArgs { float mins[4], range[4]; };
__device__ __forceinline__ float unnorm_coord(float v, const UnnormArgs& a, int d) {
  v = (v + 1.f) / 2.f;
  return v * a.range[d] + a.mins[d];
}

// the order of torch.argmin over (key, index): a NaN key comes before every number, the lower index before the higher among
// equal keys (and among NaNs).  An empty candidate (+inf, 0x7fffffff) comes after every real one.
__device__ __forceinline__ bool pick_before(float ka, int ia, float kb, int ib) {
  const bool na = ka != ka, nb = kb != kb;
  if (na != nb) return na;
  return ka < kb || ((na || ka == kb) && ia < ib);
}

// One wave's pick among B samples: is_free(b) and key(b) describe sample b.  The candidates are the free samples, or all of them when none
// is free; the winner is the first in pick_before's order.  -> the pick (-1: B = 0) on every lane, nf = the number of free samples.
template <class Free, class Key>
__device__ __forceinline__ int wave_pick(int B, Free is_free, Key key, int& nf) {
  const int lane = threadIdx.x & 63;
  nf = 0;
  for (int b = lane; b < B; b += 64) nf += is_free(b) ? 1 : 0;
  nf = wave_sum(nf);
  float best = INFINITY;
  int best_i = 0x7fffffff;
  for (int b = lane; b < B; b += 64) {
    if (nf > 0 && !is_free(b)) continue;
    const float k = key(b);
    if (pick_before(k, b, best, best_i)) { best = k; best_i = b; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ob = __shfl_xor(best, m);
    const int oi = __shfl_xor(best_i, m);
    if (pick_before(ob, oi, best, best_i)) { best = ob; best_i = oi; }
  }
  return best_i == 0x7fffffff ? -1 : best_i;
}

}  // namespace mmd
