// What every builder of an ELL constraint table [slot][t] (include/mmd_amd.h: mmd_guide_desc.cons_ell_dev) must agree on with
// mmd_pack_constraints, each fragment written once: for cons_tables.hip and path_constraints_kernel (multi_agent.hip).  Sets no fp contract.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace mmd {

// The words of a slot.  An active point is (x, y, R, R|R|): the guided step tests dist^2 <= R|R| (guide.hip: cons_term).  An unused slot is
// (0, 0, -1, -1): R|R| < 0 <= dist^2, it never acts.  r * |r| is one product, no add behind it: the same bits on the host and the device.
__host__ __device__ __forceinline__ float slot_r2(float r) { return r * fabsf(r); }
__host__ __device__ __forceinline__ float4 slot_word(float x, float y, float r, float r2) { return make_float4(x, y, r, r2); }
__host__ __device__ __forceinline__ float4 slot_word(float x, float y, float r) { return slot_word(x, y, r, slot_r2(r)); }
__host__ __device__ __forceinline__ float4 empty_word() { return make_float4(0.f, 0.f, -1.f, -1.f); }
// the all-pairs rule (cbs.py:468-508): slot j of robot `self` holds the j-th OTHER robot in ascending id
__device__ __forceinline__ int all_pairs_other(int j, int self) { return j + (j >= self ? 1 : 0); }

// "one group of S slots per robot": the three offset arrays' entries of robot i of n_local, and behind the last robot the closing ones
__device__ __forceinline__ void one_group_per_robot(int i, int n_local, int S, float weight, int* __restrict__ grp_slot_off,
                                                    float* __restrict__ grp_weight, int* __restrict__ robot_grp_off) {
  grp_slot_off[i] = i * S; grp_weight[i] = weight; robot_grp_off[i] = i;
  if (i == n_local - 1) { grp_slot_off[n_local] = n_local * S; robot_grp_off[n_local] = n_local; }
}
// The column of a lane in the wave-per-robot builders (lane = time step t): slot s of the block at col[s * H].  A point goes to the lane's
// fill; once the block is full it is dropped and counted, and the fill stays at `cap`: what was written is a prefix of the lane's list.
struct ColumnWriter {
  float4* col;
  int fill, cap, dropped;
  __device__ __forceinline__ void push(float x, float y, float radius, float r2) {
    if (fill < cap) { col[(size_t)fill * H] = slot_word(x, y, radius, r2); ++fill; }
    else ++dropped;
  }
  __device__ __forceinline__ void fill_rest() { for (; fill < cap; ++fill) col[(size_t)fill * H] = empty_word(); }   // the unused slots
};
// host side: robots [robot0, robot0 + n_local) of n_all >= 2 (no sum that could overflow); `who` names the entry point in the error text
inline int check_robot_range(const char* who, int n_all, int robot0, int n_local) {
  MMD_REQUIRE(n_all >= 2 && n_local >= 1 && robot0 >= 0 && robot0 < n_all && n_local <= n_all - robot0, "%s: bad robot range", who);
  return 0;
}
// ... and the launch grid of a grid-stride builder over `items` words, 256 threads a block
inline int grid_for(size_t items) { return items > 2048 * 256 ? 2048 : (items < 256 ? 1 : (int)((items + 255) / 256)); }

}  // namespace mmd
