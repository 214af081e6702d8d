// The one fp32 form of the robot-robot collision decision, shared by every kernel that makes it (multi_agent.hip, trial_stats.hip, cons_tables.hip).
#pragma once
#include <hip/hip_runtime.h>

// Every fp32 operation here is the one written out: the collision decision ||pa - pb|| < margin must be torch.norm's own rounding.
#pragma clang fp contract(off)

namespace mmd {

// torch.norm(pa - pb, dim=-1) over (dx, dy) in fp32: sqrt(fma(dy, dy, dx * dx)), the form of check_rr_collisions / get_conflicts.
// Any other order (dx * dx + dy * dy rounded twice, or fma(dx, dx, dy * dy)) moves pairs within an ulp of the margin across it.
__device__ __forceinline__ float torch_norm2(float dx, float dy) { return sqrtf(__builtin_fmaf(dy, dy, dx * dx)); }

// the collision test of rr_collisions_kernel, operation for operation
__device__ __forceinline__ bool rr_hit(float2 a, float2 b, float margin) {
  const float dx = a.x - b.x, dy = a.y - b.y;
  return torch_norm2(dx, dy) < margin;
}

}  // namespace mmd
