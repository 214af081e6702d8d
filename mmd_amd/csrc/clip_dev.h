// torch's clamp, min and max on one fp32 value: a NaN operand gives NaN.  fminf / fmaxf are IEEE minNum / maxNum, which return the OTHER
// operand, so a clamp written with them alone turns a NaN into one of its bounds.  Used by the DDPM step (guide_dev.h: ddpm_mean1, and
// through it the fused tail of unet_kernel.h), the cross conditioning (guide.hip) and the round pick (round_pick.hip).  Sets no fp contract.
#pragma once
#include <hip/hip_runtime.h>

namespace mmd {

// torch.clip(v, -1, 1) / x.clamp_(-1., 1.): a NaN passes through, +-inf goes to the bound
__device__ __forceinline__ float clip_unit(float v) { return v != v ? v : fminf(fmaxf(v, -1.f), 1.f); }

// torch.min(a, b) / torch.max(a, b), elementwise: NaN if either operand is
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

}  // namespace mmd
