// The cell index of a cell table (include/mmd_amd.h: mmd_cons_bins), shared by the kernel that builds the table, the guided step that
// walks it (guide.hip) and the collision kernels that walk it (multi_agent.hip): one function, so every walker looks where the builder put.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"

namespace mmd {

// clamp(floor((p - lo) * inv_cell), 0, n - 1) in fp32, per axis; the argument why a point's own cell list covers everything within the
// table's radius is written out in guide.hip (COVER).  No add behind the product: the value does not depend on fp contraction.
__device__ __forceinline__ int bin_cell(float p, float lo, float inv_cell, int n) {
  return (int)fminf(fmaxf(floorf((p - lo) * inv_cell), 0.f), (float)(n - 1));
}

// a cell table as a kernel may walk it: every field but the two device arrays' contents (guide.hip)
int check_cons_bins(const mmd_cons_bins* b);

}  // namespace mmd
