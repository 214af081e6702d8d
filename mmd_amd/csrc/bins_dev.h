// The cell lookup of a cell table (include/mmd_amd.h: mmd_cons_bins), shared by the kernel that builds the table (cons_tables.hip) and the
// kernels that walk it (guide.hip, multi_agent.hip, cons_tables.hip): one text, so every walker looks where the builder put.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"

namespace mmd {

// clamp(floor((p - lo) * inv_cell), 0, n - 1) in fp32, per axis; the argument why a point's own cell list covers everything within the
// table's radius is written out in guide.hip (COVER).  No add behind the product: the value does not depend on fp contraction.
__device__ __forceinline__ int bin_cell(float p, float lo, float inv_cell, int n) {
  return (int)fminf(fmaxf(floorf((p - lo) * inv_cell), 0.f), (float)(n - 1));
}

// the list of the cell of p at time step t: entries [e0, e1) of `ent`, each (qx, qy, bit pattern of the robot id, 0), in ascending id
struct CellList {
  const float4* ent;
  int e0, e1;
};
__device__ __forceinline__ CellList own_cell_list(const mmd_cons_bins& b, int t, float px, float py) {
  const int cell = bin_cell(px, b.lo[0], b.inv_cell[0], b.nx) * b.ny + bin_cell(py, b.lo[1], b.inv_cell[1], b.ny);
  const int* off = b.cell_off_dev + (size_t)t * (b.nx * b.ny + 1) + cell;
  return CellList{reinterpret_cast<const float4*>(b.entries_dev) + (size_t)t * 9 * b.n_all, off[0], off[1]};
}

// a cell table as a kernel may walk it: every field but the two device arrays' contents (cons_tables.hip)
int check_cons_bins(const mmd_cons_bins* b);
// ... and as a kernel may take collision decisions at `margin` on it (COVER, multi_agent.hip); `who`: the entry point, for the error text
int check_collision_bins(const char* who, const mmd_cons_bins* bins, float margin);

}  // namespace mmd
