// The workspace of mmd_grid_window_goals_apart, which mmd_grid_window_goals_aside reads (window_apart.hip, window_aside.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/mmd_amd.h"

namespace mmd {

constexpr int WA_MAX_STEPS = MMD_WINDOW_APART_MAX_STEPS, WA_MAX_SEP = MMD_WINDOW_APART_MAX_SEP;
constexpr int WA_MOVED = 1, WA_CLEAR = 2;                  // the bits of a robot's flag word

// The workspace of a call on n queries, in this order (every part is a multiple of 16 bytes from the 16-byte aligned base but the last
// four, which need 8 and 4):
//   meta   int4 [n]                  (steps, remaining, status, 0): window_goals' summary words of the plain walk
//   paths  int2 [n][max_steps + 1]   the cells of the walk, c[0 .. steps]; cells behind `steps` are never written and never read
//   origin int2 [n]
//   k      int  [2][n]               the two buffers of the sweeps; a call begins and ends with the state in buffer 0
//   flag   int  [n]                  WA_MOVED: k moved in the last sweep (after a restart: the query takes part); WA_CLEAR
struct ApartWork {
  int4* meta;
  int2* paths;
  int2* origin;
  int* k[2];
  int* flag;
};

__host__ __device__ inline size_t apart_row(int max_steps) { return (size_t)max_steps + 1; }

static inline size_t apart_work_bytes(int n, int max_steps) {
  return (size_t)n * (sizeof(int4) + apart_row(max_steps) * sizeof(int2) + sizeof(int2) + 3 * sizeof(int));
}

static inline ApartWork apart_work(void* base, int n, int max_steps) {
  ApartWork w;
  w.meta = (int4*)base;
  w.paths = (int2*)(w.meta + n);
  w.origin = w.paths + (size_t)n * apart_row(max_steps);
  w.k[0] = (int*)(w.origin + n);
  w.k[1] = w.k[0] + n;
  w.flag = w.k[1] + n;
  return w;
}

}  // namespace mmd
