// What the kernels of window_apart.hip and window_aside.hip share on the device: the conflict test and its cull, the clamps of the
// workspace's indices, and the words a query emits.  The workspace itself is window_apart_work.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "window_apart_work.h"
#include "window_walk_dev.h"

namespace mmd {

// two cells conflict iff dx^2 + dy^2 < sep^2.  The squares are taken in 64 bits: cells of a taking-part walk lie in the grid, but the
// words are device data.
__device__ __forceinline__ bool cells_conflict(int2 a, int2 b, long long sep2) {
  const long long dx = (long long)a.x - b.x, dy = (long long)a.y - b.y;
  return dx * dx + dy * dy < sep2;
}

// the cull: is b within `far` cells (Chebyshev) of s?
__device__ __forceinline__ bool cell_near(int2 b, int2 s, long long far) {
  return max(llabs((long long)b.x - s.x), llabs((long long)b.y - s.y)) <= far;
}

// Every index read from device memory is clamped before it is used: the cells query q's walk covered, and a k of it out of a k buffer
// (k_in_row: into its row, whatever the walk covered; k_of: into the cells covered).
__device__ __forceinline__ int walked_of(const ApartWork& w, int q, int max_steps) { return min(max(w.meta[q].x, 0), max_steps); }
__device__ __forceinline__ int k_in_row(const int* k_buffer, int q, int max_steps) { return min(max(k_buffer[q], 0), max_steps); }
__device__ __forceinline__ int k_of(const int* k_buffer, const ApartWork& w, int q, int max_steps) {
  return min(max(k_buffer[q], 0), walked_of(w, q, max_steps));
}

// The words a query emits, from its meta word m (the plain walk's summary), its row and the state's k buffer.  ok: the query takes part;
// one that does not gets window_goals' words and extra (steps, 0).  The k and the flag word are loaded only where they are read.
//   emitted_k      the index of the cell reported: the buffer's k, clamped into the cells covered; without part the walk's last; -1: none
//   emitted_cell   the cell at that index
//   summary_at     (k, d0 - k, status, arrived) of a query that takes part; one that does not keeps m's (steps, remaining, status, 0)
//   emitted_extra  (walked, clear)
__device__ __forceinline__ int emitted_k(int4 m, bool ok, const int* k_buffer, int q, int max_steps) {
  const int walked = min(max(m.x, -1), max_steps);
  return ok ? min(max(k_buffer[q], 0), max(walked, 0)) : walked;
}

__device__ __forceinline__ int2 emitted_extra(const ApartWork& w, int q, int4 m, bool ok) {
  return make_int2(m.x, ok && (w.flag[q] & WA_CLEAR) ? 1 : 0);
}

__device__ __forceinline__ int2 emitted_cell(const int2* row, int k) { return k >= 0 ? row[k] : make_int2(0, 0); }

__device__ __forceinline__ int4 summary_at(int4 m, int k, int max_steps) {
  const int walked = min(max(m.x, -1), max_steps);
  return make_int4(k, m.y + (walked - k), WALK_OK, m.y + (walked - k) == 0);
}

}  // namespace mmd
