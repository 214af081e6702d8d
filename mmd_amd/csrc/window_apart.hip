// World fleets: every epoch's sub-goals kept apart (include/mmd_amd.h: mmd_grid_window_goals_apart).  The definition is the numpy function
// subgoals_apart of mmd_amd/fleet_subgoals.py, and the state after s sweeps is subgoals_apart_sweeps(s); the fact a fleet rests on (starts
// pairwise `sep` apart give chosen cells pairwise `sep` apart) is argued there.  Every value here is an exact integer.  Plain loads and
// vector stores; no LDS, no atomics, no scratch, and nothing inside a launch waits on another workgroup.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/mmd_amd.h"
#include "common.h"
#include "walk_args.h"
#include "wave_dev.h"
#include "window_apart_dev.h"
#include "window_apart_work.h"
#include "window_walk_dev.h"

namespace mmd {

static_assert(WG_THREADS == 64 && MMD_ROUTE_SEED_POINTS == 64, "a wave's 64 lanes are 64 candidates, 64 blockers and 64 samples");
// (the workspace ApartWork: window_apart_work.h, which window_aside.hip reads as well)

// ---- 1. the paths: one lane per query ----
// grid_window_goals_kernel's walk (window_walk_dev.h: window_step), with every visited cell stored in the query's row.  The loop runs at
// most min(max_steps, d0) times, so the last index written is at most max_steps, the row's last.  A stuck walk keeps the cells it covered
// (window_goals reports its last one); a query outside the grid or on an unreached cell writes no cell.  Both k buffers start at
// `steps`, and the flag says "moved" for a query that takes part: nothing is proved before a sweep has run.
__global__ __launch_bounds__(WG_THREADS) void window_apart_paths_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                        const int2* __restrict__ starts, const int* __restrict__ field,
                                                                        const int2* __restrict__ goals, int n_queries, int reach,
                                                                        int max_steps, int window, ApartWork w) {
  const int q = blockIdx.x * WG_THREADS + threadIdx.x;
  if (q >= n_queries) return;
  const WalkEntry e = walk_entry(dist_all, nx, ny, n_fields, starts, field, q);
  if (e.d0 == GRID_UNREACHED) {
    w.meta[q] = make_int4(-1, -1, e.no_walk, 0);
    w.origin[q] = make_int2(0, 0);
    w.k[0][q] = w.k[1][q] = 0;
    w.flag[q] = 0;
    return;
  }
  int2* row = w.paths + (size_t)q * apart_row(max_steps);
  const int2 g = goals[e.f];
  int ix = e.s.x, iy = e.s.y, steps = 0, status = WALK_OK;
  row[0] = e.s;
  const int bound = min(max_steps, e.d0);
  for (int k = 0; k < bound; ++k) {
    const int r = window_step(e.dist, nx, ny, e.s, g, reach, e.d0 - k - 1, ix, iy);
    if (r < 0) status = WALK_STUCK;
    if (r != 1) break;
    row[++steps] = make_int2(ix, iy);
  }
  w.meta[q] = make_int4(steps, e.d0 - steps, status, 0);
  w.origin[q] = window_origin(e.s, nx, ny, window);
  w.k[0][q] = w.k[1][q] = status == WALK_OK ? steps : 0;
  w.flag[q] = status == WALK_OK ? WA_MOVED : 0;
}

// ---- 2. one sweep: one wave per robot ----
// Robot r takes the largest k in [1, walked] whose cell conflicts with no blocker (dx^2 + dy^2 < sep^2), else 0.  Its blockers are the
// cells c_j[k_prev[j]] of the taking-part robots j < r and the start cells of the taking-part robots j > r: it reads the buffer of the
// sweep before and writes only its own word of the other buffer, so a sweep is a Jacobi step whatever the order of the workgroups.
// Candidates: lane l of chunk c holds k = walked - 64 c - l and loads its cell, 8 bytes, next to its neighbours' (descending addresses).
// Blockers: 64 at a time, one per lane; one farther than reach + sep (Chebyshev) from the robot's start is dropped at once -- every
// candidate lies within `reach` of the start, so such a blocker is at least sep + 1 > sep cells from each along one axis: the cull is
// exact.  The survivors of the ballot are broadcast one by one and every lane tests its own candidate.  The first chunk with a feasible
// lane decides, and its lowest lane holds the largest k; k = 0 always serves, and what its lane found is `clear`.
// Bounds: walked and every k_prev are clamped to [0, max_steps], so every cell index lies in its row whatever the workspace holds; the
// chunk loop runs walked / 64 + 1 <= 64 times, the blocker loop ceil(n / 64) times, the broadcast loop at most 64 times.  The squares
// are taken in 64 bits (window_apart_dev.h: cells_conflict, with the cull cell_near and the clamps walked_of, k_in_row).
__global__ __launch_bounds__(WG_THREADS) void window_apart_sweep_kernel(int n_queries, int reach, int max_steps, int sep, ApartWork w,
                                                                        const int* __restrict__ k_prev, int* __restrict__ k_next) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int4 m = w.meta[r];
  if (m.z != WALK_OK) return;                              // takes no part: one decision per wave
  const size_t stride = apart_row(max_steps);
  const int2* row = w.paths + (size_t)r * stride;
  const int walked = walked_of(w, r, max_steps);
  const int2 s = row[0];
  const long long far = (long long)reach + sep, sep2 = (long long)sep * sep;
  int k_new = 0, clear = 0;
  for (int c = 0; c <= walked / WG_THREADS; ++c) {
    const int k = walked - c * WG_THREADS - lane;
    const int2 cand = row[max(k, 0)];
    bool conflict = false;
    for (int base = 0; base < n_queries; base += WG_THREADS) {
      const int j = base + lane;
      bool blocks = j < n_queries && j != r && w.meta[min(j, n_queries - 1)].z == WALK_OK;
      int2 b = make_int2(0, 0);
      if (blocks) {
        b = w.paths[(size_t)j * stride + (j < r ? k_in_row(k_prev, j, max_steps) : 0)];
        blocks = cell_near(b, s, far);
      }
      unsigned long long live = __ballot(blocks);
      while (live) {
        const int src = __ffsll((long long)live) - 1;
        live &= live - 1;
        conflict |= cells_conflict(make_int2(__shfl(b.x, src), __shfl(b.y, src)), cand, sep2);
      }
    }
    const unsigned long long serves = __ballot(k == 0 || (k > 0 && !conflict));
    if (serves) {
      const int first = __ffsll((long long)serves) - 1;
      k_new = walked - c * WG_THREADS - first;
      clear = __shfl((int)!conflict, first);
      break;
    }
  }
  if (lane == 0) {
    k_next[r] = k_new;
    w.flag[r] = (k_new != k_in_row(k_prev, r, max_steps) ? WA_MOVED : 0) | (clear ? WA_CLEAR : 0);
  }
}

// ---- 3. the outputs: one wave per robot, lane j = sample j ----
// Every word of cells, origins, summary, extra (window_apart_dev.h: emitted_k and what follows it) and (if given) samples of the robot, from the state
// in k_cur; a robot that takes no part gets window_goals' words, extra (steps, 0) and zero samples.  63 * k + 31 stays below 2^18.  The
// first workgroup also sums the moved flags of all robots (wave_dev.h: wave_sum, a fixed order) into changed[0].  With to_first, the
// robot's k goes back to buffer 0, the robot's own word: the next call finds the state there.
__global__ __launch_bounds__(WG_THREADS) void window_apart_emit_kernel(int n_queries, int max_steps, ApartWork w, const int* __restrict__ k_cur,
                                                                       int to_first, int2* __restrict__ cells, int2* __restrict__ origins,
                                                                       int4* __restrict__ summary, int2* __restrict__ extra,
                                                                       int2* __restrict__ samples, int* __restrict__ changed) {
  const int r = blockIdx.x, j = threadIdx.x;
  const int4 m = w.meta[r];
  const bool ok = m.z == WALK_OK;
  const int2* row = w.paths + (size_t)r * apart_row(max_steps);
  const int k = emitted_k(m, ok, k_cur, r, max_steps);
  if (samples) samples[(size_t)r * WG_THREADS + j] = ok ? row[(j * k + 31) / 63] : make_int2(0, 0);
  if (j == 0) {
    cells[r] = emitted_cell(row, k);
    origins[r] = w.origin[r];
    summary[r] = ok ? summary_at(m, k, max_steps) : make_int4(m.x, m.y, m.z, 0);
    extra[r] = emitted_extra(w, r, m, ok);
    if (to_first) w.k[0][r] = k_cur[r];
  }
  if (r == 0) {
    int moved = 0;
    for (int base = 0; base < n_queries; base += WG_THREADS) moved += base + j < n_queries ? (w.flag[base + j] & WA_MOVED) : 0;
    moved = wave_sum(moved);
    if (j == 0) changed[0] = moved;
  }
}

}  // namespace mmd

using namespace mmd;

extern "C" {

size_t mmd_grid_window_apart_work_bytes(int n_queries, int max_steps) {
  if (n_queries < 0 || n_queries > INT_MAX - WG_THREADS || max_steps < 1 || max_steps > WA_MAX_STEPS) return 0;
  return apart_work_bytes(n_queries, max_steps);
}

int mmd_grid_window_goals_apart(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev, const int32_t* field_dev,
                                const int32_t* goals_dev, int n_queries, int reach, int max_steps, int window, int sep, int restart,
                                int n_sweeps, void* work_dev, size_t work_bytes, int32_t* cells_dev, int32_t* origins_dev,
                                int32_t* summary_dev, int32_t* extra_dev, int32_t* samples_dev, int32_t* changed_dev, void* stream) {
  const char* name = "mmd_grid_window_goals_apart";
  if (const int refused = window_goals_ranges(name, nx, ny, n_fields, n_queries, reach, max_steps, WA_MAX_STEPS, window)) return refused;
  MMD_REQUIRE(sep >= 1 && sep <= WA_MAX_SEP, "mmd_grid_window_goals_apart: sep = %d cells (1 to %d)", sep, WA_MAX_SEP);
  MMD_REQUIRE(n_sweeps >= 0, "mmd_grid_window_goals_apart: n_sweeps = %d (>= 0)", n_sweeps);
  if (n_queries == 0) return 0;
  if (const int refused = window_goals_inputs(name, dist_dev, goals_dev, n_fields, starts_dev, field_dev)) return refused;
  MMD_REQUIRE(work_dev && (uintptr_t)work_dev % 16 == 0, "mmd_grid_window_goals_apart: NULL workspace, or one not aligned to 16 bytes");
  MMD_REQUIRE(work_bytes >= apart_work_bytes(n_queries, max_steps), "mmd_grid_window_goals_apart: workspace of %zu bytes, %zu needed",
              work_bytes, apart_work_bytes(n_queries, max_steps));
  if (const int refused = window_goals_outputs(name, cells_dev, origins_dev, summary_dev)) return refused;
  MMD_REQUIRE(extra_dev, "mmd_grid_window_goals_apart: NULL extra");
  MMD_REQUIRE(changed_dev, "mmd_grid_window_goals_apart: NULL changed");
  const ApartWork w = apart_work(work_dev, n_queries, max_steps);
  hipStream_t st = (hipStream_t)stream;
  if (restart) {
    hipLaunchKernelGGL(window_apart_paths_kernel, dim3((n_queries + WG_THREADS - 1) / WG_THREADS), dim3(WG_THREADS), 0, st,
                       (const int*)dist_dev, nx, ny, n_fields, (const int2*)starts_dev, (const int*)field_dev, (const int2*)goals_dev,
                       n_queries, reach, max_steps, window, w);
    MMD_HIP_CHECK(hipGetLastError());
  }
  int cur = 0;                                             // the buffer that holds the state
  for (int s = 0; s < n_sweeps; ++s, cur ^= 1) {
    hipLaunchKernelGGL(window_apart_sweep_kernel, dim3(n_queries), dim3(WG_THREADS), 0, st, n_queries, reach, max_steps, sep, w,
                       (const int*)w.k[cur], w.k[cur ^ 1]);
    MMD_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(window_apart_emit_kernel, dim3(n_queries), dim3(WG_THREADS), 0, st, n_queries, max_steps, w, (const int*)w.k[cur], cur,
                     (int2*)cells_dev, (int2*)origins_dev, (int4*)summary_dev, (int2*)extra_dev, (int2*)samples_dev, (int*)changed_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
