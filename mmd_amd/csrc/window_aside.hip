// World fleets: standing robots step aside for the robots they hold back (include/mmd_amd.h: mmd_grid_window_goals_aside).  The definition
// is the numpy function subgoals_aside of mmd_amd/fleet_subgoals.py; safety and containment are argued there.  The call reads the workspace of
// mmd_grid_window_goals_apart at its fixed point (phase 1: meta, paths, origin, k[0], flag) and never writes it.  Every value here is an
// exact integer.  Plain loads and vector stores, LDS in the side step only; no atomics, no scratch, and nothing inside a launch waits on
// another workgroup.  Every index read from device memory is clamped before it is used.
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

constexpr int AS_MAX_REACH = MMD_WINDOW_ASIDE_MAX_REACH, AS_MAX_STEPS = MMD_WINDOW_ASIDE_MAX_STEPS;
constexpr int AS_HELD = 1, AS_YIELDS = 2, AS_MOVED = 4, AS_RELEASED = 8;       // the role bits of the output
constexpr int AS_STANDS = 16, AS_TAKES = 32;                                   // the workspace's own: k == 0; the query takes part
constexpr int AS_THREADS = 256, AS_PATCH_SIDE = 2 * AS_MAX_REACH + 3;         // the largest box, with a border of one cell
constexpr unsigned short AS_OPEN = 0x7ffe, AS_WALL = 0x7fff, AS_BLOCKED = 0x8000;   // a patch word: a level 0 .. 4095, or one of these
static_assert(WG_THREADS == 64 && AS_MAX_STEPS < AS_OPEN && AS_PATCH_SIDE * AS_PATCH_SIDE < (1 << 15) && MMD_OCCUPANCY_MAX_SIDE <= (1 << 15) &&
                  AS_PATCH_SIDE * AS_PATCH_SIDE <= 128 * AS_THREADS,
              "a level fits a patch word, a patch index 15 bits, a cell two halves of a word, a thread's cells two 64-bit masks");

// The workspace of a call on n queries (all parts 8-byte aligned from the 16-byte aligned base):
//   side     int2 [2][n]   (l, ix << 16 | iy): the side step of a yielder, l = 0: it stays; the two buffers of the sweeps
//   k        int  [2][n]   the k of every robot: phase 1's, and k' of a released robot; the two buffers of the sweeps
//   roles    int  [n]      AS_HELD | AS_YIELDS | AS_STANDS | AS_TAKES, from phase 1 (a restart writes them)
//   released int  [n]      what the last sweep found
//   moved    int  [2][n]   1: the robot's side word / its k changed in the last sweep (after a restart: the query takes part / 0)
// A call begins and ends with the state in buffer 0.
struct AsideWork {
  int2* side[2];
  int* k[2];
  int* roles;
  int* released;
  int* moved[2];
};

static size_t aside_work_bytes(int n) { return (size_t)n * (2 * sizeof(int2) + 6 * sizeof(int)); }

static AsideWork aside_work(void* base, int n) {
  AsideWork a;
  a.side[0] = (int2*)base;
  a.side[1] = a.side[0] + n;
  a.k[0] = (int*)(a.side[1] + n);
  a.k[1] = a.k[0] + n;
  a.roles = a.k[1] + n;
  a.released = a.roles + n;
  a.moved[0] = a.released + n;
  a.moved[1] = a.moved[0] + n;
  return a;
}

__device__ __forceinline__ int2 side_cell(int word) { return make_int2((word >> 16) & 0xffff, word & 0xffff); }

// phase 1's words of query q, clamped (window_apart_dev.h: walked_of, k_of): the cells its walk covered, its k, does it take part
__device__ __forceinline__ int k1_of(const ApartWork& w, int q, int max_steps) { return k_of(w.k[0], w, q, max_steps); }
__device__ __forceinline__ int base_roles(const ApartWork& w, int q, int max_steps, int n_fields) {
  if (n_fields < 1 || w.meta[q].z != WALK_OK) return 0;
  const bool stands = k1_of(w, q, max_steps) == 0;
  return AS_TAKES | (stands ? AS_STANDS : 0) | (stands && walked_of(w, q, max_steps) >= 1 ? AS_HELD : 0);
}

// is r in clears(j)?  roles_r and roles_j are their role words, s_j is j's start; r's first step is loaded only if r is held (it has one)
__device__ __forceinline__ bool clears(const ApartWork& w, size_t stride, int r, int roles_r, int j, int roles_j, int2 s_j, long long sep2) {
  if (!(roles_r & AS_HELD) || r == j || !(roles_j & AS_STANDS) || ((roles_j & AS_HELD) && r > j)) return false;
  return cells_conflict(s_j, w.paths[(size_t)r * stride + 1], sep2);
}

// ---- 1. the roles: one wave per robot j, lanes over r in chunks of 64 ----
// HELD and STANDS come from phase 1's words; j YIELDS iff clears(j) is not empty.  The state starts as phase 1 left it: nobody moved aside,
// every k is phase 1's, nobody is released; `moved` says "changed" for a query that takes part, for nothing is proved before a sweep.
__global__ __launch_bounds__(WG_THREADS) void window_aside_roles_kernel(int n_queries, int n_fields, int max_steps, int sep, ApartWork w,
                                                                        AsideWork a) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const size_t stride = apart_row(max_steps);
  const int bj = base_roles(w, j, max_steps, n_fields);
  const long long sep2 = (long long)sep * sep;
  bool yields = false;
  if (bj & AS_STANDS) {
    const int2 s = w.paths[(size_t)j * stride];
    for (int base = 0; base < n_queries && !yields; base += WG_THREADS) {
      const int r = base + lane;
      const bool hit = r < n_queries && clears(w, stride, r, base_roles(w, min(r, n_queries - 1), max_steps, n_fields), j, bj, s, sep2);
      yields = __ballot(hit) != 0;
    }
  }
  if (lane == 0) {
    a.roles[j] = bj | (yields ? AS_YIELDS : 0);
    a.side[0][j] = a.side[1][j] = make_int2(0, 0);
    a.k[0][j] = a.k[1][j] = bj ? k1_of(w, j, max_steps) : 0;
    a.released[j] = 0;
    a.moved[0][j] = bj ? 1 : 0;
    a.moved[1][j] = 0;
  }
}

// ---- 2. one sweep, the side steps: one workgroup of 256 threads per robot j ----
// A robot that does not yield writes "stays" and leaves on one uniform test.  A yielder fills the patch of (2 aside_reach + 3)^2 uint16
// words round its start -- the box, and a border of WALL words, so that a cell's four neighbours need no test -- with the BFS level of
// every cell (level-synchronous, one barrier a level, thread t owning the cells t, t + 256, .., at most 66 of them, and holding the set
// of its cells that are still OPEN in two 64-bit masks: a level costs a thread four independent LDS reads per cell it has not reached
// yet; a thread writes only its own cells, and a neighbour's word read while it is written holds OPEN or this level, never level - 1).
// Then the blockers, 256 robots at a time: one cell per robot -- the side cell of a yielder i < j that moved in the sweep before, the
// start of any other yielder, phase 1's chosen cell of the rest -- and, for every r in clears(j), the cells of r's walk, 256 at a time
// (which r of the chunk: one ballot per wave, four LDS words that every thread takes into registers).
// A blocker farther than aside_reach + sep (Chebyshev) from the start is dropped: every candidate lies within aside_reach of the start, so
// such a blocker is at least sep + 1 cells from each along one axis; the cull is exact.  The survivors are packed into LDS in thread
// order and every thread marks its own candidates that conflict with one.  At last every thread finds the least key
// (l, own field value, patch index in (ix, iy) order) over its unmarked candidates, the wave butterfly and four LDS words give the block's.
// Bounds: the start is clamped into the grid, so the patch's cells are tested against the grid with small integers; a patch index is
// < 129^2, and a cell in a mask is a cell of the box, whose four neighbours lie in the patch; list entries are written at a prefix < 256;
// walked and every k are clamped (walked_of, k1_of); the field index is clamped.
__global__ __launch_bounds__(AS_THREADS) void window_aside_side_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                       const int* __restrict__ field, int n_queries, int max_steps, int sep,
                                                                       int aside_reach, int aside_steps, ApartWork w, AsideWork a,
                                                                       const int2* __restrict__ side_prev, int2* __restrict__ side_next,
                                                                       int* __restrict__ moved) {
  __shared__ unsigned short patch[AS_PATCH_SIDE * AS_PATCH_SIDE + 1];
  __shared__ int2 list[AS_THREADS];
  __shared__ unsigned long long in_clears[AS_THREADS / 64];    // per wave: the ballot of "robot base + 64 wave + lane is in clears(j)"
  __shared__ int lds4[4];
  __shared__ unsigned long long best[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int rj = a.roles[j];
  if (!(rj & AS_YIELDS) || n_fields < 1) {                   // one decision per workgroup
    if (tid == 0) {
      const int2 before = side_prev[j];
      side_next[j] = make_int2(0, 0);
      moved[j] = before.x != 0 || before.y != 0;
    }
    return;
  }
  const size_t stride = apart_row(max_steps);
  int2 s = w.paths[(size_t)j * stride];
  s = make_int2(min(max(s.x, 0), nx - 1), min(max(s.y, 0), ny - 1));
  const int side = 2 * aside_reach + 3, cells = side * side, ox = s.x - aside_reach - 1, oy = s.y - aside_reach - 1;    // with the border
  const int* own = dist_all + (size_t)min(max(field[j], 0), n_fields - 1) * nx * ny;
  const int step_x = AS_THREADS / side, step_y = AS_THREADS % side, first_x = tid / side, first_y = tid % side;
  const long long sep2 = (long long)sep * sep, far = (long long)aside_reach + sep;

  // the patch: which cells the BFS may enter; this thread's open cells, bit i = its cell tid + 256 i
  unsigned long long open_lo = 0, open_hi = 0;
  for (int c = tid, i = 0, px = first_x, py = first_y; c < cells; c += AS_THREADS, ++i) {
    const int ix = ox + px, iy = oy + py;
    const bool start = px == aside_reach + 1 && py == aside_reach + 1;
    const bool open = px >= 1 && px <= side - 2 && py >= 1 && py <= side - 2 && ix >= 0 && ix < nx && iy >= 0 && iy < ny && !start &&
                      own[(size_t)ix * ny + iy] != GRID_UNREACHED;
    patch[c] = start ? 0 : open ? AS_OPEN : AS_WALL;
    if (open) {
      if (i < 64) open_lo |= 1ull << i;
      else open_hi |= 1ull << (i - 64);
    }
    px += step_x; py += step_y;
    if (py >= side) { py -= side; ++px; }
  }
  __syncthreads();
  for (int level = 1; level <= aside_steps; ++level) {
    const unsigned short from = (unsigned short)(level - 1);
    int any = 0;
    unsigned long long m = open_lo;
    while (m) {
      const int bit = __ffsll((long long)m) - 1, c = tid + AS_THREADS * bit;
      m &= m - 1;
      if ((patch[c - side] == from) | (patch[c + side] == from) | (patch[c - 1] == from) | (patch[c + 1] == from)) {
        patch[c] = (unsigned short)level;
        open_lo &= ~(1ull << bit);
        any = 1;
      }
    }
    m = open_hi;
    while (m) {
      const int bit = __ffsll((long long)m) - 1, c = tid + AS_THREADS * (bit + 64);
      m &= m - 1;
      if ((patch[c - side] == from) | (patch[c + side] == from) | (patch[c - 1] == from) | (patch[c + 1] == from)) {
        patch[c] = (unsigned short)level;
        open_hi &= ~(1ull << bit);
        any = 1;
      }
    }
    if (!__syncthreads_or(any)) break;                       // (a barrier: the level is complete) an empty level ends the search
  }

  // marks this thread's candidates that conflict with one of list[0 .. total)
  auto mark = [&](int total) {
    if (total == 0) return;
    for (int c = tid, px = first_x, py = first_y; c < cells; c += AS_THREADS) {
      const unsigned short v = patch[c];
      if (v >= 1 && v <= aside_steps) {
        const int2 cell = make_int2(ox + px, oy + py);
        for (int e = 0; e < total; ++e)
          if (cells_conflict(cell, list[e], sep2)) {
            patch[c] = v | AS_BLOCKED;
            break;
          }
      }
      px += step_x; py += step_y;
      if (py >= side) { py -= side; ++px; }
    }
  };

  for (int base = 0; base < n_queries; base += AS_THREADS) {
    const int i = base + tid;
    int2 b = make_int2(0, 0);
    bool keep = false, cl = false;
    if (i < n_queries && i != j) {
      const int ri = a.roles[i];
      if (ri & AS_TAKES) {
        if (ri & AS_YIELDS) {
          const int2 sp = side_prev[i];
          b = i < j && sp.x > 0 ? side_cell(sp.y) : w.paths[(size_t)i * stride];
        } else {
          b = w.paths[(size_t)i * stride + k1_of(w, i, max_steps)];
        }
        keep = cell_near(b, s, far);
        cl = clears(w, stride, i, ri, j, rj, s, sep2);
      }
    }
    const unsigned long long wave_clears = __ballot(cl);
    if ((tid & 63) == 0) in_clears[tid >> 6] = wave_clears;
    int prefix;
    int total = block_prefix(keep, lds4, prefix);            // (two barriers: in_clears is written for all)
    if (keep) list[prefix] = b;
    // every thread takes the four ballots into registers BEFORE the next barrier: the next pass of this loop writes in_clears again only
    // behind that barrier, so no wave can overwrite a word that another still has to read
    unsigned long long cleared[AS_THREADS / 64];
#pragma unroll
    for (int wv = 0; wv < AS_THREADS / 64; ++wv) cleared[wv] = in_clears[wv];
    __syncthreads();
    mark(total);
    __syncthreads();
#pragma unroll
    for (int wv = 0; wv < AS_THREADS / 64; ++wv) {           // class (d): the same words on every thread, so the barriers below are uniform
      unsigned long long m = cleared[wv];
      while (m) {
        const int r = min(base + 64 * wv + __ffsll((long long)m) - 1, n_queries - 1), walked = walked_of(w, r, max_steps);
        m &= m - 1;
        for (int cb = 0; cb <= walked; cb += AS_THREADS) {
          const int idx = cb + tid;
          keep = idx <= walked;
          if (keep) {
            b = w.paths[(size_t)r * stride + idx];
            keep = cell_near(b, s, far);
          }
          total = block_prefix(keep, lds4, prefix);
          if (keep) list[prefix] = b;
          __syncthreads();
          mark(total);
          __syncthreads();
        }
      }
    }
  }

  // the choice: the least (l, own field value, patch index)
  unsigned long long key = ~0ull;
  for (int c = tid, px = first_x, py = first_y; c < cells; c += AS_THREADS) {
    const unsigned short v = patch[c];
    if (v >= 1 && v <= aside_steps) {
      const int d = min(max(own[(size_t)(ox + px) * ny + (oy + py)], 0), (1 << 22) - 1);
      key = min(key, (unsigned long long)v << 37 | (unsigned long long)d << 15 | (unsigned long long)c);
    }
    px += step_x; py += step_y;
    if (py >= side) { py -= side; ++px; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) key = min(key, (unsigned long long)__shfl_xor((long long)key, m));
  if ((tid & 63) == 0) best[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    key = min(min(best[0], best[1]), min(best[2], best[3]));
    int2 next = make_int2(0, 0);
    if (key != ~0ull) {
      const int c = (int)(key & 0x7fff);
      next = make_int2((int)(key >> 37), (ox + c / side) << 16 | (oy + c % side));
    }
    const int2 before = side_prev[j];
    side_next[j] = next;
    moved[j] = before.x != next.x || before.y != next.y;
  }
}

// ---- 3. one sweep, the release: one wave per robot r ----
// r is released iff it is held, did not move aside, and some j that moved aside has r in clears(j) (side_cur: what this sweep's side
// kernel wrote).  A released robot applies window_apart_sweep_kernel's rule to its walk; its blockers are the others' final cells: a side
// cell, else the walk's cell at the k of the sweep before for i < r and at phase 1's k for i > r (a released robot of higher index still
// stands on its start).  Everyone else keeps phase 1's k.  Bounds as in the sweep kernel.
__global__ __launch_bounds__(WG_THREADS) void window_aside_release_kernel(int n_queries, int reach, int max_steps, int sep, ApartWork w,
                                                                          AsideWork a, const int2* __restrict__ side_cur,
                                                                          const int* __restrict__ k_prev, int* __restrict__ k_next,
                                                                          int* __restrict__ moved) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int rr = a.roles[r];
  const size_t stride = apart_row(max_steps);
  const long long far = (long long)reach + sep, sep2 = (long long)sep * sep;
  const int walked = rr ? walked_of(w, r, max_steps) : 0;
  int k_new = rr ? k1_of(w, r, max_steps) : 0;
  bool released = false;
  if ((rr & AS_HELD) && side_cur[r].x <= 0) {
    for (int base = 0; base < n_queries && !released; base += WG_THREADS) {
      const int j = base + lane;
      bool hit = false;
      if (j < n_queries) {
        const int rj = a.roles[j];
        if ((rj & AS_YIELDS) && side_cur[j].x > 0) hit = clears(w, stride, r, rr, j, rj, w.paths[(size_t)j * stride], sep2);
      }
      released = __ballot(hit) != 0;
    }
  }
  if (released) {
    const int2* row = w.paths + (size_t)r * stride;
    const int2 s = row[0];
    k_new = 0;
    for (int c = 0; c <= walked / WG_THREADS; ++c) {
      const int k = walked - c * WG_THREADS - lane;
      const int2 cand = row[max(k, 0)];
      bool conflict = false;
      for (int base = 0; base < n_queries; base += WG_THREADS) {
        const int i = base + lane;
        bool blocks = i < n_queries && i != r && (a.roles[min(i, n_queries - 1)] & AS_TAKES);
        int2 b = make_int2(0, 0);
        if (blocks) {
          const int2 sc = side_cur[i];
          const int ki = i < r ? k_of(k_prev, w, i, max_steps) : k1_of(w, i, max_steps);
          b = sc.x > 0 ? side_cell(sc.y) : w.paths[(size_t)i * stride + ki];
          blocks = cell_near(b, s, far);
        }
        unsigned long long live = __ballot(blocks);
        while (live) {
          const int src = __ffsll((long long)live) - 1;
          live &= live - 1;
          conflict |= cells_conflict(make_int2(__shfl(b.x, src), __shfl(b.y, src)), cand, sep2);
        }
      }
      const unsigned long long serves = __ballot(k > 0 && !conflict);
      if (serves) {
        k_new = walked - c * WG_THREADS - (__ffsll((long long)serves) - 1);
        break;
      }
    }
  }
  if (lane == 0) {
    k_next[r] = k_new;
    a.released[r] = released;
    moved[r] = k_new != k_prev[r];
  }
}

// ---- 4. the outputs: one lane per query ----
// Every word of cells, origins, summary, extra and aside from the state in (side_cur, k_cur); a query that takes no part gets
// window_goals' words, extra (steps, 0) and aside (0, 0).  The first workgroup also sums both `moved` flags of all robots into
// changed[0].  With to_first, the state goes back to buffer 0, every robot its own words.
__global__ __launch_bounds__(WG_THREADS) void window_aside_emit_kernel(const int* __restrict__ dist_all, int nx, int ny, int n_fields,
                                                                       const int* __restrict__ field, int n_queries, int max_steps,
                                                                       ApartWork w, AsideWork a, const int2* __restrict__ side_cur,
                                                                       const int* __restrict__ k_cur, int to_first, int2* __restrict__ cells,
                                                                       int2* __restrict__ origins, int4* __restrict__ summary,
                                                                       int2* __restrict__ extra, int2* __restrict__ aside,
                                                                       int* __restrict__ changed) {
  const int q = blockIdx.x * WG_THREADS + threadIdx.x;
  if (q < n_queries) {
    const int4 m = w.meta[q];
    const int rr = a.roles[q];
    const bool ok = (rr & AS_TAKES) != 0;
    const int2* row = w.paths + (size_t)q * apart_row(max_steps);
    const int2 sc = side_cur[q];
    const int kk = k_cur[q];
    origins[q] = w.origin[q];
    extra[q] = emitted_extra(w, q, m, ok);
    if (ok && n_fields >= 1 && (rr & AS_YIELDS) && sc.x > 0) {
      int2 cell = side_cell(sc.y);
      cell = make_int2(min(cell.x, nx - 1), min(cell.y, ny - 1));
      const int d = dist_all[((size_t)min(max(field[q], 0), n_fields - 1) * nx + cell.x) * ny + cell.y];
      cells[q] = cell;
      summary[q] = make_int4(sc.x, d, WALK_OK, d == 0);
      aside[q] = make_int2((rr & (AS_HELD | AS_YIELDS)) | AS_MOVED, sc.x);
    } else {
      const int k = emitted_k(m, ok, k_cur, q, max_steps);
      cells[q] = emitted_cell(row, k);
      summary[q] = ok ? summary_at(m, k, max_steps) : make_int4(m.x, m.y, m.z, 0);
      aside[q] = make_int2(ok ? (rr & (AS_HELD | AS_YIELDS)) | (a.released[q] ? AS_RELEASED : 0) : 0, 0);
    }
    if (to_first) {
      a.side[0][q] = sc;
      a.k[0][q] = kk;
    }
  }
  if (blockIdx.x == 0) {
    const int lane = threadIdx.x;
    int moved = 0;
    for (int base = 0; base < n_queries; base += WG_THREADS)
      moved += base + lane < n_queries ? (a.moved[0][base + lane] != 0) + (a.moved[1][base + lane] != 0) : 0;
    moved = wave_sum(moved);
    if (lane == 0) changed[0] = moved;
  }
}

}  // namespace mmd

using namespace mmd;

extern "C" {

size_t mmd_grid_window_aside_work_bytes(int n_queries) {
  if (n_queries < 0 || n_queries > INT_MAX - WG_THREADS) return 0;
  return aside_work_bytes(n_queries);
}

int mmd_grid_window_goals_aside(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* field_dev, int n_queries, int reach,
                                int max_steps, int window, int sep, int aside_reach, int aside_steps, int restart, int n_sweeps,
                                const void* apart_work_dev, size_t apart_work_bytes_given, void* work_dev, size_t work_bytes,
                                int32_t* cells_dev, int32_t* origins_dev, int32_t* summary_dev, int32_t* extra_dev, int32_t* aside_dev,
                                int32_t* changed_dev, void* stream) {
  const char* name = "mmd_grid_window_goals_aside";
  if (const int refused = window_goals_ranges(name, nx, ny, n_fields, n_queries, reach, max_steps, WA_MAX_STEPS, window)) return refused;
  MMD_REQUIRE(sep >= 1 && sep <= WA_MAX_SEP, "mmd_grid_window_goals_aside: sep = %d cells (1 to %d)", sep, WA_MAX_SEP);
  MMD_REQUIRE(aside_reach >= 1 && aside_reach <= reach && aside_reach <= AS_MAX_REACH,
              "mmd_grid_window_goals_aside: aside_reach = %d cells (1 to min(reach, %d) = %d)", aside_reach, AS_MAX_REACH,
              reach < AS_MAX_REACH ? reach : AS_MAX_REACH);
  MMD_REQUIRE(aside_steps >= 1 && aside_steps <= AS_MAX_STEPS, "mmd_grid_window_goals_aside: aside_steps = %d (1 to %d)", aside_steps,
              AS_MAX_STEPS);
  MMD_REQUIRE(n_sweeps >= 0, "mmd_grid_window_goals_aside: n_sweeps = %d (>= 0)", n_sweeps);
  if (n_queries == 0) return 0;
  MMD_REQUIRE(dist_dev || n_fields == 0, "mmd_grid_window_goals_aside: NULL dist with n_fields = %d", n_fields);
  MMD_REQUIRE(field_dev, "mmd_grid_window_goals_aside: NULL field indices");
  MMD_REQUIRE(apart_work_dev && (uintptr_t)apart_work_dev % 16 == 0,
              "mmd_grid_window_goals_aside: NULL apart workspace, or one not aligned to 16 bytes");
  MMD_REQUIRE(apart_work_bytes_given >= apart_work_bytes(n_queries, max_steps),
              "mmd_grid_window_goals_aside: apart workspace of %zu bytes, %zu needed", apart_work_bytes_given,
              apart_work_bytes(n_queries, max_steps));
  MMD_REQUIRE(work_dev && (uintptr_t)work_dev % 16 == 0, "mmd_grid_window_goals_aside: NULL workspace, or one not aligned to 16 bytes");
  MMD_REQUIRE(work_bytes >= aside_work_bytes(n_queries), "mmd_grid_window_goals_aside: workspace of %zu bytes, %zu needed", work_bytes,
              aside_work_bytes(n_queries));
  if (const int refused = window_goals_outputs(name, cells_dev, origins_dev, summary_dev)) return refused;
  MMD_REQUIRE(extra_dev, "mmd_grid_window_goals_aside: NULL extra");
  MMD_REQUIRE(aside_dev, "mmd_grid_window_goals_aside: NULL aside");
  MMD_REQUIRE(changed_dev, "mmd_grid_window_goals_aside: NULL changed");
  const ApartWork w = apart_work(const_cast<void*>(apart_work_dev), n_queries, max_steps);        // read only
  const AsideWork a = aside_work(work_dev, n_queries);
  hipStream_t st = (hipStream_t)stream;
  if (restart) {
    hipLaunchKernelGGL(window_aside_roles_kernel, dim3(n_queries), dim3(WG_THREADS), 0, st, n_queries, n_fields, max_steps, sep, w, a);
    MMD_HIP_CHECK(hipGetLastError());
  }
  int cur = 0;                                             // the buffers that hold the state
  for (int s = 0; s < n_sweeps; ++s, cur ^= 1) {
    hipLaunchKernelGGL(window_aside_side_kernel, dim3(n_queries), dim3(AS_THREADS), 0, st, (const int*)dist_dev, nx, ny, n_fields,
                       (const int*)field_dev, n_queries, max_steps, sep, aside_reach, aside_steps, w, a, (const int2*)a.side[cur],
                       a.side[cur ^ 1], a.moved[0]);
    MMD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(window_aside_release_kernel, dim3(n_queries), dim3(WG_THREADS), 0, st, n_queries, reach, max_steps, sep, w, a,
                       (const int2*)a.side[cur ^ 1], (const int*)a.k[cur], a.k[cur ^ 1], a.moved[1]);
    MMD_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(window_aside_emit_kernel, dim3((n_queries + WG_THREADS - 1) / WG_THREADS), dim3(WG_THREADS), 0, st,
                     (const int*)dist_dev, nx, ny, n_fields, (const int*)field_dev, n_queries, max_steps, w, a, (const int2*)a.side[cur],
                     (const int*)a.k[cur], cur, (int2*)cells_dev, (int2*)origins_dev, (int4*)summary_dev, (int2*)extra_dev,
                     (int2*)aside_dev, (int*)changed_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
