// The builders of the constraint tables the guided step reads (include/mmd_amd.h): the host pack of the time-bucketed ELL table [slot][t]
// (mmd_pack_constraints), whose rules every device builder follows; the all-pairs block of the gathered best paths, a table of its own or
// the soft block of a round table; the cell table (mmd_cons_bins) and its walkers' checks; the round table of a round that repairs its
// conflicts; the framed table of a world larger than one tile.  What they share is in cons_table_dev.h.  mmd_path_constraints stays with
// the search layer (multi_agent.hip); the walkers are the guided step (guide.hip) and the collision kernels (multi_agent.hip).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include "../../include/mmd_amd.h"
#include "bins_dev.h"             // bin_cell / own_cell_list
#include "collision_dev.h"        // rr_hit: the pinned fp32 form of the collision decision (sets fp contract(off))
#include "common.h"
#include "cons_table_dev.h"
#include "wave_dev.h"             // wave_sum / wave_max

namespace mmd {

// The all-pairs block of every local robot (cbs.py:468-508): slot S_h + j of local robot i's S = S_h + n_all - 1 slots holds the j-th other
// robot's point, active at t >= 1 (column 0 keeps the point with R = -1).  S_h = 0 with the offset arrays: mmd_soft_constraints_from_paths'
// table, one group per robot.  S_h > 0 without them: the soft block behind a round table's hard block (its offsets are round_init_kernel's).
__global__ void all_pairs_kernel(const float2* __restrict__ paths, int n_all, int robot0, int n_local, int S_h, float radius, float weight,
                                 float4* __restrict__ ell, int* __restrict__ grp_slot_off, float* __restrict__ grp_weight,
                                 int* __restrict__ robot_grp_off) {
  const int slots = n_all - 1, S = S_h + slots;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = tid; idx < (size_t)n_local * slots * H; idx += step) {   // idx = (i slots + j) H + t
    const int t = idx % H;
    const unsigned row = (unsigned)(idx / H);                               // (the entry points refuse a table of 2^32 rows or more)
    const int i = row / (unsigned)slots, j = row - (unsigned)i * slots;
    const float2 p = paths[(size_t)all_pairs_other(j, robot0 + i) * H + t];
    ell[idx + (size_t)(i + 1) * S_h * H] = slot_word(p.x, p.y, t >= 1 ? radius : -1.f);   // behind the hard blocks of robots 0 .. i
  }
  if (!grp_slot_off) return;
  for (int i = (int)tid; i < n_local; i += (int)step) one_group_per_robot(i, n_local, S, weight, grp_slot_off, grp_weight, robot_grp_off);
}

// The cell table of mmd_cons_bins from the best paths: ONE workgroup per time step t, no atomics, so a list is in ascending robot id by
// construction.  The step's n_all points and cell indices (ix << 16 | iy) are staged in LDS; thread i owns the cells [i cpt, (i + 1) cpt)
// (cell = ix * ny + iy) and walks the robots 0 .. n_all - 1 in order twice: to count its cells' entries and, after the block's prefix
// sum, to write them.  A robot is in the lists of the (at most nine) cells within one index of its own, so a time step's lists fit its
// segment of 9 n_all entries.  Time steps below first_step get empty lists: a constraint table starts at 1 (time step 0 has no
// constraint, all_pairs_kernel: t in [1, H - 1]), a collision table (mmd_bin_paths) at 0.
constexpr int BIN_THREADS = 256;
__global__ __launch_bounds__(BIN_THREADS) void bin_cons_kernel(const float2* __restrict__ paths, int n_all, float lo0, float lo1, float inv0,
                                                               float inv1, int nx, int ny, int first_step, int* __restrict__ cell_off,
                                                               float4* __restrict__ entries) {
  extern __shared__ __attribute__((aligned(16))) float2 lds_pts[];       // [n_all] points, [n_all] cells, [BIN_THREADS] scan
  int* const lds_cell = reinterpret_cast<int*>(lds_pts + n_all);
  int* const scan = lds_cell + n_all;
  const int t = blockIdx.x, tid = threadIdx.x, ncell = nx * ny;
  int* const off = cell_off + (size_t)t * (ncell + 1);
  if (t < first_step) {
    for (int c = tid; c <= ncell; c += BIN_THREADS) off[c] = 0;
    return;
  }
  for (int r = tid; r < n_all; r += BIN_THREADS) {
    const float2 p = paths[(size_t)r * H + t];
    lds_pts[r] = p;
    lds_cell[r] = bin_cell(p.x, lo0, inv0, nx) << 16 | bin_cell(p.y, lo1, inv1, ny);
  }
  __syncthreads();
  const int cpt = (ncell + BIN_THREADS - 1) / BIN_THREADS;
  const int c0 = min(tid * cpt, ncell), c1 = min(c0 + cpt, ncell);
  auto near = [&](int rc, int ix, int iy) { return abs((rc >> 16) - ix) <= 1 && abs((rc & 0xffff) - iy) <= 1; };
  int cnt = 0;
  for (int c = c0; c < c1; ++c) {
    const int ix = c / ny, iy = c - ix * ny;
    for (int r = 0; r < n_all; ++r) cnt += near(lds_cell[r], ix, iy) ? 1 : 0;
  }
  scan[tid] = cnt;
  __syncthreads();
  for (int d = 1; d < BIN_THREADS; d <<= 1) {                            // inclusive prefix sum over the threads
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int pos = scan[tid] - cnt;
  float4* const seg = entries + (size_t)t * 9 * n_all;
  for (int c = c0; c < c1; ++c) {
    const int ix = c / ny, iy = c - ix * ny;
    off[c] = pos;
    for (int r = 0; r < n_all; ++r)
      if (near(lds_cell[r], ix, iy)) {
        const float2 p = lds_pts[r];
        seg[pos++] = make_float4(p.x, p.y, __builtin_bit_cast(float, r), 0.f);
      }
  }
  if (tid == BIN_THREADS - 1) off[ncell] = scan[tid];
}

constexpr int BIN_MAX_ROBOTS = 4096, BIN_MAX_CELLS = 64;     // 12 B of LDS per robot in bin_cons_kernel; cells per axis

// a cell table as a guided step or a collision kernel may use it (every field but the two device arrays' contents)
int check_cons_bins(const mmd_cons_bins* b) {
  MMD_REQUIRE(b->cell_off_dev && b->entries_dev, "cons_bins: NULL table");
  MMD_REQUIRE(b->nx >= 1 && b->nx <= BIN_MAX_CELLS && b->ny >= 1 && b->ny <= BIN_MAX_CELLS, "cons_bins: grid %d x %d outside [1, %d]", b->nx,
              b->ny, BIN_MAX_CELLS);
  MMD_REQUIRE(b->n_all >= 2 && b->robot0 >= 0 && b->robot0 < b->n_all, "cons_bins: bad robot range");
  MMD_REQUIRE(b->radius > 0.f, "cons_bins: radius must be positive");
  for (int k = 0; k < 2; ++k)
    MMD_REQUIRE(b->inv_cell[k] > 0.f && 1.0 / (double)b->inv_cell[k] >= 1.0625 * (double)b->radius * (1.0 - 1e-6),
                "cons_bins: cells smaller than (1 + 1/16) x the radius");
  return 0;
}

// what an entry point that takes collision decisions on a cell table requires: its own checks, and margin <= radius (COVER, multi_agent.hip)
int check_collision_bins(const char* who, const mmd_cons_bins* bins, float margin) {
  MMD_REQUIRE(bins, "%s: NULL table", who);
  if (int rc = check_cons_bins(bins)) return rc;
  MMD_REQUIRE(margin <= bins->radius, "%s: margin %g above the table's radius %g (a list could miss a colliding robot)", who, margin,
              bins->radius);
  return 0;
}

// ---- the round table of a many-robot round: per local robot a hard group (conflict points), then the soft all-pairs group ------------
// Local robot r owns S = S_h + n_all - 1 slots from r S on: [r S, r S + S_h) is group 2 r (hard), the rest group 2 r + 1 (soft).  The
// offsets depend on no data, so the three kernels below need no sizing pass and no synchronisation between them.
// round_init_kernel: offsets, weights, every hard slot inactive, fill and dropped zeroed
__global__ void round_init_kernel(int n_local, int S_h, int S, float w_hard, float w_soft, float4* __restrict__ ell,
                                  int* __restrict__ grp_slot_off, float* __restrict__ grp_weight, int* __restrict__ robot_grp_off,
                                  int* __restrict__ fill, int* __restrict__ dropped) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t per = (size_t)S_h * H;
  for (size_t idx = tid; idx < (size_t)n_local * per; idx += step) {
    const size_t r = idx / per;
    ell[r * S * H + (idx - r * per)] = empty_word();
  }
  for (size_t idx = tid; idx < (size_t)n_local * H; idx += step) fill[idx] = 0;
  for (size_t r = tid; r <= (size_t)n_local; r += step) {
    robot_grp_off[r] = 2 * (int)r;
    grp_slot_off[2 * r] = (int)r * S;
    if (r == (size_t)n_local) break;
    grp_slot_off[2 * r + 1] = (int)r * S + S_h;
    grp_weight[2 * r] = w_hard;
    grp_weight[2 * r + 1] = w_soft;
    dropped[r] = 0;
  }
}

// The hard points of a round's conflicts (convert_conflicts_to_constraints, mmd/common/conflict_conversion.py:41-55: both agents of a
// conflict at tc get the midpoint with range (tc - t_pad, tc + t_pad)), appended behind what earlier rounds left.  One wave per local
// robot, lane = time step t, four robots a workgroup, no atomics, no LDS.  mmd_pack_constraints' rule -- a point's slot at t is the
// number of earlier points of the list active at t -- needs no list here: the robot's records in report order are tc ascending, then
// the other robot ascending (a record (tc, a, b) has a < b: the partners below the robot's id come first), a list of the cell table is
// in ascending id (COVER, multi_agent.hip: every partner is in the list of the robot's own cell), and the points active at t are those of
// tc in [t - t_pad + 1, t + t_pad].  So lane t walks exactly its own points in list order and counts its own slots.  The midpoint is
// write_conflict's (multi_agent.hip; the sum commutes: the same bits for both robots of the pair).  A point past slot S_h - 1: ColumnWriter.
__global__ __launch_bounds__(256) void conflict_constraints_kernel(const float2* __restrict__ paths, mmd_cons_bins b, int n_local, int S_h,
                                                                     int S, int t_pad, float margin, float radius, float4* __restrict__ ell,
                                                                     int* __restrict__ fill, int* __restrict__ dropped) {
  const int t = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_local) return;
  const int a = b.robot0 + r;
  ColumnWriter w{ell + (size_t)r * S * H + t, fill[(size_t)r * H + t], S_h, 0};   // the robot's hard block, column t
  const float r2 = slot_r2(radius);
  for (int tc = max(t - t_pad + 1, 0); tc <= min(t + t_pad, H - 1); ++tc) {
    const float2 pa = paths[(size_t)a * H + tc];
    const CellList l = own_cell_list(b, tc, pa.x, pa.y);
    for (int e = l.e0; e < l.e1; ++e) {
      const float4 q = l.ent[e];
      if (__builtin_bit_cast(int, q.z) == a || !rr_hit(pa, make_float2(q.x, q.y), margin)) continue;
      w.push((pa.x + q.x) / 2.f, (pa.y + q.y) / 2.f, radius, r2);
    }
  }
  fill[(size_t)r * H + t] = w.fill;
  const int drop = wave_sum(w.dropped);
  if (t == 0) dropped[r] += drop;
}

// ---- the framed all-pairs table: every robot plans in the model's tile frame, the robots meet in a global frame ---------------------
// Robot r's trajectory lives in the model's own frame (the tile [-1, 1]^2 the normaliser spans); off[r] places that window in the world:
// global = local + off[r].  The other robots' gathered paths are global, so robot r sees robot j's point at q = paths[j][t] - off[r] (one
// fp32 subtraction per axis).  The table keeps q only where it lies in the robot's WINDOW [window_lo, window_hi] (local frame, closed,
// plain fp32 compares: a NaN fails them and is left out), packed by mmd_pack_constraints' rule: the s-th kept robot, in ascending id, goes
// to slot s of column t.  So a robot owns S slots whatever n_all is, S is sized by the local density, and every guided-step kernel reads
// the table as it reads any other.
//
// WHY LEAVING THE OTHERS OUT IS EXACT.  The guided step un-normalises with an unconditional clip, so the position p it measures from lies
// in the normaliser's position limits [min, max] up to the rounding of (c + 1) / 2 (max - min) + min with c in [-1, 1]: a few ulp of the
// limits' magnitude.  A point acts on p only within its radius R: the guided step's test fma(dx, dx, dy dy) <= R|R| (guide.hip:
// cons_term) needs |dx|, |dy| <= R (1 + 2^-23) by guide.hip's COVER (the radicand is at least each rounded square).  The Python layer
// passes the window limits -/+ 1.0625 R -- the 1/16 slack of the cell rule.  A q outside it differs from every such p by more than
// 1.0625 R - (those few ulp) on one axis, which is above R by R / 16 less a few 1e-7: it can never act, at any step of any sample.  A
// table without it gives the guided step the same ACTIVE TERMS, in ascending id.  Not the same bits as the all-pairs table: the step
// sums a group's slots in four accumulators by slot index, and culling moves a robot to another slot, so the rounding of the sum may
// differ (the dense table's 2e-6 against the oracle holds for both); the host pack of the included points has the same slots and the
// same bits.  What the caller must keep true is only that the window covers limits -/+ R with that slack.
//
// One wave per local robot, lane = time step t, four robots a workgroup, no atomics, no LDS (conflict_constraints_kernel's shape).  Lane t
// reads paths[j][t]: the wave reads one 512-byte row per j, four rows a trip (the loads of a trip are issued together; a trip past the
// end re-reads the last row and drops it), and writes 1 KiB rows of the table.  O(n_all) per lane, whatever the density: a walk over
// candidate lists or a world cell table would be O(neighbours), and is not done here.  A kept point past slot S - 1 counts into dropped[i]
// (ColumnWriter); the slots from the fill on, and all of column 0 (constraints cover t >= 1), get the empty word of an unused slot.
__global__ __launch_bounds__(256) void framed_constraints_kernel(const float2* __restrict__ paths, const float2* __restrict__ offsets,
                                                                  int n_all, int robot0, int n_local, int S, float radius, float weight,
                                                                  float2 wlo, float2 whi, float4* __restrict__ ell,
                                                                  int* __restrict__ grp_slot_off, float* __restrict__ grp_weight,
                                                                  int* __restrict__ robot_grp_off, int* __restrict__ used,
                                                                  int* __restrict__ dropped) {
  const int t = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_local) return;
  const int r = robot0 + i;
  const float2 off = offsets[r];
  ColumnWriter w{ell + (size_t)i * S * H + t, 0, S, 0};                   // the robot's block, column t
  const float r2 = slot_r2(radius);
  for (int j0 = 0; j0 < n_all; j0 += 4) {
    float2 p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = paths[(size_t)min(j0 + k, n_all - 1) * H + t];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k;
      const float qx = p[k].x - off.x, qy = p[k].y - off.y;
      const bool in = qx >= wlo.x && qx <= whi.x && qy >= wlo.y && qy <= whi.y;
      if (!(t >= 1 && j < n_all && j != r && in)) continue;
      w.push(qx, qy, radius, r2);
    }
  }
  const int fill = wave_max(w.fill);
  w.fill_rest();
  const int drop = wave_sum(w.dropped);
  if (t == 0) {
    used[i] = fill; dropped[i] = drop;
    one_group_per_robot(i, n_local, S, weight, grp_slot_off, grp_weight, robot_grp_off);
  }
}

static void put_word(float* e, float4 w) { std::memcpy(e, &w, sizeof(w)); }   // (host memory that need not be 16-byte aligned)

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_pack_constraints(int n_groups, const int32_t* n_pts, const float* const* q, const float* const* t_range,
                         const float* const* radius, int horizon, float* ell_out, int max_slots, int32_t* slots_out) {
  MMD_REQUIRE(horizon == H, "mmd_pack_constraints: horizon must be %d", H);
  int used = 0;
  for (int g = 0; g < n_groups; ++g) {
    // a point is active at integer t iff t >= t0 and t < t1 (float ranges, cost_functions.py:304-305)
    std::vector<int> fill(H, 0);
    for (int c = 0; c < n_pts[g]; ++c) {
      const int t0 = (int)ceilf(t_range[g][2 * c]), t1 = (int)ceilf(t_range[g][2 * c + 1]);
      for (int t = t0 < 0 ? 0 : t0; t < t1 && t < H; ++t) ++fill[t];
    }
    int slots = 0;
    for (int t = 0; t < H; ++t) slots = fill[t] > slots ? fill[t] : slots;
    slots_out[g] = slots;
    if (!ell_out) { used += slots; continue; }      // sizing pass
    MMD_REQUIRE(used + slots <= max_slots, "mmd_pack_constraints: need more than %d slots", max_slots);
    for (size_t k = (size_t)used * H; k < (size_t)(used + slots) * H; ++k) put_word(ell_out + 4 * k, empty_word());
    fill.assign(H, 0);
    for (int c = 0; c < n_pts[g]; ++c) {
      const int t0 = (int)ceilf(t_range[g][2 * c]), t1 = (int)ceilf(t_range[g][2 * c + 1]);
      for (int t = t0 < 0 ? 0 : t0; t < t1 && t < H; ++t)
        put_word(ell_out + ((size_t)(used + fill[t]++) * H + t) * 4, slot_word(q[g][2 * c], q[g][2 * c + 1], radius[g][c]));
    }
    used += slots;
  }
  return 0;
}

int mmd_soft_constraints_from_paths(const float* paths_dev, int n_all, int robot0, int n_local, int horizon, float radius, float weight,
                                    float* ell_out_dev, int32_t* grp_slot_off_dev, float* grp_weight_dev, int32_t* robot_grp_off_dev,
                                    void* stream) {
  MMD_REQUIRE(horizon == H, "horizon must be %d", H);
  if (int rc = check_robot_range("mmd_soft_constraints_from_paths", n_all, robot0, n_local)) return rc;
  MMD_REQUIRE((long long)n_local * (n_all - 1) <= UINT_MAX, "mmd_soft_constraints_from_paths: a table of 2^32 slots or more");
  hipLaunchKernelGGL(all_pairs_kernel, dim3(grid_for((size_t)n_local * (n_all - 1) * H)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)paths_dev, n_all, robot0, n_local, 0, radius, weight, (float4*)ell_out_dev, grp_slot_off_dev,
                     grp_weight_dev, robot_grp_off_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

size_t mmd_cons_bins_bytes(int n_all, int nx, int ny, size_t* off_bytes, size_t* entry_bytes) {
  const bool ok = n_all >= 0 && nx >= 1 && ny >= 1;
  const size_t ob = ok ? (size_t)H * ((size_t)nx * ny + 1) * sizeof(int32_t) : 0;
  const size_t eb = ok ? (size_t)H * 9 * n_all * 4 * sizeof(float) : 0;
  if (off_bytes) *off_bytes = ob;
  if (entry_bytes) *entry_bytes = eb;
  return ob + eb;
}

// the table build behind mmd_bin_constraints_from_paths (first_step = 1) and mmd_bin_paths; `who` names the entry point in the error text
static int bin_paths(const char* who, const float* paths_dev, int n_all, int horizon, float radius, const float lo[2], const float hi[2],
                     int nx, int ny, int first_step, int32_t* cell_off_dev, float* entries_dev, void* stream) {
  MMD_REQUIRE(paths_dev && lo && hi && cell_off_dev && entries_dev, "%s: NULL argument", who);
  MMD_REQUIRE(horizon == H, "%s: horizon must be %d", who, H);
  MMD_REQUIRE(first_step == 0 || first_step == 1, "%s: first_step must be 0 or 1, got %d", who, first_step);
  MMD_REQUIRE(n_all >= 2 && n_all <= BIN_MAX_ROBOTS, "%s: n_all must be in [2, %d]", who, BIN_MAX_ROBOTS);
  MMD_REQUIRE(radius > 0.f, "%s: radius must be positive", who);
  MMD_REQUIRE(nx >= 1 && nx <= BIN_MAX_CELLS && ny >= 1 && ny <= BIN_MAX_CELLS, "%s: grid %d x %d outside [1, %d]", who, nx, ny,
              BIN_MAX_CELLS);
  const int n[2] = {nx, ny};
  float inv[2];
  for (int k = 0; k < 2; ++k) {
    MMD_REQUIRE(hi[k] > lo[k], "%s: empty limits", who);
    // the cover argument above bin_cell needs (1 + 1/16) R <= the cell side
    MMD_REQUIRE(((double)hi[k] - (double)lo[k]) / n[k] >= 1.0625 * (double)radius,
                "%s: cells smaller than (1 + 1/16) x the radius (axis %d: %g < %g)", who, k, ((double)hi[k] - (double)lo[k]) / n[k],
                1.0625 * (double)radius);
    inv[k] = (float)n[k] / (hi[k] - lo[k]);                  // mmd_cons_bins.inv_cell: this fp32 quotient
  }
  hipLaunchKernelGGL(bin_cons_kernel, dim3(H), dim3(BIN_THREADS), (size_t)n_all * 12 + BIN_THREADS * sizeof(int), (hipStream_t)stream,
                     (const float2*)paths_dev, n_all, lo[0], lo[1], inv[0], inv[1], nx, ny, first_step, cell_off_dev, (float4*)entries_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_bin_constraints_from_paths(const float* paths_dev, int n_all, int horizon, float radius, const float lo[2], const float hi[2],
                                   int nx, int ny, int32_t* cell_off_dev, float* entries_dev, void* stream) {
  return bin_paths("mmd_bin_constraints_from_paths", paths_dev, n_all, horizon, radius, lo, hi, nx, ny, 1, cell_off_dev, entries_dev, stream);
}

int mmd_bin_paths(const float* paths_dev, int n_all, int horizon, float reach, const float lo[2], const float hi[2], int nx, int ny,
                  int first_step, int32_t* cell_off_dev, float* entries_dev, void* stream) {
  return bin_paths("mmd_bin_paths", paths_dev, n_all, horizon, reach, lo, hi, nx, ny, first_step, cell_off_dev, entries_dev, stream);
}

// what the three round-table entry points require of the shape: the guided step indexes the table's (slot, t) words with an int
static int check_round_table(const char* who, int n_all, int robot0, int n_local, int horizon, int hard_slots) {
  MMD_REQUIRE(horizon == H, "%s: horizon must be %d", who, H);
  MMD_REQUIRE(hard_slots >= 1, "%s: hard_slots must be at least 1, got %d", who, hard_slots);
  if (int rc = check_robot_range(who, n_all, robot0, n_local)) return rc;
  MMD_REQUIRE((long long)n_local * ((long long)hard_slots + n_all - 1) * H <= INT_MAX, "%s: a table of more than 2^31 - 1 points", who);
  return 0;
}

int mmd_round_constraints_init(int n_all, int n_local, int horizon, int hard_slots, float weight_hard, float weight_soft, float* ell_dev,
                               int32_t* grp_slot_off_dev, float* grp_weight_dev, int32_t* robot_grp_off_dev, int32_t* fill_dev,
                               int32_t* dropped_dev, void* stream) {
  MMD_REQUIRE(ell_dev && grp_slot_off_dev && grp_weight_dev && robot_grp_off_dev && fill_dev && dropped_dev,
              "mmd_round_constraints_init: NULL argument");
  if (int rc = check_round_table("mmd_round_constraints_init", n_all, 0, n_local, horizon, hard_slots)) return rc;
  hipLaunchKernelGGL(round_init_kernel, dim3(grid_for((size_t)n_local * hard_slots * H)), dim3(256), 0, (hipStream_t)stream, n_local,
                     hard_slots, hard_slots + n_all - 1, weight_hard, weight_soft, (float4*)ell_dev, grp_slot_off_dev, grp_weight_dev,
                     robot_grp_off_dev, fill_dev, dropped_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_round_soft_from_paths(const float* paths_dev, int n_all, int robot0, int n_local, int horizon, int hard_slots, float radius,
                              float* ell_dev, void* stream) {
  MMD_REQUIRE(paths_dev && ell_dev, "mmd_round_soft_from_paths: NULL argument");
  if (int rc = check_round_table("mmd_round_soft_from_paths", n_all, robot0, n_local, horizon, hard_slots)) return rc;
  hipLaunchKernelGGL(all_pairs_kernel, dim3(grid_for((size_t)n_local * (n_all - 1) * H)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)paths_dev, n_all, robot0, n_local, hard_slots, radius, 0.f, (float4*)ell_dev, nullptr, nullptr, nullptr);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_conflict_constraints_append(const float* paths_dev, const mmd_cons_bins* bins, int n_local, int horizon, int hard_slots, int t_pad,
                                    float margin, float radius, float* ell_dev, int32_t* fill_dev, int32_t* dropped_dev, void* stream) {
  MMD_REQUIRE(paths_dev && ell_dev && fill_dev && dropped_dev, "mmd_conflict_constraints_append: NULL argument");
  MMD_REQUIRE(t_pad >= 1, "mmd_conflict_constraints_append: t_pad must be at least 1, got %d", t_pad);
  if (int rc = check_collision_bins("mmd_conflict_constraints_append", bins, margin)) return rc;
  if (int rc = check_round_table("mmd_conflict_constraints_append", bins->n_all, bins->robot0, n_local, horizon, hard_slots)) return rc;
  hipLaunchKernelGGL(conflict_constraints_kernel, dim3((n_local + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float2*)paths_dev,
                     *bins, n_local, hard_slots, hard_slots + bins->n_all - 1, t_pad < H ? t_pad : H, margin, radius, (float4*)ell_dev,
                     fill_dev, dropped_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_framed_constraints_from_paths(const float* paths_dev, const float* offsets_dev, int n_all, int robot0, int n_local, int horizon,
                                      int slots, float radius, float weight, const float window_lo[2], const float window_hi[2],
                                      float* ell_out_dev, int32_t* grp_slot_off_dev, float* grp_weight_dev, int32_t* robot_grp_off_dev,
                                      int32_t* used_dev, int32_t* dropped_dev, void* stream) {
  const char* who = "mmd_framed_constraints_from_paths";
  MMD_REQUIRE(paths_dev && offsets_dev && window_lo && window_hi && ell_out_dev && grp_slot_off_dev && grp_weight_dev && robot_grp_off_dev &&
                  used_dev && dropped_dev, "%s: NULL argument", who);
  MMD_REQUIRE(horizon == H, "%s: horizon must be %d", who, H);
  MMD_REQUIRE(n_all >= 2 && n_all <= 4096, "%s: n_all must be in [2, 4096], got %d", who, n_all);
  if (int rc = check_robot_range(who, n_all, robot0, n_local)) return rc;
  MMD_REQUIRE(slots >= 1 && slots <= n_all - 1, "%s: slots must be in [1, n_all - 1], got %d", who, slots);
  MMD_REQUIRE(radius > 0.f, "%s: radius must be positive", who);
  for (int k = 0; k < 2; ++k)
    MMD_REQUIRE(window_lo[k] < window_hi[k], "%s: empty window (axis %d: %g >= %g)", who, k, window_lo[k], window_hi[k]);
  // (n_local slots H <= 4096 x 4095 x 64 < 2^31: the guided step's int index of the table's (slot, t) words holds)
  hipLaunchKernelGGL(framed_constraints_kernel, dim3((n_local + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float2*)paths_dev,
                     (const float2*)offsets_dev, n_all, robot0, n_local, slots, radius, weight, make_float2(window_lo[0], window_lo[1]),
                     make_float2(window_hi[0], window_hi[1]), (float4*)ell_out_dev, grp_slot_off_dev, grp_weight_dev, robot_grp_off_dev,
                     used_dev, dropped_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
