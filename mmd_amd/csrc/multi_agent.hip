// Multi-agent layer pieces that sit right next to the sampler, so a planning round
// (gather -> sample -> pick the sample with the fewest robot-robot collisions -> conflicts) needs no host round trip:
//   * robot-robot collisions of the chosen best paths: RobotPlanarDisk.check_rr_collisions
//     (deps/torch_robotics/torch_robotics/robots/robot_planar_disk.py:173-203) as called by CBS.get_conflicts
//     (mmd/planners/multi_agent/cbs.py:166-246) for equal start times and densification 1;
//   * the 'least_collisions' batch scan (cbs.py:446-458): for every sample of a robot's batch, how many (t, other robot)
//     pairs collide with the other robots' best paths;
//   * the search layer of CBS / PrioritizedPlanning over agents with their own path lengths and start times
//     (cbs.py:166-246, :446-508; prioritized_planning.py:149-182, :212-298): the conflict list of a search state, the
//     'least_collisions' choice of a re-planned agent, and the soft / hard constraint table built from the other agents' paths.
//     Agent k's position at global time t is path_k[clamp(t - s_k, 0, L_k - 1)] (global_pad_paths, multi_agent_utils.py:120-143,
//     without the padded tensors);
//   * the same pick and the conflict report of a round's best paths on a CELL table of those paths (include/mmd_amd.h: mmd_cons_bins,
//     built by mmd_bin_paths with first_step = 0): a point meets only the robots in the list of its own cell, so a round of N robots
//     costs O(N x list length) where the kernels above walk all N (or all N^2 pairs);
//   * the round table of a many-robot round that repairs its conflicts: per local robot the hard points of the conflicts seen so far
//     (convert_conflicts_to_constraints, mmd/common/conflict_conversion.py:41-55; CBS passes them in front of the soft group,
//     cbs.py:407-413), appended round after round from the same cell table, and behind them the soft all-pairs group;
//   * which robots a round re-plans (mmd_round_select): the robots in conflict, or an independent set of the conflict graph found by
//     priority propagation on the same cell table -- CBS re-plans one agent of a conflict against the others' fixed paths (cbs.py:316-324);
//     a round does that for every robot of the set at once -- and the stable partition that makes the selected robots a prefix;
//   * the framed all-pairs table of a round in a world larger than one tile (mmd_framed_constraints_from_paths): every robot plans in
//     the model's tile frame at its own offset, and its table keeps the other robots' global points that fall into its window.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mmd_amd.h"
#include "bins_dev.h"             // own_cell_list / check_cons_bins: the cell table of guide.hip
#include "collision_dev.h"        // torch_norm2 / rr_hit: the pinned fp32 form of the collision decision (sets fp contract(off))
#include "common.h"
#include "wave_dev.h"             // wave_sum / block_sum / block_prefix / block_prefix_count

namespace mmd {

__global__ void rr_collisions_kernel(const float2* __restrict__ paths, int n, int T, float margin,
                                     unsigned char* __restrict__ mask, float2* __restrict__ mid) {
  const size_t tot = (size_t)T * n * n;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
    const int j = idx % n, i = (idx / n) % n, t = idx / ((size_t)n * n);
    const float2 a = paths[(size_t)i * T + t], b = paths[(size_t)j * T + t];
    const float dx = a.x - b.x, dy = a.y - b.y;
    const bool c = torch_norm2(dx, dy) < margin && i != j;
    mask[idx] = c ? 1 : 0;
    if (mid) {
      const float nanv = __builtin_nanf("");
      mid[idx] = c ? make_float2((a.x + b.x) / 2.f, (a.y + b.y) / 2.f) : make_float2(nanv, nanv);
    }
  }
}

// one wave per sample trajectory, lane = time step
__global__ __launch_bounds__(256) void count_collisions_kernel(const float4* __restrict__ trajs,
                                                               const float2* __restrict__ paths, int robot0,
                                                               int samples_per_robot, int n_traj, int n_all, float margin,
                                                               int* __restrict__ counts) {
  const int t = threadIdx.x & 63;
  const int traj = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (traj >= n_traj) return;
  const int self = robot0 + traj / samples_per_robot;
  const float4 p = trajs[(size_t)traj * H + t];
  int c = 0;
  for (int j = 0; j < n_all; ++j) {
    if (j == self) continue;
    const float2 q = paths[(size_t)j * H + t];
    const float dx = p.x - q.x, dy = p.y - q.y;
    c += torch_norm2(dx, dy) < margin ? 1 : 0;
  }
  c = wave_sum(c);
  if (t == 0) counts[traj] = c;
}

// ---- search layer over mmd_agent_path tables ----------------------------------------------------------------------------------------
__device__ __forceinline__ float2 sample_pos(const float* batch, int index, int length, int u) {
  const float* p = batch + ((size_t)index * length + u) * 4;
  return make_float2(p[0], p[1]);
}

// global_pad_paths: the start state before s_k, the last state after s_k + L_k - 1
__device__ __forceinline__ float2 agent_pos(const mmd_agent_path& a, int t) {
  int u = t - a.start_time;
  u = u < 0 ? 0 : (u > a.length - 1 ? a.length - 1 : u);
  return sample_pos(a.batch_dev, a.index, a.length, u);
}

// cell c of row t: (a, b) = (c / n, c % n); MMD_CONFLICTS_ORDERED keeps a != b (torch.nonzero order of cbs.py:193-246),
// MMD_CONFLICTS_PAIRS keeps a < b (the loops of prioritized_planning.py:271-298); `exclude` drops every pair with that agent
__device__ __forceinline__ bool cell_kept(int a, int b, int mode, int exclude) {
  if (a == exclude || b == exclude) return false;
  return mode == MMD_CONFLICTS_PAIRS ? a < b : a != b;
}

// what the two emit kernels do before they walk row t of `n_rows`: the number of records before the row (returned), and in the last row the
// total and, when it is 0, the first record that says "none"
__device__ __forceinline__ int records_before(const int* __restrict__ row_counts, int t, int n_rows, int* lds4, int* __restrict__ count,
                                              mmd_conflict* __restrict__ first) {
  int before = 0;
  for (int k = threadIdx.x; k < t; k += 256) before += row_counts[k];
  before = block_sum(before, lds4);
  if (t == n_rows - 1 && threadIdx.x == 0) {
    const int total = before + row_counts[t];
    *count = total;
    if (total == 0 && first) {
      mmd_conflict none{};
      none.t = none.a = none.b = -1;
      *first = none;
    }
  }
  return before;
}

// record idx of the (t, a, b) list: robots a at pa and b at pb at time step t
__device__ __forceinline__ void write_conflict(int idx, int t, int a, int b, float2 pa, float2 pb, mmd_conflict* __restrict__ first,
                                               mmd_conflict* __restrict__ list, int list_cap) {
  mmd_conflict r;
  r.t = t; r.a = a; r.b = b; r.reserved = 0;
  r.pa[0] = pa.x; r.pa[1] = pa.y; r.pb[0] = pb.x; r.pb[1] = pb.y;
  r.mid[0] = (pa.x + pb.x) / 2.f; r.mid[1] = (pa.y + pb.y) / 2.f;
  r.reserved2[0] = r.reserved2[1] = 0.f;
  if (idx == 0 && first) *first = r;
  if (list && idx < list_cap) list[idx] = r;
}

// one workgroup per global time step t: the number of conflicts in row t
__global__ __launch_bounds__(256) void conflict_rows_kernel(const mmd_agent_path* __restrict__ agents, int n, float margin,
                                                             int mode, int exclude, int* __restrict__ row_counts) {
  __shared__ int lds4[4];
  const int t = blockIdx.x;
  int c = 0;
  for (int cell = threadIdx.x; cell < n * n; cell += 256) {
    const int a = cell / n, b = cell % n;
    if (cell_kept(a, b, mode, exclude)) c += rr_hit(agent_pos(agents[a], t), agent_pos(agents[b], t), margin) ? 1 : 0;
  }
  c = block_sum(c, lds4);
  if (threadIdx.x == 0) row_counts[t] = c;
}

// one workgroup per t: the records of row t at their place in the (t, a, b) row-major list
__global__ __launch_bounds__(256) void conflict_emit_kernel(const mmd_agent_path* __restrict__ agents, int n, int Tg, float margin,
                                                             int mode, const int* __restrict__ row_counts, int* __restrict__ count,
                                                             mmd_conflict* __restrict__ first, mmd_conflict* __restrict__ list,
                                                             int list_cap) {
  __shared__ int lds4[4];
  const int t = blockIdx.x;
  const int before = records_before(row_counts, t, Tg, lds4, count, first);
  if (row_counts[t] == 0) return;
  const bool want_first = first && before == 0;
  const bool want_list = list && before < list_cap;
  if (!want_first && !want_list) return;
  int base = before;
  for (int c0 = 0; c0 < n * n; c0 += 256) {
    const int cell = c0 + threadIdx.x;
    const int a = cell / n, b = cell % n;
    bool hit = false;
    float2 pa = make_float2(0.f, 0.f), pb = pa;
    if (cell < n * n && cell_kept(a, b, mode, -1)) {
      pa = agent_pos(agents[a], t);
      pb = agent_pos(agents[b], t);
      hit = rr_hit(pa, pb, margin);
    }
    int prefix;
    const int total = block_prefix(hit, lds4, prefix);
    if (hit) write_conflict(base + prefix, t, a, b, pa, pb, first, list, list_cap);
    base += total;
  }
}

// ---- the pick and the conflict report on a cell table of the best paths -------------------------------------------------------------
//
// COVER (the argument of guide.hip's comment on bin_cell, for the collision decision): a point p meets a table point q iff rr_hit, i.e.
// sqrtf(s) < margin with s = fma(dy, dy, dx * dx) in fp32.  sqrtf is correctly rounded and monotone, so s < margin^2 (1 + 2^-22).  The
// exact radicand dy^2 + fl(dx * dx) is at least fl(dx * dx) and at least dy^2, and rounding is monotone: s >= fl(dx * dx) >=
// dx^2 (1 - 2^-24) and s >= fl(dy^2) >= dy^2 (1 - 2^-24).  Hence |dx|, |dy| < margin (1 + 2^-22): a few ulp over margin.  With
// margin <= bins->radius that is the bound the cell rule (cells >= (1 + 1/16) x radius) was made for: the cell indices of p and q
// differ by at most 1 per axis, so q is in the list of p's own cell, and the entry points refuse margin > radius.
// A count is an integer: the order of a list does not matter to it, only that every hit is in the list exactly once (a robot has one
// entry per time step and list) and that the robot's own entry is skipped by id.  The table must list time step 0 (mmd_bin_paths with
// first_step = 0): the dense kernels count collisions there.

// count_collisions_kernel on the table: one wave per trajectory, lane = time step, four trajectories a workgroup, no LDS.  The wave
// walks the lanes' lists four entries a trip -- the loads of a trip are issued together -- while any lane has entries left; a lane past
// its list re-reads an entry of the segment and drops it.  P = float4 (sample trajectories) or float2 (the best paths themselves: the
// per-robot counts of the conflict report).
template <typename P>
__global__ __launch_bounds__(256) void count_collisions_binned_kernel(const P* __restrict__ pts, mmd_cons_bins b, int robot0,
                                                                      int samples_per_robot, int n_traj, float margin,
                                                                      int* __restrict__ counts) {
  const int t = threadIdx.x & 63;
  const int traj = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (traj >= n_traj) return;
  const int self = robot0 + traj / samples_per_robot;
  const P pt = pts[(size_t)traj * H + t];
  const float2 p = make_float2(pt.x, pt.y);
  const CellList l = own_cell_list(b, t, p.x, p.y);
  const int last = max(l.e1 - 1, 0);
  int c = 0;
  for (int e = l.e0; __builtin_amdgcn_ballot_w64(e < l.e1) != 0; e += 4) {
    float4 q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = l.ent[min(e + j, last)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool other = e + j < l.e1 && __builtin_bit_cast(int, q[j].z) != self;
      c += other && rr_hit(p, make_float2(q[j].x, q[j].y), margin) ? 1 : 0;
    }
  }
  c = wave_sum(c);
  if (t == 0) counts[traj] = c;
}

// the number of robots b > a that robot a (at pa, time step t) collides with: the entries of its own list above its id
__device__ __forceinline__ int pairs_above(const CellList& l, int a, float2 pa, float margin) {
  int c = 0;
  for (int e = l.e0; e < l.e1; ++e) {
    const float4 q = l.ent[e];
    c += __builtin_bit_cast(int, q.z) > a && rr_hit(pa, make_float2(q.x, q.y), margin) ? 1 : 0;
  }
  return c;
}

// conflict_rows_kernel (MMD_CONFLICTS_PAIRS, equal start times) on the table: one workgroup per time step, a thread per robot
__global__ __launch_bounds__(256) void path_conflict_rows_binned_kernel(const float2* __restrict__ paths, mmd_cons_bins b, float margin,
                                                                         int* __restrict__ row_counts) {
  __shared__ int lds4[4];
  const int t = blockIdx.x;
  int c = 0;
  for (int a = threadIdx.x; a < b.n_all; a += 256) {
    const float2 pa = paths[(size_t)a * H + t];
    c += pairs_above(own_cell_list(b, t, pa.x, pa.y), a, pa, margin);
  }
  c = block_sum(c, lds4);
  if (threadIdx.x == 0) row_counts[t] = c;
}

// conflict_emit_kernel on the table: the records of row t at their place in the (t, a, b) list, a < b.  Robots in blocks of 256 in
// ascending id; robot a's records are the entries of its own list above its id, which a list holds in ascending id: a first pass counts
// them, the block's prefix places them, a second pass writes them.  No atomics: the list is the same on every run.
__global__ __launch_bounds__(256) void path_conflict_emit_binned_kernel(const float2* __restrict__ paths, mmd_cons_bins b, float margin,
                                                                         const int* __restrict__ row_counts, int* __restrict__ count,
                                                                         mmd_conflict* __restrict__ first, mmd_conflict* __restrict__ list,
                                                                         int list_cap) {
  __shared__ int lds4[4];
  const int t = blockIdx.x;
  const int before = records_before(row_counts, t, H, lds4, count, first);
  if (row_counts[t] == 0) return;
  const bool want_first = first && before == 0;
  if (!want_first && !(list && before < list_cap)) return;
  int base = before;
  for (int a0 = 0; a0 < b.n_all; a0 += 256) {
    if (base > 0 && base >= list_cap) return;               // (the rest of the row lies past the list; uniform over the block)
    const int a = a0 + threadIdx.x;
    float2 pa = make_float2(0.f, 0.f);
    CellList l{nullptr, 0, 0};
    int mine = 0;
    if (a < b.n_all) {
      pa = paths[(size_t)a * H + t];
      l = own_cell_list(b, t, pa.x, pa.y);
      mine = pairs_above(l, a, pa, margin);
    }
    int idx;
    const int total = block_prefix_count(mine, lds4, idx);
    idx += base;
    for (int e = l.e0; mine > 0 && e < l.e1; ++e) {
      const float4 q = l.ent[e];
      const int ob = __builtin_bit_cast(int, q.z);
      const float2 pb = make_float2(q.x, q.y);
      if (!(ob > a && rr_hit(pa, pb, margin))) continue;
      write_conflict(idx++, t, a, ob, pa, pb, first, list, list_cap);
      --mine;
    }
    base += total;
  }
}

// one wave per candidate, lane = global time step: #{(t, j != self) : candidate(t) hits agent j(t)}
__global__ __launch_bounds__(256) void candidate_pairs_kernel(const mmd_agent_path* __restrict__ agents, int n, int Tg, int self,
                                                               const float* __restrict__ cand_batch, const int* __restrict__ cand_idx,
                                                               int n_cand, float margin, int* __restrict__ pair_counts) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_cand) return;
  const mmd_agent_path me = agents[self];
  const int idx = cand_idx[c];
  int hits = 0;
  for (int t = lane; t < Tg; t += 64) {
    int u = t - me.start_time;
    u = u < 0 ? 0 : (u > me.length - 1 ? me.length - 1 : u);
    const float2 p = sample_pos(cand_batch, idx, me.length, u);
    for (int j = 0; j < n; ++j)
      if (j != self) hits += rr_hit(p, agent_pos(agents[j], t), margin) ? 1 : 0;
  }
  hits = wave_sum(hits);
  if (lane == 0) pair_counts[c] = hits;
}

// the selection rule over the n_free candidates (candidate n_free = the PP rule's starting sample), one workgroup
__global__ __launch_bounds__(256) void select_candidate_kernel(const int* __restrict__ base_rows, int Tg, const int* __restrict__ pair_counts,
                                                                const int* __restrict__ cand_idx, int n_free, int mult, int rule,
                                                                int* __restrict__ counts_out, int* __restrict__ result) {
  __shared__ int lds4[4];
  __shared__ long long best_w[4];
  int b = 0;
  for (int k = threadIdx.x; k < Tg; k += 256) b += base_rows[k];
  const int base = block_sum(b, lds4);
  // (count, position) packed so that the minimum is the FIRST candidate with the smallest count
  long long best = LLONG_MAX;
  for (int c = threadIdx.x; c < n_free; c += 256) {
    const int total = base + mult * pair_counts[c];
    if (counts_out) counts_out[c] = total;
    const long long key = ((long long)total << 32) | (unsigned)c;
    best = key < best ? key : best;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const long long o = __shfl_xor(best, m);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) best_w[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) best = best_w[w] < best ? best_w[w] : best;
    int pick = -1, count = -1;
    if (best != LLONG_MAX) {
      pick = cand_idx[(int)(best & 0xffffffffll)];
      count = (int)(best >> 32);
    }
    if (rule == MMD_SELECT_PP) {                 // start from idx_best_traj; only a strictly smaller count replaces it
      const int init = base + mult * pair_counts[n_free];
      if (pick < 0 || count >= init) {
        pick = cand_idx[n_free];
        count = init;
      }
    }
    result[0] = pick;
    result[1] = count;
  }
}

// thread t of agent `self`'s horizon: slot s holds the s-th other agent (in agent order) with a point active at t
__global__ void path_constraints_kernel(const mmd_agent_path* __restrict__ agents, int n_state, int self, int self_start, int self_last,
                                        int hard, int horizon, float radius, float weight, int n_slots, float4* __restrict__ ell,
                                        int* __restrict__ grp_slot_off, float* __restrict__ grp_weight, int* __restrict__ robot_grp_off) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && grp_slot_off) {                   // one group of n_slots slots for one robot
    grp_slot_off[0] = 0; grp_slot_off[1] = n_slots;
    grp_weight[0] = weight;
    robot_grp_off[0] = 0; robot_grp_off[1] = 1;
  }
  if (t >= horizon) return;
  int fill = 0;
  // soft: range (t, t + 1); hard: clamped to (max(0, min(t, H-1)), min(H-1, t + 1)), i.e. active only for t <= H - 2
  const bool active = t >= 1 && (!hard || t <= horizon - 2);
  if (active) {
    for (int j = 0; j < n_state && fill < n_slots; ++j) {
      if (j == self) continue;
      const mmd_agent_path o = agents[j];
      const int tj = t + self_start - o.start_time;
      const int last = self_last >= 0 ? self_last : o.length - 1;
      if (tj < 0 || tj > o.length - 1 || t > last) continue;
      const float2 p = sample_pos(o.batch_dev, o.index, o.length, tj);
      ell[(size_t)fill * horizon + t] = make_float4(p.x, p.y, radius, radius * fabsf(radius));
      ++fill;
    }
  }
  for (; fill < n_slots; ++fill) ell[(size_t)fill * horizon + t] = make_float4(0.f, 0.f, -1.f, -1.f);
}

// ---- the round table of a many-robot round: per local robot a hard group (conflict points), then the soft all-pairs group ------------
//
// Local robot r owns S = S_h + n_all - 1 slots from r S on: [r S, r S + S_h) is group 2 r (hard), the rest group 2 r + 1 (soft).  The
// offsets depend on no data, so the three kernels below need no sizing pass and no synchronisation between them.

// offsets, weights, every hard slot inactive, fill and dropped zeroed
__global__ void round_init_kernel(int n_local, int S_h, int S, float w_hard, float w_soft, float4* __restrict__ ell,
                                  int* __restrict__ grp_slot_off, float* __restrict__ grp_weight, int* __restrict__ robot_grp_off,
                                  int* __restrict__ fill, int* __restrict__ dropped) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t per = (size_t)S_h * H;
  for (size_t idx = tid; idx < (size_t)n_local * per; idx += step) {
    const size_t r = idx / per;
    ell[r * S * H + (idx - r * per)] = make_float4(0.f, 0.f, -1.f, -1.f);
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

// the soft block of every local robot: the words soft_cons_kernel (guide.hip) writes for that robot, behind its hard block
__global__ void round_soft_kernel(const float2* __restrict__ paths, int n_all, int robot0, int n_local, int S_h, float radius,
                                  float4* __restrict__ ell) {
  const int slots = n_all - 1, S = S_h + slots;
  const size_t tot = (size_t)n_local * slots * H;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
    const int t = idx % H;
    const int j = (idx / H) % slots;
    const int i = idx / ((size_t)H * slots);
    const int other = j + (j >= robot0 + i ? 1 : 0);
    const float2 p = paths[(size_t)other * H + t];
    const float r = t >= 1 ? radius : -1.f;                               // constraints cover t in [1, H-1]
    ell[((size_t)i * S + S_h + j) * H + t] = make_float4(p.x, p.y, r, r * fabsf(r));
  }
}

// The hard points of a round's conflicts (convert_conflicts_to_constraints, mmd/common/conflict_conversion.py:41-55: both agents of a
// conflict at tc get the midpoint with range (tc - t_pad, tc + t_pad)), appended behind what earlier rounds left.  One wave per local
// robot, lane = time step t, four robots a workgroup, no atomics, no LDS.  mmd_pack_constraints' rule -- a point's slot at t is the
// number of earlier points of the list active at t -- needs no list here: the robot's records in report order are tc ascending, then
// the other robot ascending (a record (tc, a, b) has a < b: the partners below the robot's id come first), a list of the cell table is
// in ascending id (COVER above: every partner is in the list of the robot's own cell), and the points active at t are those of
// tc in [t - t_pad + 1, t + t_pad].  So lane t walks exactly its own points in list order and counts its own slots.  The midpoint is
// write_conflict's expression (the sum commutes: the same bits whichever robot of the pair the lane serves).  A point past slot
// S_h - 1 is dropped and counted; the lane's fill stays at S_h, so everything later is dropped too and what was written is a prefix.
__global__ __launch_bounds__(256) void conflict_constraints_kernel(const float2* __restrict__ paths, mmd_cons_bins b, int n_local, int S_h,
                                                                    int S, int t_pad, float margin, float radius, float4* __restrict__ ell,
                                                                    int* __restrict__ fill, int* __restrict__ dropped) {
  const int t = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_local) return;
  const int a = b.robot0 + r;
  float4* const col = ell + (size_t)r * S * H + t;                        // the robot's hard block, column t
  const float r2 = radius * fabsf(radius);
  int f = fill[(size_t)r * H + t], drop = 0;
  const int tc1 = min(t + t_pad, H - 1);
  for (int tc = max(t - t_pad + 1, 0); tc <= tc1; ++tc) {
    const float2 pa = paths[(size_t)a * H + tc];
    const CellList l = own_cell_list(b, tc, pa.x, pa.y);
    for (int e = l.e0; e < l.e1; ++e) {
      const float4 q = l.ent[e];
      if (__builtin_bit_cast(int, q.z) == a || !rr_hit(pa, make_float2(q.x, q.y), margin)) continue;
      if (f < S_h) {
        col[(size_t)f * H] = make_float4((pa.x + q.x) / 2.f, (pa.y + q.y) / 2.f, radius, r2);
        ++f;
      } else {
        ++drop;
      }
    }
  }
  fill[(size_t)r * H + t] = f;
  drop = wave_sum(drop);
  if (t == 0) dropped[r] += drop;
}

// ---- the framed all-pairs table: every robot plans in the model's tile frame, the robots meet in a global frame ---------------------
//
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
// cons_term) needs |dx|, |dy| <= R (1 + 2^-23) by COVER's argument (the radicand is at least each rounded square).  The Python layer
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
// candidate lists or a world cell table would be O(neighbours), and is not done here.  A kept point past slot S - 1 is not written and
// counts into dropped[i]; the lane's fill stays at S, so what was written is a prefix of the list.  Slots from the fill on, and all of
// column 0 (constraints cover t >= 1), get the empty word (0, 0, -1, -1) mmd_pack_constraints leaves in an unused slot.
__global__ __launch_bounds__(256) void framed_constraints_kernel(const float2* __restrict__ paths, const float2* __restrict__ offsets,
                                                                  int n_all, int robot0, int n_local, int S, float radius, float weight,
                                                                  float2 wlo, float2 whi, float4* __restrict__ ell,
                                                                  int* __restrict__ grp_slot_off, float* __restrict__ grp_weight,
                                                                  int* __restrict__ robot_grp_off, int* __restrict__ used,
                                                                  int* __restrict__ dropped) {
  const int t = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_local) return;
  const int r = robot0 + i;
  const float2 off = offsets[r];
  float4* const col = ell + (size_t)i * S * H + t;                        // the robot's block, column t
  const float r2 = radius * fabsf(radius);
  int f = 0, drop = 0;
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
      if (f < S) {
        col[(size_t)f * H] = make_float4(qx, qy, radius, r2);
        ++f;
      } else {
        ++drop;
      }
    }
  }
  const int fill = wave_max(f);
  for (; f < S; ++f) col[(size_t)f * H] = make_float4(0.f, 0.f, -1.f, -1.f);
  drop = wave_sum(drop);
  if (t == 0) {                                                           // one group of S slots per robot
    used[i] = fill;
    dropped[i] = drop;
    grp_slot_off[i] = i * S;
    grp_weight[i] = weight;
    robot_grp_off[i] = i;
    if (i == n_local - 1) {
      grp_slot_off[n_local] = n_local * S;
      robot_grp_off[n_local] = n_local;
    }
  }
}

// ---- which robots a round re-plans: the robots in conflict, or an independent set of the conflict graph -----------------------------
//
// The conflict graph: robots r != j are neighbours iff rr_hit(p_r(t), p_j(t), margin) at some t in [0, H).  rr_hit is symmetric in its two
// points (dx and dy change sign, dx * dx and dy * dy do not), so the graph is undirected: whatever robot r's wave sees of j, j's wave sees
// of r.  COVER above applies to the walk (margin <= bins->radius is enforced): a robot's neighbours at t are all in the list of its own cell
// at t.  A robot with a neighbour has a count above 0, its neighbour too.  Priority is a total order: r beats j iff counts[r] > counts[j],
// or the counts are equal and r < j.
//
// Every robot has a state; at the start OUT if its count is 0, else UNDECIDED.  One Jacobi iteration reads only the old array and writes
// the new one: an UNDECIDED r becomes OUT if a neighbour is IN, else IN if every neighbour that beats it is OUT, else it stays.  IN and
// OUT are final.  For every number of iterations:
//   INDEPENDENT -- no two neighbours are IN.  Say neighbours r and j both are, and r beats j.  If they turned IN in the same iteration, j
//     needed r OUT in the old array, where r was UNDECIDED.  If j turned later, r was IN in the old array and j became OUT; if r turned
//     later, j (a neighbour, whether it beats r or not) was IN in the old array and r became OUT.
//   NON-EMPTY -- where there is a conflict, the robot that beats every other robot of a count above 0 has no neighbour that beats it:
//     the first iteration makes it IN (nothing is IN before), and it stays.
//   NEIGHBOURS STAY -- every neighbour of a selected robot is not selected: that is INDEPENDENT read from one robot.  So a re-planned robot
//     is guided against neighbours that keep their paths this round.
// Iteration 1 selects the strict local maxima of the priority; the limit is the lexicographically first maximal independent set in
// priority order.
#define MMD_SEL_UNDECIDED 0
#define MMD_SEL_IN 1
#define MMD_SEL_OUT 2

// MMD_REPLAN_CONFLICTED as a state array: IN where the count is above 0, else OUT
__global__ void round_select_conflicted_kernel(const int* __restrict__ counts, int n_all, int* __restrict__ state) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_all) state[r] = counts[r] > 0 ? MMD_SEL_IN : MMD_SEL_OUT;
}

// One iteration, in the shape of count_collisions_binned_kernel<float2>: one wave per robot, lane = time step, four robots a workgroup,
// the lane's own cell list four entries a trip, no LDS, no atomics.  `old_state` NULL: the first iteration, whose old array is the
// start state, read off the counts.  A robot that is decided copies its state without a walk (uniform over the wave).  The two
// predicates of the rule are reduced over the wave's lanes with one ballot each.
__global__ __launch_bounds__(256) void round_select_iter_kernel(const float2* __restrict__ paths, mmd_cons_bins b, float margin,
                                                                const int* __restrict__ counts, const int* __restrict__ old_state,
                                                                int* __restrict__ new_state) {
  const int t = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= b.n_all) return;
  const int mine = counts[r];
  const int st = old_state ? old_state[r] : (mine == 0 ? MMD_SEL_OUT : MMD_SEL_UNDECIDED);
  if (st != MMD_SEL_UNDECIDED) {
    if (t == 0) new_state[r] = st;
    return;
  }
  const float2 p = paths[(size_t)r * H + t];
  const CellList l = own_cell_list(b, t, p.x, p.y);
  const int last = max(l.e1 - 1, 0);
  bool near_in = false, held = false;                       // a neighbour is IN; a neighbour that beats r is not OUT
  for (int e = l.e0; __builtin_amdgcn_ballot_w64(e < l.e1) != 0; e += 4) {
    float4 q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = l.ent[min(e + j, last)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = __builtin_bit_cast(int, q[j].z);
      if (!(e + j < l.e1 && o != r && rr_hit(p, make_float2(q[j].x, q[j].y), margin))) continue;
      const int oc = counts[o];
      const int os = old_state ? old_state[o] : MMD_SEL_UNDECIDED;      // (a neighbour has a count above 0)
      near_in |= os == MMD_SEL_IN;
      held |= os != MMD_SEL_OUT && (oc > mine || (oc == mine && o < r));
    }
  }
  const bool any_in = __builtin_amdgcn_ballot_w64(near_in) != 0;
  const bool any_held = __builtin_amdgcn_ballot_w64(held) != 0;
  if (t == 0) new_state[r] = any_in ? MMD_SEL_OUT : (any_held ? MMD_SEL_UNDECIDED : MMD_SEL_IN);
}

// selected, the stable partition and the header from the final states: one workgroup, the robots in chunks of 256 in ascending id, no
// atomics.  A first pass counts; in the second the block's prefix places a selected robot behind the selected robots below it and any
// other robot behind all n_sel selected ones, at its rank among the robots not selected.
__global__ __launch_bounds__(256) void round_select_partition_kernel(const int* __restrict__ state, int n_all, int robot0, int n_local,
                                                                     int* __restrict__ selected, int* __restrict__ perm,
                                                                     int* __restrict__ header) {
  __shared__ int lds4[4];
  int n_sel = 0, below = 0, inside = 0, undecided = 0;
  for (int r = threadIdx.x; r < n_all; r += 256) {
    const int st = state[r];
    const int in = st == MMD_SEL_IN ? 1 : 0;
    n_sel += in;
    below += r < robot0 ? in : 0;
    inside += r >= robot0 && r < robot0 + n_local ? in : 0;
    undecided += st == MMD_SEL_UNDECIDED ? 1 : 0;
  }
  n_sel = block_sum(n_sel, lds4);
  below = block_sum(below, lds4);
  inside = block_sum(inside, lds4);
  undecided = block_sum(undecided, lds4);
  if (threadIdx.x == 0) {
    header[0] = n_sel; header[1] = below; header[2] = inside; header[3] = undecided;
  }
  int base = 0;                                              // selected robots below the chunk
  for (int r0 = 0; r0 < n_all; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const bool in = r < n_all && state[r] == MMD_SEL_IN;
    int prefix;
    const int total = block_prefix(in, lds4, prefix);
    if (r < n_all) {
      const int sel_below = base + prefix;
      selected[r] = in ? 1 : 0;
      perm[in ? sel_below : n_sel + (r - sel_below)] = r;
    }
    base += total;
  }
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_rr_collisions(const float* paths_dev, int n_robots, int horizon, float margin, uint8_t* mask_dev,
                      float* midpoints_dev, void* stream) {
  MMD_REQUIRE(paths_dev && mask_dev && n_robots >= 1 && horizon >= 1, "mmd_rr_collisions: bad arguments");
  const size_t tot = (size_t)horizon * n_robots * n_robots;
  int grid = (int)((tot + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(rr_collisions_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float2*)paths_dev,
                     n_robots, horizon, margin, mask_dev, (float2*)midpoints_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_count_collisions(const float* trajs_dev, const float* paths_dev, int robot0, int n_local,
                         int samples_per_robot, int n_all, int horizon, float margin, int32_t* counts_dev, void* stream) {
  MMD_REQUIRE(trajs_dev && paths_dev && counts_dev, "mmd_count_collisions: NULL argument");
  MMD_REQUIRE(horizon == H, "horizon must be %d", H);
  MMD_REQUIRE(n_local >= 1 && samples_per_robot >= 1 && robot0 >= 0 && robot0 + n_local <= n_all, "bad robot range");
  const int n_traj = n_local * samples_per_robot;
  hipLaunchKernelGGL(count_collisions_kernel, dim3((n_traj + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)trajs_dev, (const float2*)paths_dev, robot0, samples_per_robot, n_traj, n_all, margin,
                     counts_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

// what the two report entry points require of the list: a capacity, and a pointer where it is positive; a list of 0 records is none
static int check_conflict_list(const char* who, mmd_conflict*& list_dev, int list_cap) {
  MMD_REQUIRE(list_cap >= 0 && (list_cap == 0 || list_dev), "%s: list_cap without a list", who);
  if (list_cap == 0) list_dev = nullptr;
  return 0;
}

// what the two collision entry points on a cell table share: the table's own checks, and margin <= radius (COVER above)
static int check_collision_bins(const char* who, const mmd_cons_bins* bins, float margin) {
  MMD_REQUIRE(bins, "%s: NULL table", who);
  if (int rc = check_cons_bins(bins)) return rc;
  MMD_REQUIRE(margin <= bins->radius, "%s: margin %g above the table's radius %g (a list could miss a colliding robot)", who, margin,
              bins->radius);
  return 0;
}

int mmd_count_collisions_binned(const float* trajs_dev, const mmd_cons_bins* bins, int n_local, int samples_per_robot, float margin,
                                int32_t* counts_dev, void* stream) {
  MMD_REQUIRE(trajs_dev && counts_dev, "mmd_count_collisions_binned: NULL argument");
  if (int rc = check_collision_bins("mmd_count_collisions_binned", bins, margin)) return rc;
  MMD_REQUIRE(n_local >= 1 && samples_per_robot >= 1 && bins->robot0 + n_local <= bins->n_all, "mmd_count_collisions_binned: bad robot range");
  const int n_traj = n_local * samples_per_robot;
  hipLaunchKernelGGL(count_collisions_binned_kernel<float4>, dim3((n_traj + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)trajs_dev, *bins, bins->robot0, samples_per_robot, n_traj, margin, counts_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_path_conflicts_binned(const float* paths_dev, const mmd_cons_bins* bins, int horizon, float margin, int32_t* row_counts_dev,
                              int32_t* robot_counts_dev, int32_t* count_dev, mmd_conflict* first_dev, mmd_conflict* list_dev, int list_cap,
                              void* stream) {
  MMD_REQUIRE(paths_dev && row_counts_dev && count_dev, "mmd_path_conflicts_binned: NULL argument");
  MMD_REQUIRE(horizon == H, "mmd_path_conflicts_binned: horizon must be %d", H);
  if (int rc = check_conflict_list("mmd_path_conflicts_binned", list_dev, list_cap)) return rc;
  if (int rc = check_collision_bins("mmd_path_conflicts_binned", bins, margin)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float2* paths = (const float2*)paths_dev;
  hipLaunchKernelGGL(path_conflict_rows_binned_kernel, dim3(H), dim3(256), 0, st, paths, *bins, margin, row_counts_dev);
  hipLaunchKernelGGL(path_conflict_emit_binned_kernel, dim3(H), dim3(256), 0, st, paths, *bins, margin, row_counts_dev, count_dev, first_dev,
                     list_dev, list_cap);
  if (robot_counts_dev)                                  // every robot's own path as a "sample" of one: each pair counts for both robots
    hipLaunchKernelGGL(count_collisions_binned_kernel<float2>, dim3((bins->n_all + 3) / 4), dim3(256), 0, st, paths, *bins, 0, 1,
                       bins->n_all, margin, robot_counts_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_find_conflicts(const mmd_agent_path* agents_dev, int n_agents, int horizon_global, float margin, int mode,
                       int32_t* row_counts_dev, int32_t* count_dev, mmd_conflict* first_dev, mmd_conflict* list_dev, int list_cap,
                       void* stream) {
  MMD_REQUIRE(agents_dev && row_counts_dev && count_dev && n_agents >= 1 && horizon_global >= 1, "mmd_find_conflicts: bad arguments");
  MMD_REQUIRE(mode == MMD_CONFLICTS_ORDERED || mode == MMD_CONFLICTS_PAIRS, "mmd_find_conflicts: unknown mode %d", mode);
  if (int rc = check_conflict_list("mmd_find_conflicts", list_dev, list_cap)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conflict_rows_kernel, dim3(horizon_global), dim3(256), 0, st, agents_dev, n_agents, margin, mode, -1,
                     row_counts_dev);
  hipLaunchKernelGGL(conflict_emit_kernel, dim3(horizon_global), dim3(256), 0, st, agents_dev, n_agents, horizon_global, margin, mode,
                     row_counts_dev, count_dev, first_dev, list_dev, list_cap);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_scan_candidates(const mmd_agent_path* agents_dev, int n_agents, int horizon_global, int agent, const float* cand_batch_dev,
                        const int32_t* cand_idx_dev, int n_free, float margin, int mode, int rule, int32_t* scratch_dev,
                        int32_t* counts_dev, int32_t* result_dev, void* stream) {
  MMD_REQUIRE(agents_dev && scratch_dev && result_dev, "mmd_scan_candidates: NULL argument");
  MMD_REQUIRE(n_agents >= 1 && agent >= 0 && agent < n_agents && horizon_global >= 1 && n_free >= 0, "mmd_scan_candidates: bad arguments");
  MMD_REQUIRE(mode == MMD_CONFLICTS_ORDERED || mode == MMD_CONFLICTS_PAIRS, "mmd_scan_candidates: unknown mode %d", mode);
  MMD_REQUIRE(rule == MMD_SELECT_CBS || rule == MMD_SELECT_PP, "mmd_scan_candidates: unknown rule %d", rule);
  const int n_cand = n_free + (rule == MMD_SELECT_PP ? 1 : 0);
  // CBS without candidates reads neither (an empty index tensor has no storage): the result is (-1, -1)
  MMD_REQUIRE(n_cand == 0 || (cand_batch_dev && cand_idx_dev), "mmd_scan_candidates: NULL candidates");
  hipStream_t st = (hipStream_t)stream;
  int32_t* base_rows = scratch_dev;                    // [horizon_global]
  int32_t* pairs = scratch_dev + horizon_global;       // [n_cand]
  hipLaunchKernelGGL(conflict_rows_kernel, dim3(horizon_global), dim3(256), 0, st, agents_dev, n_agents, margin, mode, agent, base_rows);
  if (n_cand > 0)
    hipLaunchKernelGGL(candidate_pairs_kernel, dim3((n_cand + 3) / 4), dim3(256), 0, st, agents_dev, n_agents, horizon_global, agent,
                       cand_batch_dev, (const int*)cand_idx_dev, n_cand, margin, pairs);
  hipLaunchKernelGGL(select_candidate_kernel, dim3(1), dim3(256), 0, st, base_rows, horizon_global, pairs, (const int*)cand_idx_dev,
                     n_free, mode == MMD_CONFLICTS_ORDERED ? 2 : 1, rule, counts_dev, result_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

int mmd_path_constraints(const mmd_agent_path* agents_dev, int n_state, int agent, int agent_start_time, int agent_last_t, int hard,
                         int horizon, float radius, float weight, int n_slots, float* ell_out_dev, int32_t* grp_slot_off_dev,
                         float* grp_weight_dev, int32_t* robot_grp_off_dev, void* stream) {
  MMD_REQUIRE(agents_dev && ell_out_dev && n_state >= 0 && n_slots >= 0, "mmd_path_constraints: bad arguments");
  MMD_REQUIRE(horizon == H, "mmd_path_constraints: horizon must be %d", H);
  const bool offsets = grp_slot_off_dev && grp_weight_dev && robot_grp_off_dev;
  MMD_REQUIRE(offsets || !(grp_slot_off_dev || grp_weight_dev || robot_grp_off_dev), "mmd_path_constraints: all three offset arrays or none");
  if (n_slots > 0 || offsets)
    hipLaunchKernelGGL(path_constraints_kernel, dim3(1), dim3(H), 0, (hipStream_t)stream, agents_dev, n_state, agent, agent_start_time,
                       agent_last_t, hard, H, radius, weight, n_slots, (float4*)ell_out_dev, offsets ? grp_slot_off_dev : nullptr,
                       grp_weight_dev, robot_grp_off_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

// what the three round-table entry points require of the shape: the guided step indexes the table's (slot, t) words with an int
static int check_round_table(const char* who, int n_all, int robot0, int n_local, int horizon, int hard_slots) {
  MMD_REQUIRE(horizon == H, "%s: horizon must be %d", who, H);
  MMD_REQUIRE(hard_slots >= 1, "%s: hard_slots must be at least 1, got %d", who, hard_slots);
  MMD_REQUIRE(n_all >= 2 && n_local >= 1 && robot0 >= 0 && robot0 < n_all && n_local <= n_all - robot0, "%s: bad robot range", who);
  MMD_REQUIRE((long long)n_local * ((long long)hard_slots + n_all - 1) * H <= INT_MAX, "%s: a table of more than 2^31 - 1 points", who);
  return 0;
}

static int grid_for(size_t items) {
  const size_t g = (items + 255) / 256;
  return g > 2048 ? 2048 : (g < 1 ? 1 : (int)g);
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
  hipLaunchKernelGGL(round_soft_kernel, dim3(grid_for((size_t)n_local * (n_all - 1) * H)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)paths_dev, n_all, robot0, n_local, hard_slots, radius, (float4*)ell_dev);
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
  MMD_REQUIRE(n_local >= 1 && robot0 >= 0 && robot0 < n_all && n_local <= n_all - robot0, "%s: bad robot range", who);
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

int mmd_round_select(const float* paths_dev, const mmd_cons_bins* bins, const int32_t* robot_counts_dev, int n_local, int horizon,
                     float margin, int mode, int iters, int32_t* state_dev, int32_t* selected_dev, int32_t* perm_dev, int32_t* header_dev,
                     void* stream) {
  MMD_REQUIRE(paths_dev && robot_counts_dev && state_dev && selected_dev && perm_dev && header_dev, "mmd_round_select: NULL argument");
  MMD_REQUIRE(horizon == H, "mmd_round_select: horizon must be %d", H);
  MMD_REQUIRE(mode == MMD_REPLAN_CONFLICTED || mode == MMD_REPLAN_INDEPENDENT, "mmd_round_select: unknown mode %d", mode);
  MMD_REQUIRE(mode != MMD_REPLAN_INDEPENDENT || iters >= 1, "mmd_round_select: iters must be at least 1, got %d", iters);
  if (int rc = check_collision_bins("mmd_round_select", bins, margin)) return rc;
  MMD_REQUIRE(n_local >= 1 && n_local <= bins->n_all - bins->robot0, "mmd_round_select: bad robot range");
  hipStream_t st = (hipStream_t)stream;
  const int n_all = bins->n_all;
  int32_t* final_state = state_dev;
  if (mode == MMD_REPLAN_CONFLICTED) {
    hipLaunchKernelGGL(round_select_conflicted_kernel, dim3((n_all + 255) / 256), dim3(256), 0, st, robot_counts_dev, n_all, state_dev);
  } else {
    // iteration i reads what iteration i - 1 wrote: the two halves of state_dev in turn, the first from the counts alone
    const int32_t* old_state = nullptr;
    for (int i = 0; i < iters; ++i) {
      final_state = state_dev + (size_t)(i & 1) * n_all;
      hipLaunchKernelGGL(round_select_iter_kernel, dim3((n_all + 3) / 4), dim3(256), 0, st, (const float2*)paths_dev, *bins, margin,
                         robot_counts_dev, old_state, final_state);
      old_state = final_state;
    }
  }
  hipLaunchKernelGGL(round_select_partition_kernel, dim3(1), dim3(256), 0, st, final_state, n_all, bins->robot0, n_local, selected_dev,
                     perm_dev, header_dev);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
