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
//   * which robots a round re-plans (mmd_round_select): the robots in conflict, or an independent set of the conflict graph found by
//     priority propagation on the same cell table -- CBS re-plans one agent of a conflict against the others' fixed paths (cbs.py:316-324);
//     a round does that for every robot of the set at once -- and the stable partition that makes the selected robots a prefix.
// The guided step's other tables are built in cons_tables.hip: only mmd_path_constraints is here, with the mmd_agent_path states it reads.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mmd_amd.h"
#include "bins_dev.h"             // own_cell_list / check_collision_bins: the cell table built in cons_tables.hip
#include "collision_dev.h"        // torch_norm2 / rr_hit: the pinned fp32 form of the collision decision (sets fp contract(off))
#include "common.h"
#include "cons_table_dev.h"       // slot_word / empty_word / one_group_per_robot / check_robot_range: what every ELL table builder shares
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
  if (t == 0 && grp_slot_off) one_group_per_robot(0, 1, n_slots, weight, grp_slot_off, grp_weight, robot_grp_off);
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
      ell[(size_t)fill * horizon + t] = slot_word(p.x, p.y, radius);
      ++fill;
    }
  }
  for (; fill < n_slots; ++fill) ell[(size_t)fill * horizon + t] = empty_word();
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

int mmd_round_select(const float* paths_dev, const mmd_cons_bins* bins, const int32_t* robot_counts_dev, int n_local, int horizon,
                     float margin, int mode, int iters, int32_t* state_dev, int32_t* selected_dev, int32_t* perm_dev, int32_t* header_dev,
                     void* stream) {
  MMD_REQUIRE(paths_dev && robot_counts_dev && state_dev && selected_dev && perm_dev && header_dev, "mmd_round_select: NULL argument");
  MMD_REQUIRE(horizon == H, "mmd_round_select: horizon must be %d", H);
  MMD_REQUIRE(mode == MMD_REPLAN_CONFLICTED || mode == MMD_REPLAN_INDEPENDENT, "mmd_round_select: unknown mode %d", mode);
  MMD_REQUIRE(mode != MMD_REPLAN_INDEPENDENT || iters >= 1, "mmd_round_select: iters must be at least 1, got %d", iters);
  if (int rc = check_collision_bins("mmd_round_select", bins, margin)) return rc;
  if (int rc = check_robot_range("mmd_round_select", bins->n_all, bins->robot0, n_local)) return rc;
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
