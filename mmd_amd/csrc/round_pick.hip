// A planning round's pick in one native pass (include/mmd_amd.h: mmd_round_pick): what MultiRobotSampler.best_paths strings together from
// a handful of elementwise launches, mmd_postprocess_trajs, mmd_count_collisions, mmd_select_best and an index gather, as two kernels that
// read the sampling loop's NORMALISED samples -- so that the sampling loop can enqueue a stream chunk's pick on the chunk's own stream
// behind its last step (api.hip: mmd_p_sample_loop_pick).
//   * round_pick_sample_kernel: one wave per sample, lane = support point (four samples a workgroup).  Un-normalise with the clip, the map
//     and joint-limit check, path length and smoothness, the robot-robot collision count: each with the expressions of postprocess.hip /
//     multi_agent.hip (postprocess_dev.h, collision_dev.h) in their order, sums over the wave with the same butterfly.
//   * round_pick_robot_kernel: one wave per robot.  select_best_kernel's scan (postprocess_dev.h: wave_pick) over the robot's samples, then
//     the pick's positions, un-normalised again from the sample.
// Bitwise the results of the chain of calls (tests/test_gpu_round_pick.py), and held to its definition on the CPU (tests/round_pick_model.py)
// at every decision edge and pick size (tests/test_gpu_round_pick_edges.py).
#include "postprocess_dev.h"      // sets fp contract(off)
#include "collision_dev.h"        // torch_norm2
#include "clip_dev.h"             // clip_unit: torch.clip(v, -1, 1), a NaN passes through
#include "round_pick.h"

namespace mmd {

struct PickArgs {
  EnvDev env;
  UnnormArgs un;
  const float4* x;              // [n_robots * spr][H] normalised samples of the call
  const float2* paths;          // [n_all][H] or null
  int n_all, robot0, spr, n_interp;
  int traj0, n_traj;            // the samples of this launch
  float alpha[MAX_INTERP], one_minus_alpha[MAX_INTERP];
  float margin, q_min[2], q_max[2], rr_margin;
  float* key;                   // [n_robots * spr]: collision count, or path length + smoothness
  unsigned char* free_mask;     // [n_robots * spr]
  float2* paths_out;            // [n_robots][H]
  int* idx;                     // [n_robots]
  int* n_free;                  // [n_robots]
};

// MultiRobotSampler.unnormalize of one state
__device__ __forceinline__ float4 unnorm_clipped(const float4& v, const UnnormArgs& un) {
  return make_float4(unnorm_coord(clip_unit(v.x), un, 0), unnorm_coord(clip_unit(v.y), un, 1), unnorm_coord(clip_unit(v.z), un, 2),
                     unnorm_coord(clip_unit(v.w), un, 3));
}

__global__ __launch_bounds__(256) void round_pick_sample_kernel(PickArgs a) {
  const int t = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.n_traj) return;                              // (whole waves leave: no barrier below)
  const int traj = a.traj0 + w, robot = traj / a.spr;
  const float4 x = unnorm_clipped(a.x[(size_t)traj * H + t], a.un);
  const float nx = lane_next_f(x.x), ny = lane_next_f(x.y), nz = lane_next_f(x.z), nw = lane_next_f(x.w);
  // postprocess_kernel (K = 1, all_free = 0): the interpolated points of segment t -> t + 1 against the map, the support point against the limits
  const float4* grid = robot_grid(a.env, robot);
  bool coll = false;
  if (a.n_interp == 0) {
    coll = point_collides(a.env, grid, x.x, x.y, a.margin);
  } else if (t < H - 1) {
    for (int j = 0; j < a.n_interp; ++j) {
      const float px = interp_coord(x.x, nx, a.alpha[j], a.one_minus_alpha[j]);
      const float py = interp_coord(x.y, ny, a.alpha[j], a.one_minus_alpha[j]);
      const bool c = point_collides(a.env, grid, px, py, a.margin);
      coll = coll || c;
    }
  }
  const bool bad = coll || !inside_limits(x.x, x.y, a.q_min, a.q_max);
  const unsigned long long wave_bad = __ballot(bad);
  float key;
  if (a.paths) {
    // count_collisions_kernel: the other robots' points of time step t within the margin
    const int self = a.robot0 + robot;
    int c = 0;
    for (int j = 0; j < a.n_all; ++j) {
      if (j == self) continue;
      const float2 q = a.paths[(size_t)j * H + t];
      const float dx = x.x - q.x, dy = x.y - q.y;
      c += torch_norm2(dx, dy) < a.rr_margin ? 1 : 0;
    }
    key = (float)wave_sum(c);
  } else {
    float pl = 0.f, sm = 0.f;
    if (t < H - 1) segment_costs(x, nx, ny, nz, nw, pl, sm);
    // (postprocess_kernel adds its one wave's sums to 0.f before it stores them; select_best_kernel adds the two)
    pl = 0.f + wave_sum(pl);
    sm = 0.f + wave_sum(sm);
    key = pl + sm;
  }
  if (t == 0) {
    a.key[traj] = key;
    a.free_mask[traj] = wave_bad ? 0 : 1;
  }
}

__global__ __launch_bounds__(64) void round_pick_robot_kernel(PickArgs a, int robot_first) {
  const int r = robot_first + blockIdx.x, lane = threadIdx.x;
  const size_t base = (size_t)r * a.spr;
  int nf;
  const int best = wave_pick(a.spr, [&](int b) { return a.free_mask[base + b] != 0; }, [&](int b) { return a.key[base + b]; }, nf);
  if (best >= 0) {
    const float4 v = a.x[(base + best) * H + lane];
    a.paths_out[(size_t)r * H + lane] = make_float2(unnorm_coord(clip_unit(v.x), a.un, 0), unnorm_coord(clip_unit(v.y), a.un, 1));
  }
  if (lane == 0) {
    a.idx[r] = best;
    a.n_free[r] = nf;
  }
}

int round_pick_check(const char* who, const mmd_guide_desc* env, const mmd_round_pick* p, const float* x_dev, int n_robots, int samples_per_robot) {
  MMD_REQUIRE(env && p && x_dev, "%s: NULL argument", who);
  MMD_REQUIRE(n_robots >= 1 && samples_per_robot >= 1, "%s: empty batch", who);
  MMD_REQUIRE(p->paths_out_dev && p->idx_out_dev && p->n_free_out_dev && p->scratch_dev, "%s: mmd_round_pick without its outputs or scratch", who);
  MMD_REQUIRE(p->num_interpolation >= 0 && p->num_interpolation <= MAX_INTERP && (p->num_interpolation == 0 || p->alpha),
              "%s: 0 <= num_interpolation <= %d with its alpha table", who, MAX_INTERP);
  MMD_REQUIRE(!p->paths_all_dev || (p->robot0 >= 0 && p->n_all >= 1 && p->robot0 + n_robots <= p->n_all),
              "%s: robots [%d, %d) outside the %d paths", who, p->robot0, p->robot0 + n_robots, p->n_all);
  EnvDev e{};
  return fill_env(env, e);
}

int round_pick_launch(const mmd_guide_desc* env, const mmd_round_pick* p, const float* x_dev, int n_robots, int robot_first, int n,
                      int samples_per_robot, hipStream_t st) {
  PickArgs a{};
  if (int rc = fill_env(env, a.env)) return rc;
  for (int d = 0; d < 4; ++d) { a.un.mins[d] = p->norm_min[d]; a.un.range[d] = p->norm_max[d] - p->norm_min[d]; }
  a.x = reinterpret_cast<const float4*>(x_dev);
  a.paths = reinterpret_cast<const float2*>(p->paths_all_dev);
  a.n_all = p->n_all; a.robot0 = p->robot0; a.spr = samples_per_robot; a.n_interp = p->num_interpolation;
  a.traj0 = robot_first * samples_per_robot; a.n_traj = n * samples_per_robot;
  for (int j = 0; j < p->num_interpolation; ++j) {
    a.alpha[j] = p->alpha[j];
    a.one_minus_alpha[j] = 1.f - p->alpha[j];        // torch: (1 - alpha) in fp32
  }
  a.margin = p->margin; a.rr_margin = p->rr_margin;
  for (int k = 0; k < 2; ++k) { a.q_min[k] = p->q_min[k]; a.q_max[k] = p->q_max[k]; }
  // scratch: [keys of all the call's samples][their free flags]
  a.key = reinterpret_cast<float*>(p->scratch_dev);
  a.free_mask = reinterpret_cast<unsigned char*>(a.key + (size_t)n_robots * samples_per_robot);
  a.paths_out = reinterpret_cast<float2*>(p->paths_out_dev);
  a.idx = p->idx_out_dev; a.n_free = p->n_free_out_dev;
  hipLaunchKernelGGL(round_pick_sample_kernel, dim3((a.n_traj + 3) / 4), dim3(256), 0, st, a);
  hipLaunchKernelGGL(round_pick_robot_kernel, dim3(n), dim3(64), 0, st, a, robot_first);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace mmd

using namespace mmd;

extern "C" {

int mmd_round_pick_paths(const mmd_guide_desc* env, const mmd_round_pick* pick, const float* x_dev, int n_robots, int samples_per_robot,
                         void* stream) {
  if (int rc = round_pick_check("mmd_round_pick_paths", env, pick, x_dev, n_robots, samples_per_robot)) return rc;
  return round_pick_launch(env, pick, x_dev, n_robots, 0, n_robots, samples_per_robot, (hipStream_t)stream);
}

}  // extern "C"
