/*
 * mmd_amd.h -- C ABI of libmmd_amd.so: the MI355X (gfx950) guided-diffusion trajectory sampler that drops in
 * behind yoraish/mmd's MPD / MPDEnsemble planners.
 *
 * The reference has no FFI layer (it is pure Python); the boundary a maintainer would bind is the
 * "inner" call contract of the planner.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference checkout).  All pointers suffixed _dev are device (HIP) pointers to contiguous
 * fp32 / int32 data; everything else is host memory.  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Every function returns 0 on success and a non-zero code on failure; mmd_last_error() gives the text.
 * No global state besides the last-error string (thread-local) and lazily created per-(thread, device) side streams;
 * handles are immutable after creation, so entry points are re-entrant per (handle, stream).  The library never reads the
 * environment: every switch, measurement ones included, is a field of a descriptor passed with the call (mmd_unet_options,
 * mmd_sampler_desc.flags / .n_streams / .guide_coop_max).
 *
 * Trajectory tensors are [n_traj, H, D] fp32 with D = 4 (x, y, vx, vy) and H = 64 support points, in the
 * NORMALISED space of the diffusion model; n_traj = n_robots * samples_per_robot, robot-major.
 */
#ifndef MMD_AMD_H
#define MMD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMD_AMD_ABI_VERSION 9
#define MMD_STATE_DIM 4
#define MMD_HORIZON 64

typedef struct mmd_unet_s* mmd_unet_t; /* opaque: packed TemporalUnet weights + time-embedding table on device */

int mmd_abi_version(void);
const char* mmd_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * TemporalUnet  (replaces mmd/models/diffusion_models/temporal_unet.py:23-174 `TemporalUnet.__init__/forward`,
 * layers mmd/models/layers/layers.py:232-358)
 * ---------------------------------------------------------------------------------------------------------- */

/* Number of parameter tensors, and the element count of tensor i, in the reference's state_dict order for
 * TemporalUnet(state_dim=4, n_support_points=64, unet_input_dim, dim_mults=(1, 2, 4, 8)[:n_levels]).
 * unet_input_dim: a multiple of 8 in [8, 64]; n_levels 1 .. 4 (UNET_DIM_MULTS, mmd/models/__init__.py:8-11: option 0 =
 * 3 levels, option 1 = 4 levels); anything else returns -1.  unet_input_dim == 32 with 3 levels (the released checkpoints)
 * runs the fused one-launch kernel, every other shape the layer-by-layer kernels (csrc/unet_layers.hip). */
int mmd_unet_num_tensors(int unet_input_dim, int n_levels);
int64_t mmd_unet_tensor_numel(int unet_input_dim, int n_levels, int index);

/* Build the device-side model from HOST fp32 tensors given in state_dict order (the values of
 * `{k: v for k, v in diffusion_model.state_dict().items() if k.startswith('model.')}`; replaces
 * `diffusion_model.load_state_dict(...)`, mmd/planners/single_agent/mpd.py:167-172).  `numels[i]` is checked
 * against mmd_unet_tensor_numel.  Also precomputes, on the GPU, the time-embedding projections of every integer
 * diffusion step t in [0, n_diffusion_steps) (TimeEncoder + the 12 cond_mlp heads; t is identical across the
 * batch, mmd/models/diffusion_models/diffusion_model_base.py:27-29). */
typedef struct mmd_unet_options {     /* creation-time choices, fixed for the life of the handle.  NULL = every default.  An all-zero
                                       * struct is the defaults EXCEPT rtb_fused: 0 there selects "no fused block"; pass a negative
                                       * rtb_fused (or NULL) for its default */
  uint32_t flags;                     /* MMD_UNET_* below */
  int32_t rtb_fused;                  /* layer-by-layer path, A/B: the widest ResidualTemporalBlock run as ONE launch (channels);
                                       * 0 = none, < 0 = default (64) */
  int32_t mconv_max_cs;               /* layer-by-layer path, A/B: the widest column slice of its matrix-pipe kernel; 0 = default (128) */
  int32_t two_per_workgroup_max;      /* fused kernel, A/B: batches up to this size run two trajectories per workgroup; 0 = default
                                       * (512), < 0 = never */
  int32_t precision;                  /* MMD_UNET_PRECISION_* below; anything else is an error, and so is F16 on the layer-by-layer path
                                       * (a non-fused shape, MMD_UNET_LAYERED) */
} mmd_unet_options;
#define MMD_UNET_PRECISION_F32 0      /* the default: fp32-accurate convs (two fp16 pieces per operand, three MFMAs per product) */
#define MMD_UNET_PRECISION_F16 1      /* opt-in mixed precision of the fused kernel: conv inputs and weights rounded to ONE fp16 piece under
                                       * the same power-of-two scales, fp32 accumulation, GroupNorm / Mish / the sampler step in fp32.
                                       * ~1e-3 relative to the fp32 forward (outside the 1e-3-per-step parity bar).  Fixed for the life of
                                       * the handle: every entry point that takes the handle follows it */
#define MMD_UNET_LAYERED 1u           /* the layer-by-layer kernels for the fused kernel's own configuration too (the two
                                       * implementations share no device code: tests hold one against the other) */
#define MMD_UNET_LAYERED_VALU 2u      /* layer-by-layer path: every layer on the vector-ALU kernels (A/B of its matrix-pipe kernel) */

int mmd_unet_create(mmd_unet_t* out, int unet_input_dim, int n_levels, int n_diffusion_steps,
                    const float* const* tensors, const int64_t* numels, int n_tensors, const mmd_unet_options* options,
                    void* stream);
int mmd_unet_destroy(mmd_unet_t unet);

/* Scratch needed by mmd_unet_forward for n_traj trajectories; allocate it with the host framework.  (The fused kernel keeps
 * every activation on chip: 12 KiB, the step table + argument block of a persistent run of unguided steps in mmd_p_sample_loop;
 * the layer-by-layer path keeps (5 + n_levels) tensors of n_traj x 64 x unet_input_dim floats there.) */
size_t mmd_unet_workspace_bytes(mmd_unet_t unet, int n_traj);

/* eps = model(x, t, context=None)  (temporal_unet.py:121; called from p_mean_variance,
 * diffusion_model_base.py:152).  t is one integer for the whole batch. */
int mmd_unet_forward(mmd_unet_t unet, const float* x_dev, int t, float* eps_dev, int n_traj, void* workspace_dev,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Guide  (replaces GuideManagerTrajectoriesWithVelocity.forward, mmd/models/diffusion_models/guides.py:180-226,
 * with the cost terms of deps/motion_planning_baselines/mp_baselines/planners/costs/cost_functions.py:149-193,
 * :275-326, :505-542 and the SDF fields of deps/torch_robotics/.../distance_fields.py:333-367,
 * environments/grid_map_sdf.py:84-114)
 * ---------------------------------------------------------------------------------------------------------- */

/* The inter-robot soft constraints of a many-robot round as a CELL table (the alternative to the all-pairs ELL table of
 * mmd_soft_constraints_from_paths, whose N - 1 slots per robot make a round's constraint work and memory grow with N^2): for every time
 * step t and cell c of an nx x ny grid over the map, the robots whose best-path point at t lies in the 3 x 3 cells around c, in ascending
 * robot id.  A point acts on a trajectory point only within `radius`, and a cell is at least (1 + 1/16) x radius wide, so the list of a
 * trajectory point's own cell holds every robot that can act on it -- 10 to 20 candidates where the all-pairs table has N - 1 slots -- and
 * the guided step on this table returns the SAME BITS as on the all-pairs table of the same paths.  One table serves every robot of a
 * GPU: the step skips the entry of the trajectory's own robot, robot0 + its index in the call.  Fill the two arrays with
 * mmd_bin_constraints_from_paths and hand the struct over in mmd_guide_desc.cons_bins. */
typedef struct mmd_cons_bins {
  float lo[2], inv_cell[2];          /* cell index = clamp((int)floorf((p - lo) * inv_cell), 0, n - 1), per axis, in fp32; cell =
                                      * ix * ny + iy.  lo = the limits mmd_bin_constraints_from_paths was given, inv_cell[k] = the fp32
                                      * quotient (float)n[k] / (hi[k] - lo[k]) */
  int32_t nx, ny, n_all, robot0;     /* the grid, the number of robots in the table, the GLOBAL id of the call's first robot */
  float radius, weight;              /* one radius for every point (as tables from mmd_soft_constraints_from_paths have), and the
                                      * weight of the one constraint group every robot has */
  const int32_t* cell_off_dev;       /* [H][nx * ny + 1]: list of (t, c) = entries [off[t][c], off[t][c + 1]) of time step t's segment */
  const float* entries_dev;          /* [H][9 * n_all][4]: (qx, qy, bit pattern of the GLOBAL robot id, 0); a point is in at most 9
                                      * lists, so a segment of 9 * n_all entries always fits */
} mmd_cons_bins;

typedef struct mmd_guide_desc {
  /* LimitsNormalizer (mmd/datasets/normalization.py:145-168): x_u = (clip(x,-1,1)+1)/2*(max-min)+min.
   * The clip is applied unconditionally (the reference clips only if the batch leaves [-1-1e-4, 1+1e-4]). */
  float norm_min[MMD_STATE_DIM];
  float norm_max[MMD_STATE_DIM];
  /* SDF grids of the fixed objects: GridMapSDF (grid_map_sdf.py:9-114).  Cell (ix,iy) holds float4
   * (sdf, d sdf/dx, d sdf/dy, 0); layout [n_maps][n_grids][nx][ny][4]; index = floor((p-lo)/(hi-lo)*n) clamped.
   * n_grids == 0 declares an obstacle-free map (EnvEmpty2D: sdf == 1, primitives.py:109-110): no gather is issued. */
  float limits_lo[2];
  float limits_hi[2];
  int32_t grid_nx, grid_ny, n_grids, n_maps;
  const float* sdf_grids_dev;
  const int32_t* robot_map_dev;      /* [n_robots] map index per robot, or NULL (all robots use map 0) */
  /* workspace boundaries (tasks.py:75-86, already scaled by 1.08) */
  float ws_min[2];
  float ws_max[2];
  float margin;                      /* 1.1 * robot radius + obstacle cutoff margin (distance_fields.py:117) */
  float dt;                          /* trajectory_duration / n_support_points (mpd.py:140) */
  float sigma_gp;                    /* 1.0 (mpd.py:237) */
  float weight_collision;            /* weight_grad_cost_collision  (mmd_params.py:40) */
  float weight_smoothness;           /* weight_grad_cost_smoothness (mmd_params.py:41) */
  float max_grad_norm;               /* 1.0 (guides.py:154) */
  /* Constraints: one group per CostConstraint (= per MultiPointConstraint, mmd/common/constraints.py:46-85),
   * stored time-bucketed (ELL): slot j of a group holds, for every time step t, at most one active point
   * float4 (qx, qy, radius, radius * |radius|) with radius < 0 meaning "no point".  cons_ell_dev is [n_slots][H][4];
   * group g owns slots [grp_slot_off[g], grp_slot_off[g+1]); robot r owns groups
   * [robot_grp_off[r], robot_grp_off[r+1]).  Build it with mmd_pack_constraints or
   * mmd_soft_constraints_from_paths.  NULL pointers = no constraints. */
  const float* cons_ell_dev;
  const int32_t* grp_slot_off_dev;
  const float* grp_weight_dev;
  const int32_t* robot_grp_off_dev;
  int32_t max_slots_per_robot;       /* max over robots of their total slot count (sizes the LDS staging; 0 = unknown) */
  float cons_uniform_radius;         /* > 0: every active point of the table has exactly this radius (tables made by
                                      * mmd_soft_constraints_from_paths): the kernel then keeps only (qx, qy) on chip,
                                      * twice the slots per workgroup.  0 = radii vary, general path. */
  /* Extra objects of the environment (EnvBase.obj_extra_list, env_base.py:76-89: an ObjectField of primitive fields at the
   * identity pose), evaluated ANALYTICALLY as the reference does -- one more signed-distance field next to the grids of the
   * fixed objects (df_obj_l = [grid, *obj_extra_list]; cost = max over the fields, distance_fields.py:110-126): spheres
   * |p - c| - r (MultiSphereField, primitives.py:108-115), boxes as the rounded box of the fixed objects (MultiBoxField --
   * an ALIAS of MultiRoundedBoxField, primitives.py:345 -- i.e. primitives.py:326-333: corner radius 0.15 x the smaller size), minimum over all of them.  n = 0 / NULL: the env has none (every shipped map: an empty sphere list, sdf = 1). */
  const float* extra_spheres_dev;    /* [n_extra_spheres][4]: (cx, cy, r, 0) */
  const float* extra_boxes_dev;      /* [n_extra_boxes][4]: (cx, cy, half size x, half size y) */
  int32_t n_extra_spheres, n_extra_boxes;
  /* GuideManager.clip_gradient (guides.py:228-259), applied to every cost's per-point gradient: 0 = clip_grad_by_norm with
   * max_grad_norm (what MPD / MPDEnsemble set, mpd.py:258-265), 1 = clip_grad_by_value: torch.clip(grad, -max_grad_value,
   * max_grad_value) (the class default 0.1), 2 = clip_grad = False */
  int32_t clip_grad_rule;
  float max_grad_value;
  /* The inter-robot constraints as a cell table (above) instead of the ELL table, or NULL: every guided step of mmd_guide_steps,
   * mmd_ddpm_step, mmd_p_sample_loop, mmd_ddim_sample and mmd_p_sample_loop_ensemble then runs the binned step kernel, at every launch
   * size.  Each robot has exactly one constraint group, of weight cons_bins->weight.  Errors: together with cons_ell_dev, with
   * mmd_sampler_desc.robot_seeds_dev, or in a call of mmd_debug_ddpm_step_trace. */
  const mmd_cons_bins* cons_bins;
} mmd_guide_desc;

/* Host helper: time-bucket one robot's constraint groups.  For group g (n_pts[g] points): q [n,2], t_range [n,2]
 * as [t0, t1) (exclusive end, cost_functions.py:305), radius [n].  Writes the ELL block into `ell_out`
 * ([max_slots][H][4], host) and returns the number of slots used by each group in slots_out[g]; returns an error
 * if max_slots is too small.  With ell_out == NULL only slots_out is filled (sizing pass).  (Replaces the per-call CostConstraint construction, mpd.py:329-342.) */
int mmd_pack_constraints(int n_groups, const int32_t* n_pts, const float* const* q, const float* const* t_range,
                         const float* const* radius, int horizon, float* ell_out, int max_slots,
                         int32_t* slots_out);

/* Device helper: all-pairs soft constraints from the robots' current best paths (replaces
 * CBS.create_soft_constraints_from_other_agents_paths, mmd/planners/multi_agent/cbs.py:468-508, for equal start
 * times).  paths_dev [n_all, H, 2] un-normalised positions of ALL robots (after the all-gather); this rank owns
 * robots [robot0, robot0 + n_local).  Writes one group of (n_all-1) slots per local robot into ell_out_dev
 * ([n_local*(n_all-1)][H][4]) plus the three offset/weight arrays (sizes n_local+1, n_local, n_local+1). */
int mmd_soft_constraints_from_paths(const float* paths_dev, int n_all, int robot0, int n_local, int horizon,
                                    float radius, float weight, float* ell_out_dev, int32_t* grp_slot_off_dev,
                                    float* grp_weight_dev, int32_t* robot_grp_off_dev, void* stream);

/* Device helper: the cell table of mmd_cons_bins from the same paths_dev [n_all, H, 2] (equal start times; time step 0 carries no
 * constraint: empty lists, as the all-pairs table has no active point there).  lo / hi: the map's limits (host, [2]); points outside them
 * go to the border cells.  nx, ny in [1, 64] with (hi - lo) / n >= (1 + 1/16) * radius on both axes (smaller cells are an error: a list
 * could then miss an acting robot); n_all in [2, 4096].  mmd_cons_bins_bytes gives the sizes of the two arrays (and returns their sum).
 * One launch on `stream`, one workgroup per time step, no atomics and no host synchronisation: the lists are deterministic. */
size_t mmd_cons_bins_bytes(int n_all, int nx, int ny, size_t* off_bytes, size_t* entry_bytes);
int mmd_bin_constraints_from_paths(const float* paths_dev, int n_all, int horizon, float radius, const float lo[2], const float hi[2],
                                   int nx, int ny, int32_t* cell_off_dev, float* entries_dev, void* stream);

/* The same table with a choice of the first listed time step: mmd_bin_constraints_from_paths is the first_step = 1 call (bit for bit).
 * first_step = 0 also lists time step 0 -- a COLLISION table, for mmd_count_collisions_binned and mmd_path_conflicts_binned below, which
 * count collisions at t = 0 as the all-pairs kernels do; `reach` = the largest distance at which the table's walkers may need a point
 * (mmd_cons_bins.radius; a collision table of reach = the constraint radius shares the constraint table's grid).  Time steps below
 * first_step get empty lists; first_step outside {0, 1} is an error.  Same checks, sizes (mmd_cons_bins_bytes), cell rule
 * ((hi - lo) / n >= (1 + 1/16) * reach) and kernel.  The struct does not record first_step: hand a guided step only tables of
 * first_step = 1 (its bits are promised on those), the two collision calls only tables of first_step = 0. */
int mmd_bin_paths(const float* paths_dev, int n_all, int horizon, float reach, const float lo[2], const float hi[2], int nx, int ny,
                  int first_step, int32_t* cell_off_dev, float* entries_dev, void* stream);

/* n_steps x { x += guide(x); apply_hard_conditioning }  (guide_gradient_steps,
 * mmd/models/diffusion_models/sample_functions.py:89-107).  Hard conditions (apply_hard_conditioning,
 * sample_functions.py:8-14: the dict {support point: state}): bit t of hard_rows set = support point t of every trajectory
 * is pinned; hard_dev [n_robots][popcount(hard_rows)][4] holds each robot's pinned states in ascending row order
 * (MPD's {0: start, H-1: goal} = hard_rows 0x8000000000000001, hard_dev [n_robots][2][4]).  chain_dev, if not NULL,
 * receives the state after EVERY iteration, [n_steps][n_traj, H, 4] (the post-diffusion guide steps of planner_alg
 * 'diffusion_prior_then_guide', mmd/planners/single_agent/mpd.py:429-453, in one launch). */
int mmd_guide_steps(const mmd_guide_desc* g, float* x_dev, const float* hard_dev, uint64_t hard_rows, int n_robots,
                    int samples_per_robot, int n_steps, float* chain_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * DDPM sampling  (replaces ddpm_sample_fn, sample_functions.py:40-86, and GaussianDiffusionModel.p_sample_loop /
 * run_inference / run_local_inference, diffusion_model_base.py:162-211, :320-421)
 * ---------------------------------------------------------------------------------------------------------- */

typedef struct mmd_sampler_desc {
  int32_t n_diffusion_steps;                /* T of the schedule tables */
  /* [T] host tables (GaussianDiffusionModel buffers, diffusion_model_base.py:83-105) */
  const float* sqrt_recip_alphas_cumprod;
  const float* sqrt_recipm1_alphas_cumprod;
  const float* posterior_mean_coef1;
  const float* posterior_mean_coef2;
  const float* posterior_log_variance_clipped;
  int32_t n_guide_steps;                    /* 20 (mmd_params.py:38) */
  int32_t t_start_guide;                    /* guide iff loop index i < t_start_guide (sample_functions.py:63) */
  float noise_std_extra;                    /* 0.5 (mpd.py:303) */
  uint64_t hard_rows;                       /* as in mmd_guide_steps */
  int32_t n_streams;                        /* mmd_p_sample_loop splits the robots into this many concurrent HIP
                                             * streams (forked from / joined to `stream`) so one chunk's staging and
                                             * epilogues overlap the other's MFMA phases; 0 = auto (2 above 512
                                             * trajectories, else 1), 1 = off */
  int64_t traj_index_base;                  /* GLOBAL index of this call's trajectory 0 (= first global robot * samples per
                                             * robot).  The in-kernel Philox4x32-10 draws are keyed by (seed, draw, global
                                             * trajectory * H + t), so a rank that samples robots [r0, r1) of an N-robot
                                             * instance draws exactly the noise those rows get in the unsharded call
                                             * (per-robot outputs bitwise identical for G = 1, 2, 4, 8).
                                             * Counter layout: with point = global trajectory * H + t, the 128-bit counter is
                                             * (point & 0xFFFFFFFF, draw, point >> 32, 0) and the key (seed & 0xFFFFFFFF, seed >> 32);
                                             * the four output words give four N(0,1) values by Box-Muller (words 0, 1 -> radius,
                                             * angle of the first pair, words 2, 3 of the second).  Draws: mmd_p_sample_loop numbers
                                             * its steps k = 0, 1, ... in loop order, mmd_ddpm_step uses the caller's draw_index;
                                             * 0xFFFFFFFF is RESERVED for x_T and 0xFFFFFFFE for mmd_q_sample (the Python layer
                                             * passes it): a step must not draw under either */
  const float* noise_std_extra_by_t;        /* optional [T] host table: noise_std_extra_schedule_fn(t) evaluated for every
                                             * t (sample_functions.py:83-86 calls it per step); NULL = the constant above */
  void* profiler;                           /* optional mmd_profiler_t (include/mmd_amd_debug.h) that brackets UNet launches
                                             * with HIP events; NULL in production */
  int32_t scale_grad_by_std;                /* 1: every guide gradient is multiplied by model_var = exp(posterior_log_variance_
                                             * clipped[t]) before it is added (guide_gradient_steps, sample_functions.py:100-101) */
  int32_t model_predicts_x0;                /* 1: GaussianDiffusionModel(predict_epsilon=False): the network output IS x_recon
                                             * (predict_start_from_noise / predict_noise_from_start, diffusion_model_base.py:114-141) */
  uint32_t flags;                           /* MMD_SAMPLER_* below (measurement switches; 0 in production) */
  int32_t guide_coop_max;                   /* A/B: a guided step of up to this many trajectories per launch runs four waves per
                                             * trajectory; 0 = default (512), < 0 = never */
  const uint64_t* robot_seeds_dev;          /* optional DEVICE array [n_robots]: one Philox stream per ROBOT -- robot r's draws are
                                             * keyed by (robot_seeds[r], draw, index within the robot * H + t) and `seed` /
                                             * traj_index_base are ignored.  R independent planner calls (cbs.py:316-324,
                                             * inference_multi_agent.py:225-237: one MPD call per agent) batched into ONE launch
                                             * sequence then draw exactly the noise of the R separate calls with those seeds.
                                             * NULL = one stream per call */
} mmd_sampler_desc;
#define MMD_SAMPLER_NO_FUSED_STEP 1u        /* unguided steps as separate step-kernel launches instead of the UNet launch's tail */
#define MMD_SAMPLER_PERSIST 2u              /* the leading run of unguided steps of mmd_p_sample_loop as persistent launches (<= 64
                                             * steps each; the first 12 KiB of the workspace then hold the step table) */

/* Scratch needed by mmd_ddpm_step / mmd_p_sample_loop: [mmd_unet_workspace_bytes][eps: n_traj * H * 4 floats].  The chunked
 * (n_streams > 1) loop uses slices of the same eps block, so this size is exact for every n_streams. */
size_t mmd_sampler_workspace_bytes(mmd_unet_t unet, int n_traj);

/* One ddpm_sample_fn call + the apply_hard_conditioning that follows it in p_sample_loop
 * (diffusion_model_base.py:199-203): x <- step(x) for loop index i (i < 0 means t = 0, no noise).
 * guide may be NULL (no guidance).  noise_dev [n_traj,H,4] is the injected randn_like draw, or NULL to draw it
 * in-kernel from Philox4x32-10 keyed by (seed, draw_index).
 * Non-finite values: the x0 clamp is x_recon.clamp_(-1., 1.) (diffusion_model_base.py:155) -- a NaN x0 (a NaN network output, or
 * 0 * inf) stays NaN, +-inf goes to the bound; a trajectory whose forward is NaN stays NaN in every row that is not pinned, in this
 * call and in every sampling loop (the step in the UNet launch's tail included), and is for the pick to discard. */
int mmd_ddpm_step(mmd_unet_t unet, const mmd_sampler_desc* s, const mmd_guide_desc* guide, float* x_dev,
                  const float* hard_dev, int n_robots, int samples_per_robot, int i, const float* noise_dev,
                  uint64_t seed, uint32_t draw_index, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The whole loop: for i = n_steps-1 ... -n_steps_without_noise.  x_dev holds x_T (or the warm start; NULL noise
 * + init_noise != 0 draws x_T in-kernel) on entry and the final sample on exit.  chain_dev, if not NULL, receives
 * [n_steps + n_steps_without_noise + 1][n_traj,H,4] (chain[0] = conditioned x_T).  step_noise_dev, if not NULL, is
 * [n_steps + n_steps_without_noise][n_traj,H,4] injected draws in loop order. */
int mmd_p_sample_loop(mmd_unet_t unet, const mmd_sampler_desc* s, const mmd_guide_desc* guide, float* x_dev,
                      const float* hard_dev, int n_robots, int samples_per_robot, int n_steps,
                      int n_steps_without_noise, int init_noise, const float* step_noise_dev, uint64_t seed,
                      float* chain_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* GaussianDiffusionModel.ddim_sample (diffusion_model_base.py:213-290) with eta = 0: x_T (drawn with Philox when
 * init_noise != 0, else the contents of x_dev) -> conditioned -> one step per consecutive pair (times[k], times[k+1]) of
 * the host array `times` ([n_times], strictly decreasing, as the reference builds it: reversed int(linspace(0, T-1,
 * T/5 + 1)) followed by -1): eps = model(x, times[k]); x_start = predict_start_from_noise (not clamped);
 * x = x_start sqrt(acp[t_next]) + sqrt(1 - acp[t_next]) eps; s->n_guide_steps guide steps iff a guide is given and
 * t_next < s->t_start_guide (the reference effectively runs ONE: it does not forward n_guide_steps to
 * guide_gradient_steps); hard conditioning; on the pair that ends in -1, x = x_start.  alphas_cumprod is the host [T]
 * buffer of that name.  chain_dev: [n_times][n_traj, H, 4] or NULL. */
int mmd_ddim_sample(mmd_unet_t unet, const mmd_sampler_desc* s, const float* alphas_cumprod, const int32_t* times,
                    int n_times, const mmd_guide_desc* guide, float* x_dev, const float* hard_dev, int n_robots,
                    int samples_per_robot, int init_noise, uint64_t seed, float* chain_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);

/* q_sample (diffusion_model_base.py:425-433): x = a * x_start + b * noise (noise injected or Philox keyed by
 * traj_index_base like the sampler).  n_traj counts blocks of H = 64 support points: a [B, K*64, 4] ensemble seed
 * (diffusion_ensemble.py:279-281) is n_traj = B * K. */
int mmd_q_sample(float* x_dev, const float* x_start_dev, const float* noise_dev, float sqrt_alphas_cumprod_t,
                 float sqrt_one_minus_alphas_cumprod_t, uint64_t seed, uint32_t draw_index, int64_t traj_index_base,
                 int n_traj, void* stream);

/* apply_cross_conditioning for one (m1, m2) tile pair (sample_functions.py:17-31): row ind1 of x1 := min(row ind2
 * of x2 + rel, boundary); then row ind2 of x2 := max(row ind1 of x1 - rel, -boundary); rel / boundary are [4] host.
 * min / max are torch.min / torch.max: a NaN in the stitch row is NaN in both tiles afterwards, never the boundary. */
int mmd_cross_condition(float* x1_dev, float* x2_dev, int ind1, int ind2, const float* rel, const float* boundary,
                        int n_traj, void* stream);

/* DiffusionsEnsemble.p_sample_loop (mmd/models/diffusion_models/diffusion_ensemble.py:55-106): K tile models chained
 * along the horizon.  Per outer step the tiles step IN ORDER (UNet + fused DDPM/guide kernel of tile m on its own
 * x_dev), each followed by apply_cross_conditioning over all (m1, m2) pairs (sample_functions.py:17-31) -- the whole
 * loop is enqueued by this ONE call (no per-step host round trip).  Every tile has its own model handle, sampler
 * (schedule, guide-step counts, hard mask, Philox seed via `seed` or sampler->robot_seeds_dev), guide, state, chain and injected-noise buffers; all
 * tiles share n_robots / samples_per_robot and the workspace (sized by mmd_sampler_workspace_bytes of the largest). */
typedef struct mmd_ensemble_tile {
  mmd_unet_t unet;
  const mmd_sampler_desc* sampler;
  const mmd_guide_desc* guide;       /* or NULL */
  float* x_dev;                      /* [n_traj, H, 4]: x_T / warm start on entry (init_noise != 0: drawn), result on exit */
  const float* hard_dev;             /* [n_robots][2][4] */
  const float* step_noise_dev;       /* [n_steps + n_steps_without_noise][n_traj, H, 4] injected draws, or NULL */
  float* chain_dev;                  /* [n_steps + n_steps_without_noise + 1][n_traj, H, 4], or NULL.  Rows as the reference's
                                        chains hold them (it stores the tensor object and stitches in place,
                                        diffusion_ensemble.py:86-103): row k of tile m >= 1 also carries the boundary rows stitched
                                        after the earlier tiles' steps of outer step k + 1; the last row is the result */
  uint64_t seed;
} mmd_ensemble_tile;

typedef struct mmd_cross_cond {
  int32_t m1, m2, ind1, ind2;        /* row ind1 of tile m1 is stitched to row ind2 of tile m2 */
  float rel[4];                      /* transforms[m2] - transforms[m1], zero padded to the state dim */
  float boundary[4];                 /* rel / ||rel|| with zeros replaced by 1e6 */
  const float* by_robot_dev;         /* optional DEVICE table [n_robots][2][4] = (rel, boundary) per robot, replacing the two above:
                                        batched planner calls whose robots traverse different tile skeletons
                                        (inference_multi_agent.py:418-431: [[0,0],[0,1]] and [[0,1],[0,0]]); NULL = one pair */
} mmd_cross_cond;

int mmd_p_sample_loop_ensemble(const mmd_ensemble_tile* tiles, int n_tiles, const mmd_cross_cond* cross, int n_cross,
                               int n_robots, int samples_per_robot, int n_steps, int n_steps_without_noise,
                               int init_noise, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-agent layer next to the sampler
 * ---------------------------------------------------------------------------------------------------------- */

/* RobotPlanarDisk.check_rr_collisions (deps/torch_robotics/torch_robotics/robots/robot_planar_disk.py:173-203) as
 * CBS.get_conflicts calls it (mmd/planners/multi_agent/cbs.py:185-190, equal start times, densification 1):
 * mask_dev [T][N][N] uint8 = (||p_i(t) - p_j(t)|| < margin) && i != j; midpoints_dev [T][N][N][2] = (p_i + p_j)/2 or
 * NaN where there is no collision (may be NULL).  paths_dev [N,T,2] un-normalised positions, T = `horizon` >= 1 (T = 1:
 * the start / goal validity check of mmd/common/multi_agent_utils.py:74-79); margin = 2.1 * radius. */
int mmd_rr_collisions(const float* paths_dev, int n_robots, int horizon, float margin, uint8_t* mask_dev,
                      float* midpoints_dev, void* stream);

/* The 'least_collisions' scan of CBS.expand (cbs.py:446-458) without the per-sample get_conflicts loop:
 * counts_dev[r*B + b] = #{(t, j != robot0 + r) : ||x_{r,b}(t) - p_j(t)|| < margin} for the local robots' sample
 * batches trajs_dev [n_local*B, H, 4] (un-normalised; only x, y are read) against ALL robots' best paths
 * paths_dev [n_all, H, 2].  (The reference's conflict count for sample b is a constant plus twice this number.) */
int mmd_count_collisions(const float* trajs_dev, const float* paths_dev, int robot0, int n_local,
                         int samples_per_robot, int n_all, int horizon, float margin, int32_t* counts_dev, void* stream);

/* mmd_count_collisions on a cell table of the best paths (mmd_bin_paths, first_step = 0) instead of the paths: every (sample, t) point
 * meets only the robots in the list of its own cell instead of all n_all, and the counts are the SAME INTEGERS.  trajs_dev
 * [n_local * B, H, 4] as above; the local robots are [bins->robot0, bins->robot0 + n_local) and a trajectory skips the entry of its own
 * robot.  margin <= bins->radius is what makes a cell's list complete (csrc/multi_agent.hip, COVER); a larger margin, a NULL table, or a
 * grid / robot range a guided step would refuse are error returns before any launch.  bins->weight is not read.  One launch. */
int mmd_count_collisions_binned(const float* trajs_dev, const mmd_cons_bins* bins, int n_local, int samples_per_robot, float margin,
                                int32_t* counts_dev, void* stream);

/* ---- the search layer of CBS / PrioritizedPlanning (mmd/planners/multi_agent/cbs.py, prioritized_planning.py) ----------------
 * Agent k of a search state is its chosen sample of a batch, with its own length and start time.  Its position at global time t
 * is path_k[clamp(t - s_k, 0, L_k - 1)]: global_pad_paths (mmd/common/multi_agent_utils.py:120-143) without the padded tensors.
 * The global horizon is Tg = max_k (L_k + s_k).  The collision test and the midpoint are the fp32 operations of mmd_rr_collisions:
 * ||p_a - p_b|| < margin (margin = 2.1 * radius, robot_planar_disk.py:186) and (p_a + p_b) / 2. */
typedef struct mmd_agent_path {
  const float* batch_dev;        /* [B_k, L_k, 4] un-normalised (x, y, vx, vy) samples of agent k (only x, y are read) */
  int32_t index;                 /* the chosen sample (SearchState.ix_best_path_in_batch_l[k]) */
  int32_t length;                /* L_k: 64 for MPD, K * 64 for a K-tile MPDEnsemble */
  int32_t start_time;            /* s_k (CBS / PrioritizedPlanning start_time_l) */
  int32_t reserved;
} mmd_agent_path;                /* 24 bytes */

typedef struct mmd_conflict {
  int32_t t, a, b, reserved;     /* global time step, the two agents */
  float pa[2], pb[2];            /* both agents' positions at t (PointConflict.p_l, VertexConflict.q_l) */
  float mid[2];                  /* (pa + pb) / 2 (PointConflict.q_l, the midpoint of check_rr_collisions) */
  float reserved2[2];
} mmd_conflict;                  /* 48 bytes */

#define MMD_CONFLICTS_ORDERED 0  /* CBS.get_conflicts with PointConflict (cbs.py:193-246): every (t, a, b), a != b, in torch.nonzero
                                  * row-major order -- each pair twice */
#define MMD_CONFLICTS_PAIRS 1    /* PrioritizedPlanning.get_conflicts (prioritized_planning.py:249-298): (t, a, b), a < b, loop order */
#define MMD_SELECT_CBS 0         /* CBS.expand 'least_collisions' (cbs.py:446-456): the first free index with the smallest count */
#define MMD_SELECT_PP 1          /* PrioritizedPlanning.plan (prioritized_planning.py:172-182): start from idx_best_traj and its count;
                                  * only a strictly smaller count replaces it */

/* The conflict list of a search state in one launch sequence (CBS.get_conflicts, cbs.py:166-246, densification 1;
 * PrioritizedPlanning.get_conflicts, prioritized_planning.py:249-298).  agents_dev [n_agents] (device copy of the table),
 * horizon_global = Tg.  count_dev [1] = the number of conflicts; first_dev (may be NULL) = the first record, or t = a = b = -1
 * when there is none; list_dev (may be NULL) = the first min(count, list_cap) records in order (count > list_cap: truncated).
 * row_counts_dev [Tg] int32 scratch (afterwards: the count per time step). */
int mmd_find_conflicts(const mmd_agent_path* agents_dev, int n_agents, int horizon_global, float margin, int mode,
                       int32_t* row_counts_dev, int32_t* count_dev, mmd_conflict* first_dev, mmd_conflict* list_dev, int list_cap,
                       void* stream);

/* The conflict report of a round's best paths on a cell table of those paths (mmd_bin_paths, first_step = 0): paths_dev [n_all, H, 2] with
 * n_all = bins->n_all, horizon = H, equal start times.  count_dev, first_dev, list_dev / list_cap and row_counts_dev [H] are exactly what
 * mmd_find_conflicts(..., MMD_CONFLICTS_PAIRS, ...) gives for an agent table of the same paths with start_time 0 and length 64 -- the
 * records (t, a, b), a < b, in row-major order, pa / pb / mid the same bits -- and robot_counts_dev [n_all] (may be NULL) =
 * #{(t, j != r) : ||p_r(t) - p_j(t)|| < margin}: every pair counts once for each of its two robots (the row sums of mmd_rr_collisions'
 * mask).  Work and memory are O(n_all x list length): robot a walks the list of its own cell and keeps the ids above its own.  Three
 * launches, no atomics, no host synchronisation; the list is the same on every run.  Errors as mmd_count_collisions_binned. */
int mmd_path_conflicts_binned(const float* paths_dev, const mmd_cons_bins* bins, int horizon, float margin, int32_t* row_counts_dev,
                              int32_t* robot_counts_dev, int32_t* count_dev, mmd_conflict* first_dev, mmd_conflict* list_dev, int list_cap,
                              void* stream);

/* The 'least_collisions' choice for re-planned agent `agent` without the per-candidate get_conflicts loop (cbs.py:446-458,
 * prioritized_planning.py:172-182): for candidate c (sample cand_idx_dev[c] of cand_batch_dev [B, L_agent, 4], in the order of
 * trajs_final_free_idxs) the conflict count (in `mode`) of the state with that sample swapped in for agent `agent` -- the pairs
 * without `agent` are one constant, the rest counted per candidate -- then `rule` picks one.  MMD_SELECT_PP reads one more entry,
 * cand_idx_dev[n_free] = idx_best_traj.  The other agents' entries of agents_dev are fixed; the entry of `agent` gives L and s
 * (its batch / index are not read).  result_dev [2] = (chosen sample index, its count), (-1, -1) for CBS without candidates;
 * counts_dev [n_free] (may be NULL) = every candidate's count; scratch_dev: horizon_global + n_free + 1 int32. */
int mmd_scan_candidates(const mmd_agent_path* agents_dev, int n_agents, int horizon_global, int agent, const float* cand_batch_dev,
                        const int32_t* cand_idx_dev, int n_free, float margin, int mode, int rule, int32_t* scratch_dev,
                        int32_t* counts_dev, int32_t* result_dev, void* stream);

/* The constraint group the two searches build from the other agents' chosen paths, as ONE ELL block (the layout of
 * mmd_pack_constraints, bitwise the table it makes from the equivalent MultiPointConstraint, in the same slot order):
 *   soft (hard = 0): CBS.create_soft_constraints_from_other_agents_paths (cbs.py:468-508) -- for every agent j != agent of
 *     agents_dev[0, n_state) and every t_j < L_j: t_i = t_j + s_j - s_i is kept iff 1 <= t_i <= agent_last_t (L_i - 1 when agent i
 *     has a path in the state; agent_last_t < 0: L_j - 1, the reference's rule when it has none), range (t_i, t_i + 1);
 *   hard (hard = 1): PrioritizedPlanning.plan (prioritized_planning.py:149-159) -- the same points, the ranges clamped to
 *     (max(0, min(t0, H - 1)), min(H - 1, t1)).
 * Every point has radius `radius` (vertex_constraint_radius).  ell_out_dev [n_slots][H][4]; n_slots = the largest number of agents
 * with a point active at one t (a function of the lengths and start times only: the caller sizes it; the kernel never writes past
 * it).  grp_slot_off_dev [2], grp_weight_dev [1] (= weight), robot_grp_off_dev [2]: one group for one robot, or all three NULL. */
int mmd_path_constraints(const mmd_agent_path* agents_dev, int n_state, int agent, int agent_start_time, int agent_last_t, int hard,
                         int horizon, float radius, float weight, int n_slots, float* ell_out_dev, int32_t* grp_slot_off_dev,
                         float* grp_weight_dev, int32_t* robot_grp_off_dev, void* stream);

/* ---- the round table: conflict-driven hard constraints next to the soft all-pairs group, for many-robot rounds -----------------
 * A dense constraint table in the layout mmd_guide_desc reads, for the local robots [robot0, robot0 + n_local) of n_all.  With
 * S_h = hard_slots (the caller's cap) and S = S_h + n_all - 1, local robot r owns the slots [r S, (r + 1) S) and two groups, hard
 * first (the order CBS passes them in, cbs.py:407-413):
 *   group 2 r     = slots [r S, r S + S_h), weight_hard: the points of the robot's conflicts (convert_conflicts_to_constraints,
 *                   mmd/common/conflict_conversion.py:41-55, weight_grad_cost_constraints = 2e-1);
 *   group 2 r + 1 = slots [r S + S_h, (r + 1) S), weight_soft: the words mmd_soft_constraints_from_paths writes for the robot.
 * ell_dev [n_local S][H][4], grp_slot_off_dev [2 n_local + 1], grp_weight_dev [2 n_local], robot_grp_off_dev [n_local + 1] (= 2 r),
 * max_slots_per_robot = S; fill_dev int32 [n_local][H] (the hard slots in use per time step) and dropped_dev int32 [n_local] belong to
 * the table and persist between calls.  No offset depends on data: no sizing pass, no host synchronisation, one launch each.
 * horizon = H.  NULL pointers, hard_slots < 1, a robot range outside [0, n_all) or n_all < 2 are error returns before any launch.
 *
 * mmd_round_constraints_init: offsets and weights, every hard slot inactive ((0, 0, -1, -1), as mmd_pack_constraints leaves an unused
 * slot), fill and dropped zeroed.  The soft blocks are not written. */
int mmd_round_constraints_init(int n_all, int n_local, int horizon, int hard_slots, float weight_hard, float weight_soft, float* ell_dev,
                               int32_t* grp_slot_off_dev, float* grp_weight_dev, int32_t* robot_grp_off_dev, int32_t* fill_dev,
                               int32_t* dropped_dev, void* stream);

/* The soft blocks of a round from the best paths paths_dev [n_all, H, 2]: slot j of robot r's block = the j-th other robot in ascending
 * id, every time step t >= 1 active with `radius`, t = 0 inactive -- bit for bit mmd_soft_constraints_from_paths' block of that robot. */
int mmd_round_soft_from_paths(const float* paths_dev, int n_all, int robot0, int n_local, int horizon, int hard_slots, float radius,
                              float* ell_dev, void* stream);

/* Appends the hard points of the conflicts of paths_dev [n_all, H, 2] (n_all = bins->n_all, local robots from bins->robot0) to the hard
 * blocks, read off the round's collision cell table `bins` (mmd_bin_paths of the same paths, first_step = 0).  Every record (tc, a, b,
 * mid) of mmd_path_conflicts_binned's report gives both a and b the point (mid.x, mid.y, radius, radius |radius|) -- the report's bits
 * -- with range (tc - t_pad, tc + t_pad), i.e. active at the time steps tc - t_pad <= t < tc + t_pad of [0, H).  The slots are
 * mmd_pack_constraints' for the list of the robot's records in report order, behind the lists of earlier calls: a point's slot at t is
 * fill[r][t] when it arrives, which it then increments (CBS accumulates constraints down a branch the same way).  A point whose slot
 * would reach hard_slots is not written and counts into dropped_dev[r]; everything before it in order is kept.  The collision test is
 * mmd_rr_collisions'.  t_pad < 1, margin > bins->radius, or a table mmd_count_collisions_binned would refuse are error returns. */
int mmd_conflict_constraints_append(const float* paths_dev, const mmd_cons_bins* bins, int n_local, int horizon, int hard_slots, int t_pad,
                                    float margin, float radius, float* ell_dev, int32_t* fill_dev, int32_t* dropped_dev, void* stream);

/* ---- which robots a round re-plans -----------------------------------------------------------------------------------------------
 * A round that re-samples every robot moves every path at once: each robot is guided away from paths that no longer hold.  A robot that
 * keeps its path is a constraint that stays true, so a round may re-plan a SUBSET: `selected_dev` int32 [n_all], 0 / 1, from the conflicts
 * of paths_dev [n_all, H, 2] (n_all = bins->n_all), read off the round's collision cell table `bins` (mmd_bin_paths of the same paths,
 * first_step = 0) and robot_counts_dev [n_all], mmd_path_conflicts_binned's per-robot counts of these paths.  Robots r != j are
 * neighbours iff ||p_r(t) - p_j(t)|| < margin at some t (mmd_rr_collisions' test, symmetric in the two robots). */
#define MMD_REPLAN_CONFLICTED 0  /* selected[r] = counts[r] > 0: every robot of a conflict.  iters is ignored */
#define MMD_REPLAN_INDEPENDENT 1 /* an independent set of the conflict graph, by iters >= 1 Jacobi iterations of priority propagation:
                                  * r beats j iff counts[r] > counts[j], or the counts are equal and r < j.  A robot starts OUT if its
                                  * count is 0, else UNDECIDED; an iteration reads the old states and writes the new ones: an UNDECIDED
                                  * robot becomes OUT if a neighbour is IN, else IN if every neighbour that beats it is OUT, else stays.
                                  * selected = IN after the last iteration.  For every iters: no two selected robots are neighbours (every
                                  * re-planned robot's neighbours keep their paths), and a robot is selected whenever there is a conflict.
                                  * iters = 1 selects the strict local maxima of the priority; the limit is the lexicographically first
                                  * maximal independent set */
/* perm_dev int32 [n_all]: the stable partition of 0 .. n_all - 1, the selected ids ascending, then the others ascending.  The instance
 * paths[perm] has the selected robots as a prefix, and since a rank owns a block of ascending ids, its selected robots are the block
 * [header[1], header[1] + header[2]) of that prefix: a subset round of the rank is an ordinary round of the permuted instance with
 * robot0 = header[1], n_local = header[2] (mmd_soft_constraints_from_paths / mmd_bin_constraints_from_paths, the sampler with
 * traj_index_base = header[1] * B, mmd_count_collisions), with the rows that round gives those robots.
 * header_dev int32 [4] = (robots selected, of them below bins->robot0, of them in the shard [bins->robot0, bins->robot0 + n_local),
 * robots left UNDECIDED: 0 in mode CONFLICTED).  state_dev int32 [2][n_all]: scratch.  iters + 1 launches in mode INDEPENDENT, 2 in
 * mode CONFLICTED, no atomics, no host synchronisation.  NULL pointers, an unknown mode, iters < 1 in mode INDEPENDENT, margin >
 * bins->radius, a shard outside [0, n_all), or a table mmd_count_collisions_binned would refuse are error returns before any launch. */
int mmd_round_select(const float* paths_dev, const mmd_cons_bins* bins, const int32_t* robot_counts_dev, int n_local, int horizon,
                     float margin, int mode, int iters, int32_t* state_dev, int32_t* selected_dev, int32_t* perm_dev, int32_t* header_dev,
                     void* stream);

/* ---- the framed all-pairs table: many-robot rounds in a world larger than one tile ------------------------------------------------
 * Every robot plans in the model's own tile frame; offsets_dev [n_all, 2] places each robot's window in a global frame (global = local +
 * offset), and paths_dev [n_all, H, 2] holds GLOBAL positions.  For local robot i (r = robot0 + i) and time step t >= 1, walk j = 0 ..
 * n_all - 1 without j == r: q = (paths[j][t].x - off[r].x, paths[j][t].y - off[r].y), one fp32 subtraction per axis; j is INCLUDED iff
 * window_lo.x <= q.x <= window_hi.x and the same in y (plain fp32 compares: a NaN is excluded).  The s-th included j in ascending id is
 * written as (q.x, q.y, radius, radius |radius|) into slot s of robot i, column t -- mmd_pack_constraints' slot rule, so the host pack of
 * the included points gives the same table.  An included point past slot `slots` - 1 is not written and counts into dropped_dev[i] (summed
 * over t); slots from the fill up, and every slot of column t = 0, hold the empty word (0, 0, -1, -1).  used_dev[i] = the largest fill
 * over t.  One group per robot: grp_slot_off[i] = i slots, robot_grp_off[i] = i, grp_weight[i] = weight; max_slots_per_robot = slots,
 * cons_uniform_radius = radius.  ell_out_dev [n_local slots][H][4], grp_slot_off_dev and robot_grp_off_dev [n_local + 1], grp_weight_dev,
 * used_dev, dropped_dev [n_local].  window_lo / window_hi: host, the robot's local frame.  The culling is exact for the guided step when
 * the window covers the normaliser's position limits widened by (1 + 1/16) radius: the step clips every position into those limits and a
 * point acts only within its radius (the argument is next to the kernel).  With zero offsets, an unbounded window and slots = n_all - 1
 * the columns t >= 1 are mmd_soft_constraints_from_paths' bit for bit.  One launch, no atomics, no host synchronisation; O(n_all) work
 * per (robot, time step).  NULL pointers, horizon != H, n_all outside [2, 4096], a robot range outside [0, n_all), slots outside
 * [1, n_all - 1], radius <= 0 or window_lo[k] >= window_hi[k] are error returns before any launch. */
int mmd_framed_constraints_from_paths(const float* paths_dev, const float* offsets_dev, int n_all, int robot0, int n_local, int horizon,
                                      int slots, float radius, float weight, const float window_lo[2], const float window_hi[2],
                                      float* ell_out_dev, int32_t* grp_slot_off_dev, float* grp_weight_dev, int32_t* robot_grp_off_dev,
                                      int32_t* used_dev, int32_t* dropped_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The statistics of a returned solution (scripts/inference/inference_multi_agent.py:285-342, run_multi_agent_trial)
 * ---------------------------------------------------------------------------------------------------------- */

/* The data-adherence rule of a tile's environment (compute_traj_data_adherence of deps/torch_robotics/torch_robotics/environments/):
 * every rule reads the tile's 64 positions after its offset was subtracted and gives a score in [0, 1]. */
#define MMD_ADHERENCE_LINE 0        /* EnvEmpty2D, EnvEmptyNoWait2D (env_empty_2d.py:132-146): the fraction of points closer than 0.1
                                     * (mmd_params.py:57) times the first-to-last distance to that line; first == last: 0 */
#define MMD_ADHERENCE_HIGHWAYS 1    /* EnvHighways2D (env_highways_2d.py:255-273): 1 iff the cross products of consecutive normalised
                                     * position vectors sum to > 0 (counter-clockwise); a point at the origin: 0 */
#define MMD_ADHERENCE_CONVEYOR 2    /* EnvConveyor2D (env_conveyor_2d.py:161-185): 1 iff the three waypoints of the top corridor (right
                                     * to left) or of the bottom one (left to right) are visited in order (radius 0.2) */
#define MMD_ADHERENCE_DROP_REGION 3 /* EnvDropRegion2D (env_drop_region_2d.py:183-196): 1 iff 16 consecutive points among rows 0 .. 62 lie
                                     * within 0.15 of one of the 16 drop-region centres */

typedef struct mmd_tile_ref {    /* one (agent, skeleton step) of a solution */
  int32_t agent;                 /* row of paths_dev */
  int32_t t0;                    /* first of the tile's 64 rows in the agent's padded path: start_time + skeleton_step * 64 */
  float offset[2];               /* the tile's transform, subtracted before scoring (inference_multi_agent.py:310-313) */
  int32_t rule;                  /* MMD_ADHERENCE_* */
  int32_t reserved;
} mmd_tile_ref;                  /* 24 bytes */

/* paths_dev [n_agents, horizon_global, 4]: the solution as CBS.plan / PrioritizedPlanning.plan return it -- un-normalised (x, y, vx, vy),
 * global frame, globally padded (global_pad_paths); horizon_global = Tg >= 1 is arbitrary (K * 64 + stagger).  The tile table is passed twice,
 * as agents_dev tables are built by their caller: tiles [n_tiles] on the HOST, checked here (a rule other than MMD_ADHERENCE_*, an agent
 * outside [0, n_agents) or 64 rows that do not fit in Tg are error returns), and tiles_dev, the same table on the device, which the kernel
 * reads.
 * stats_dev: ONE buffer of 1 + 2 * n_agents + n_tiles 4-byte words, so that a trial needs one device -> host copy:
 *   [0]                       int32  #{(t, i < j) : ||p_i(t) - p_j(t)|| < collision_dist} over all Tg rows (inference_multi_agent.py:288-294;
 *                                    the fp32 form of mmd_rr_collisions; collision_dist = 2.0 * radius there)
 *   [1, 1 + n)                fp32   path_length[a] = sum_t ||p_{t+1} - p_t|| (trajectory/metrics.py:13-16)
 *   [1 + n, 1 + 2n)           fp32   mean_accel[a] = mean_t ||v_{t+1} - v_t|| over Tg - 1 terms (trajectory/metrics.py:52-65)
 *   [1 + 2n, 1 + 2n + tiles)  fp32   adherence[tile]
 * The count and the adherence scores are exact; the two sums are fixed-order (no floating-point atomics). */
int mmd_solution_stats(const float* paths_dev, int n_agents, int horizon_global, float collision_dist, const mmd_tile_ref* tiles,
                       int n_tiles, const mmd_tile_ref* tiles_dev, float* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Post-sampling selection: the step right after the sampler in MPD.__call__
 * (mmd/planners/single_agent/mpd.py:344-405)
 * ---------------------------------------------------------------------------------------------------------- */

/* PlanningTask.get_trajs_collision_and_free (deps/torch_robotics/torch_robotics/tasks/tasks.py:236-311) +
 * compute_path_length / compute_smoothness (trajectory/metrics.py:7-39) + smooth_trajs
 * (mmd/common/trajectory_utils.py:31-40) for a batch of UN-normalised trajectories trajs_dev [n_traj, horizon, 4]
 * (horizon = 64, or K * 64 for MPDEnsemble's K tiles chained along the horizon; H below = horizon):
 *   - every segment is linearly interpolated at `num_interpolation` points x_t * alpha_j + x_{t+1} * (1 - alpha_j)
 *     (alpha [num_interpolation] host = torch.linspace(0, 1, n + 2)[1:n+1], trajectory/utils.py:73-86) and each point
 *     is tested against the fixed-object SDF grids and workspace boundaries of `env` (only its map / boundary fields
 *     are read: limits_*, grid_*, n_grids, sdf_grids_dev, robot_map_dev, ws_*) with `margin` (= robot radius,
 *     tasks.py:251-253): waypoint_collisions_dev [n_traj][(H-1) * num_interpolation] (may be NULL); num_interpolation = 0
 *     tests the H support points themselves, as interpolate_traj_via_points returns the trajectory then
 *     (trajectory/utils.py:76-77): waypoint_collisions_dev [n_traj][H] (with all_free != 0 nothing is written);
 *   - free_dev[n] = 1 iff no interpolated point collides and every support point lies inside [q_min, q_max]
 *     (tasks.py:262-281); all_free != 0 skips both tests (PlanningTaskEnsemble, tasks_ensemble.py:271-277);
 *   - path_length_dev / smoothness_dev [n_traj]: sum_t ||p_{t+1} - p_t||, sum_t ||v_{t+1} - v_t||;
 *   - smoothed_dev [n_traj, H, 4] (may be NULL) = S @ trajectory with the Savitzky-Golay operator savgol_dev [H][H]
 *     (row-major, device; NULL = copy) whose row r is zero outside columns [r - savgol_band, r + savgol_band]. */
int mmd_postprocess_trajs(const mmd_guide_desc* env, const float* trajs_dev, int n_robots, int samples_per_robot,
                          int horizon, int num_interpolation, const float* alpha, float margin, const float* q_min,
                          const float* q_max, int all_free, const float* savgol_dev, int savgol_band,
                          uint8_t* waypoint_collisions_dev,
                          uint8_t* free_dev, float* path_length_dev, float* smoothness_dev, float* smoothed_dev,
                          void* stream);

/* Per robot, the index (within its samples_per_robot samples) of the best FREE sample: with counts_dev == NULL the
 * argmin of cost_a (+ cost_b if not NULL) (torch.argmin(cost_all), mpd.py:366-370) in torch.argmin's order: the first
 * index wins among equal keys, and a NaN key counts as smaller than every number (the first NaN candidate is the pick; a NaN on
 * a sample that is no candidate is ignored); with counts_dev the first free
 * sample with the fewest robot-robot collisions (CBS 'least_collisions', cbs.py:446-458).  n_free_dev[r] = number of
 * free samples; when it is 0 the pick is made over all samples instead.  summary_dev (optional, fp32 [n_traj + n_robots]): the free
 * flags as 0 / 1 followed by the picks -- laid out so that, with path_length_dev / smoothness_dev of mmd_postprocess_trajs placed right
 * behind it, everything the host needs to assemble a PlannerOutput crosses in ONE device -> host copy. */
int mmd_select_best(const uint8_t* free_dev, const float* cost_a_dev, const float* cost_b_dev, const int32_t* counts_dev,
                    int n_robots, int samples_per_robot, int32_t* idx_best_dev, int32_t* n_free_dev, float* summary_dev,
                    void* stream);

/* A planning round's pick in one pass (MultiRobotSampler.best_paths of the dense-table round): for the robots of a sampling call, straight
 * from their NORMALISED samples x_dev [n_robots * samples_per_robot, H, 4], what the chain un-normalise (with the clip to [-1, 1] applied to
 * every element: torch.clip, a NaN stays a NaN) -> mmd_postprocess_trajs (all_free = 0, no smoothing) -> mmd_count_collisions ->
 * mmd_select_best -> gather of the picks' positions computes, bit for bit, in two kernels: per sample (one wave, lane = support point) the
 * free flag, path length + smoothness and the collision count against paths_all_dev; per robot the pick (mmd_select_best's rule: the free
 * samples first, the fewest collisions or, with paths_all_dev == NULL, the smallest path length + smoothness, the first index among equals,
 * all samples when none is free) and its un-normalised positions. */
typedef struct mmd_round_pick {
  const float* paths_all_dev;     /* [n_all, H, 2] un-normalised best paths of all robots, or NULL: the cost rule */
  int32_t n_all;                  /* robots in paths_all_dev (ignored without it) */
  int32_t robot0;                 /* index in paths_all_dev of the call's first robot (its own path is not counted) */
  float norm_min[4], norm_max[4]; /* the normaliser's limits: x_u = (clip(x) + 1) / 2 * (max - min) + min */
  int32_t num_interpolation;      /* as mmd_postprocess_trajs, with its host table alpha [num_interpolation] */
  const float* alpha;
  float margin;                   /* map / workspace margin (the robot radius) */
  float q_min[2], q_max[2];       /* joint limits of the support points */
  float rr_margin;                /* robot-robot collision distance (mmd_count_collisions' margin) */
  float* paths_out_dev;           /* [n_robots, H, 2]: the picks' un-normalised positions */
  int32_t* idx_out_dev;           /* [n_robots]: the pick within the robot's samples */
  int32_t* n_free_out_dev;        /* [n_robots]: free samples of the robot */
  void* scratch_dev;              /* n_robots * samples_per_robot * 8 bytes */
} mmd_round_pick;

/* The pick of robots [0, n_robots) of x_dev on `stream`.  env: only its map / boundary fields are read, as in mmd_postprocess_trajs;
 * robot r reads map robot_map_dev[r]. */
int mmd_round_pick_paths(const mmd_guide_desc* env, const mmd_round_pick* pick, const float* x_dev, int n_robots,
                         int samples_per_robot, void* stream);

/* mmd_p_sample_loop followed by mmd_round_pick_paths of its final samples (env = guide, which must not be NULL), in one call.  With
 * stream chunks, every chunk's pick is enqueued on the chunk's own stream behind its last step, before the join: the pick of the chunk
 * that finishes first runs beside the other chunk's last step, and the caller's stream sees the one join.  With one chunk, or without
 * side streams, the pick follows the loop on the caller's stream.  pick->paths_all_dev must not be written while the call runs (it is the
 * previous round's gathered paths).  Samples and picks are bitwise those of the two calls made one after the other. */
int mmd_p_sample_loop_pick(mmd_unet_t unet, const mmd_sampler_desc* s, const mmd_guide_desc* guide, float* x_dev,
                           const float* hard_dev, int n_robots, int samples_per_robot, int n_steps,
                           int n_steps_without_noise, int init_noise, const float* step_noise_dev, uint64_t seed,
                           float* chain_dev, void* workspace_dev, size_t workspace_bytes, const mmd_round_pick* pick,
                           void* stream);

/* PlanningTask.compute_collision (tasks.py:141-143, :204-232; occupancy of the fixed objects + workspace boundaries)
 * for n_points positions (x, y at points_dev[i * point_stride + {0, 1}]) on map `map_index` of `env`. */
int mmd_points_collision(const mmd_guide_desc* env, const float* points_dev, int n_points, int point_stride, int map_index,
                         float margin, uint8_t* out_dev, void* stream);

/* LimitsNormalizer.unnormalize (mmd/datasets/normalization.py:157-168; TrajectoryDataset.unnormalize_trajectories, what MPD.__call__
 * applies to the sampled chain, mpd.py:344-347) for n_points float4 states (x, y, vx, vy): a tensor is clipped to [-1, 1] as a WHOLE iff any of
 * its elements lies outside [-1 - eps, 1 + eps] (the reference's data-dependent clip, decided on the device) AND none is a NaN (with a NaN
 * the reference's `x.max() > 1 + eps or x.min() < -1 - eps` is false: the tensor stays unclipped and no NaN ever becomes a number), then
 * x_u = (x + 1) / 2 * (maxs - mins) + mins.  One call may hold SEVERAL tensors interleaved (the chains of R planner calls batched robot-major, [steps][R][B*H]):
 * point i belongs to tensor (i % period_points) / segment_points, each tensor gets its own clip decision; period_points = segment_points = 0
 * means one tensor.  flags_dev: period_points / segment_points uint32 of scratch (per tensor: byte 0 = out of range, byte 1 = NaN seen).  mins / maxs: host [4].  out_dev may alias x_dev. */
int mmd_unnormalize_trajs(const float* x_dev, size_t n_points, size_t period_points, size_t segment_points, const float* mins,
                          const float* maxs, float eps, float* out_dev, uint32_t* flags_dev, void* stream);

/* compute_variance_waypoints (trajectory/metrics.py:17-27): var_per_waypoint_dev[t] = unbiased variance of all
 * n_traj^2 entries of triu(cdist(p_t, p_t), 1); the metric is their sum over t. */
int mmd_variance_waypoints(const float* trajs_dev, int n_traj, int horizon, float* var_per_waypoint_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Custom maps: the fixed objects' SDF grid built on the device from spheres and rounded boxes
 * ---------------------------------------------------------------------------------------------------------- */

/* GridMapSDF.precompute_sdf (deps/torch_robotics/torch_robotics/environments/grid_map_sdf.py:34-63) for one
 * ObjectField([MultiSphereField(spheres), MultiBoxField(boxes)]) at the identity pose (primitives.py:108-115, :326-333, :569-572):
 * grid_dev[ix * ny + iy] = (sdf, dsdf/dx, dsdf/dy, 0) at the node (xs_dev[ix], ys_dev[iy]) -- one map's slice [nx][ny] of
 * mmd_guide_desc.sdf_grids_dev.  The node coordinates are the caller's (torch.linspace(lo, hi, n) of the reference, computed once on the
 * host), so the nodes are the reference's to the bit.
 *   spheres_dev [n_spheres][4] = (cx, cy, r, 0)             -- mmd_guide_desc.extra_spheres_dev's layout
 *   boxes_dev   [n_boxes][4]   = (cx, cy, half x, half y)   -- mmd_guide_desc.extra_boxes_dev's layout; rounding radius 0.15 x the smaller size
 * The value and the gradient are those of torch autograd on the host, bit for bit but for the sign of a zero (plain fp32, no contraction, both norms as
 * sqrt(fma(y, y, x * x)), correctly rounded division and square root), with torch's sub-gradients at the ties:
 *   - among equal minima the first wins, spheres before boxes, in table order (torch.min over the primitives, then over the fields);
 *   - an empty sphere field is the constant 1 with gradient 0 and takes part in the minimum first (primitives.py:109-110); an empty box
 *     field is left out; no primitive at all: (1, 0, 0, 0) everywhere;
 *   - a sphere centred on the node has gradient 0 (torch.norm's backward at 0);
 *   - inside a box the amax tie qx == qy splits evenly, and minimum(max q, 0) passes half at max q == 0 (primitives.py:331-332);
 *   - a gradient component that is zero is +0 (autograd's own zero may be -0 = 0 * -1 where a field has one primitive: equal in value).
 * Error returns, before anything is launched: a NULL table with a non-zero count or a negative count, nx or ny below 1, nx * ny of
 * 2^31 - 256 or more, a NULL coordinate row, a NULL grid. */
int mmd_sdf_grid_build(const float* spheres_dev, int n_spheres, const float* boxes_dev, int n_boxes, const float* xs_dev, int nx,
                       const float* ys_dev, int ny, float* grid_dev, void* stream);

/* The same texture from an OCCUPANCY BITMAP (a floor plan, a benchmark grid, a costmap): an exact Euclidean distance transform with
 * nearest-site tracking.  occ_dev [nx][ny] bytes, non-zero = occupied, indexed like the grid: cell (ix, iy) is the cell the lookup
 * floor((p - lo) / (hi - lo) * n) gives a point; `cell` is the cell pitch.  grid_dev[ix * ny + iy] = (sdf, dsdf/dx, dsdf/dy, 0):
 *   - the site of a cell is the nearest cell of the other class by D2 = (ix - jx)^2 + (iy - jy)^2 (an exact integer), the
 *     lexicographically smallest (jx, jy) among equal D2;
 *   - s = sqrt(float(D2)), v = cell * s - 0.5 * cell (the surface lies on the cell edge), plain fp32, one rounding per operation;
 *   - a free cell: (+v, (ix - jx) / s, (iy - jy) / s, 0), away from the obstacle; with v not below 1: (1, 0, 0, 0), the constant-1 field
 *     of the primitive maps;
 *   - an occupied cell: (-v, (jx - ix) / s, (jy - iy) / s, 0), towards free space;
 *   - a zero component is +0; no occupied cell at all: (1, 0, 0, 0) everywhere; no free cell at all: (-1, 0, 0, 0) everywhere (both
 *     decided on the device: the call does not synchronise).
 * mmd_amd/environments.py::occupancy_sdf_texture is the same definition on the host, and the grid is that texture bit for bit.
 * work_dev: mmd_sdf_grid_occupancy_work_bytes(nx, ny) bytes of device memory (two [nx][ny] int16 tables: per row, the signed iy offset to
 * the nearest occupied and to the nearest free cell), 2-byte aligned, overwritten by every call; the result does not depend on what it held.
 * Error returns, before anything is launched: NULL occupancy, grid or workspace; nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE (every D2
 * is then an exact fp32 integer); a cell that is not finite and positive; work_bytes too small.
 * mmd_sdf_grid_occupancy_work_bytes returns 0 for a size the build refuses. */
#define MMD_OCCUPANCY_MAX_SIDE 2048
size_t mmd_sdf_grid_occupancy_work_bytes(int nx, int ny);
int mmd_sdf_grid_from_occupancy(const unsigned char* occ_dev, int nx, int ny, float cell, float* grid_dev, void* work_dev,
                                size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * World maps: one texture for a world larger than a tile, the robots' windows cut from it on the device
 * ---------------------------------------------------------------------------------------------------------- */

/* Robot windows of a WORLD texture (mmd_sdf_grid_from_occupancy of a bitmap of up to 2048 cells per side): n_windows slices of
 * mmd_guide_desc.sdf_grids_dev, in one launch.  world_grid_dev [wnx][wny][4], origins_dev [n_windows][2] = (i0, j0) int32 on the device,
 * windows_dev [n_windows][nx][ny][4]:
 *   windows[k][ix][iy] = world[clamp(i0_k + ix, 0, wnx - 1)][clamp(j0_k + iy, 0, wny - 1)],
 * all four words copied as bits (NaN payloads and the sign of a zero survive).  The origins are device data, so the source index is
 * clamped per axis: that is the defined result for an origin outside the world (any int32), not an error.  A window of the world's
 * transform is not the transform of the cropped bitmap: an obstacle just outside the window acts on the texels near its border, and
 * overlapping windows agree where they overlap.  The windows must not overlap the world grid in memory.
 * Error returns, before anything is launched: n_windows negative or above MMD_SDF_GRID_MAX_WINDOWS; wnx or wny below 1; nx (ny) below 1
 * or above wnx (wny); wnx * wny of 2^31 - 256 or more; with n_windows > 0, a NULL world grid, origins or windows.  n_windows == 0
 * returns 0 and launches nothing. */
#define MMD_SDF_GRID_MAX_WINDOWS 65535
int mmd_sdf_grid_windows(const float* world_grid_dev, int wnx, int wny, const int32_t* origins_dev /* [n][2] */, int n_windows,
                         int nx, int ny, float* windows_dev /* [n][nx][ny][4] */, void* stream);

/* The texel every consumer of a texture reads for a point: out_dev[i] = grid_dev[ix][iy] (four words) with, per axis and in fp32,
 * ix = floor((px - lo[0]) / |hi[0] - lo[0]| * nx) clamped to [0, nx - 1] -- the sequence of the guided step's gather and of the
 * post-sampling collision test, so "is this point free on the resident texture" has their answer.  points_dev [n_points][2],
 * out_dev [n_points][4].  A point with a non-finite coordinate gives four NaNs and reads no texel.
 * Error returns, before anything is launched: a negative n_points; nx or ny below 1 or nx * ny above 2^31 - 1; NULL limits, limits that are
 * not finite or an axis of zero extent; with n_points > 0, a NULL grid, points or out.  n_points == 0 returns 0 and launches nothing. */
int mmd_sdf_grid_lookup(const float* grid_dev, int nx, int ny, const float lo[2], const float hi[2],
                        const float* points_dev /* [n][2] */, int n_points, float* out_dev /* [n][4] */, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * World routes: geodesic distance fields of a texture's routable cells, and the tiles a descent crosses
 * ---------------------------------------------------------------------------------------------------------- */

/* The distance fields of n_fields goals over one SDF texture grid_dev [nx][ny][4] (any map's: a world texture, a tile's slice).  All
 * integers are exact; mmd_amd/world_routes.py (routable_cells, grid_distance_field) is the same definition on the host.
 *   routable[ix][iy] = grid[ix][iy][0] > clearance (a strict fp32 compare: a NaN texel is not routable) and
 *                      region[0] <= ix < region[2] and region[1] <= iy < region[3]   (region = (i_lo, j_lo, i_hi, j_hi), a host array)
 *   dist[f][ix][iy]  = the length in steps of the shortest 4-connected path over routable cells from goals[f] to (ix, iy), unit cost per
 *                      step; MMD_GRID_DIST_UNREACHED on a cell that is not routable or cannot be reached.  goals_dev [n_fields][2] =
 *                      (ix, iy) int32 on the device: a goal that is not routable or lies outside the grid gives a field that is
 *                      UNREACHED everywhere, not an error.
 * The method is a block-tiled Bellman-Ford: a workgroup owns a block of MMD_GRID_DIST_BLOCK x MMD_GRID_DIST_BLOCK cells of one field,
 * relaxes it in LDS against a one-cell halo until nothing in it changes, writes back what fell and marks itself changed; a block runs
 * in a sweep iff it or one of its 4 neighbour blocks changed in the sweep before.  One launch per sweep: nothing inside a sweep waits on
 * another workgroup, and the result does not depend on the order or the placement of the workgroups (the argument stands next to the
 * kernel, csrc/grid_route.hip).
 *   restart != 0: every cell becomes UNREACHED, a routable goal 0, and the goal's block is flagged; then n_sweeps sweeps.
 *   restart == 0: n_sweeps more sweeps on dist_dev and work_dev as the previous call on the same arguments left them.  A caller restarts
 *                 after the texture, the clearance, the region or a goal changed.
 *   changed_dev[f] = the number of blocks of field f that lowered a value in the call's last sweep (after a restart with n_sweeps == 0: 1
 *                 if the goal was seeded, else 0).  0 means converged: dist[f] is the exact field, and further sweeps do nothing.
 * The call runs exactly n_sweeps sweeps and does not synchronise: the convergence policy is the caller's (the number of routable cells
 * + 2 sweeps always suffice; an open grid of bx x by blocks needs at most bx + by).
 * work_dev: mmd_grid_distance_work_bytes(nx, ny, n_fields) bytes, 4-byte aligned: per field a sweep count and one int32 per block.  A
 * restart initialises it; between a restart and its continuations the caller leaves it alone.
 * Error returns, before anything is launched: nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE; n_fields negative or above
 * MMD_GRID_DIST_MAX_FIELDS (the field is a block index); n_sweeps negative; a clearance that is not finite; a NULL region, or one with
 * lo > hi or outside [0, nx] x [0, ny]; with n_fields > 0, a NULL grid, goals, dist, workspace or changed, or work_bytes too small.
 * n_fields == 0, or n_sweeps == 0 with restart == 0, returns 0 and launches nothing.
 * mmd_grid_distance_work_bytes returns 0 for a size the call refuses. */
#define MMD_GRID_DIST_BLOCK 64
#define MMD_GRID_DIST_UNREACHED 0x7fffffff
#define MMD_GRID_DIST_MAX_FIELDS 65535
size_t mmd_grid_distance_work_bytes(int nx, int ny, int n_fields);
int mmd_grid_distance_field(const float* grid_dev, int nx, int ny, float clearance, const int32_t region[4],
                            const int32_t* goals_dev /* [n_fields][2] */, int n_fields, int restart, int n_sweeps,
                            int32_t* dist_dev /* [n_fields][nx][ny] */, void* work_dev, size_t work_bytes,
                            int32_t* changed_dev /* [n_fields] */, void* stream);

/* The descent of n_queries starts through converged fields, one lane per query, and the lattice tiles each walk crosses
 * (mmd_amd/world_routes.py::descend is the same definition on the host).  Lattice tile (a, b) covers the cells
 * [o_i + a * tile, o_i + (a + 1) * tile) x [o_j + b * tile, o_j + (b + 1) * tile), lattice_origin = (o_i, o_j), a host array.
 * Query q starts at cell starts_dev[q] in field field_dev[q], both device data.  From cell c with d = dist[c], while d > 0: the
 * candidates are the neighbours in the order +x, -x, +y, -y that lie inside the grid and hold exactly d - 1; the walk takes the first
 * candidate in the lattice tile of c, or, if there is none, the first candidate.  tiles_dev[q] starts with the start's tile and gets a
 * tile each time the walk enters a tile other than the last one listed (a tile may occur twice).  summary_dev[q] = (steps, n_tiles,
 * status, 0):
 *   0  ok: steps = dist[start], n_tiles tiles written
 *   1  the start holds MMD_GRID_DIST_UNREACHED: steps = -1, n_tiles = 0, nothing written
 *   2  stuck: no neighbour holds d - 1 (the field was not converged); the walk stops there, steps and n_tiles are what it covered
 *   3  more than max_tiles tiles: n_tiles is the true count, the first max_tiles are written, steps = dist[start]
 *   4  the start lies outside the grid, or the field index outside [0, n_fields): steps = -1, n_tiles = 0, nothing written
 * The loop runs at most dist[start] times whatever the field holds (d falls by one per step); rows of tiles_dev behind n_tiles are not
 * written.  Error returns, before anything is launched: nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE; a negative n_fields or
 * n_queries; tile or max_tiles below 1; a NULL lattice_origin or one beyond +-2^30; with n_queries > 0, a NULL dist (with n_fields > 0),
 * starts, field indices, tiles or summary.  n_queries == 0 returns 0 and launches nothing. */
int mmd_grid_descend(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev /* [n][2] */,
                     const int32_t* field_dev /* [n] */, int n_queries, int tile, const int32_t lattice_origin[2], int max_tiles,
                     int32_t* tiles_dev /* [n][max_tiles][2] */, int32_t* summary_dev /* [n][4] */, void* stream);

/* mmd_grid_descend with the support cells of the cell path (mmd_amd/world_routes.py::descend_samples is the same definition on the
 * host).  The walk, tiles_dev and summary_dev are mmd_grid_descend's, word for word.  The cell path is c_0 (the start) .. c_steps (the
 * goal); visit k, the k-th listed tile, owns the path indices [f_k, f_k + m_k), m_k >= 1, and
 *   visit_cells_dev[q][k] = m_k
 *   cells_dev[q][k][j]    = c[f_k + (j * (m_k - 1) + 31) / 63], j = 0 .. 63 (integer division): monotone in j, j = 0 the visit's first
 *                           cell and j = 63 its last; with m_k = 1 all 64 are that cell.
 * Rows of visit_cells_dev and cells_dev behind a query's n_tiles, and all rows of a query whose status is not 0, are written 0 (every
 * word of both buffers is written).  One lane per query walks the field twice, with no buffer proportional to the path: the first walk
 * counts m_k, the second emits each visit's samples as it passes them.  Each walk's loop runs at most dist[start] times whatever the
 * field holds.  Error returns, before anything is launched: those of mmd_grid_descend, max_tiles above MMD_ROUTE_SEED_MAX_TILES, a NULL
 * visit_cells or cells with n_queries > 0.  n_queries == 0 returns 0 and launches nothing. */
#define MMD_ROUTE_SEED_POINTS 64
#define MMD_ROUTE_SEED_MAX_TILES 16
int mmd_grid_descend_samples(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev /* [n][2] */,
                             const int32_t* field_dev /* [n] */, int n_queries, int tile, const int32_t lattice_origin[2], int max_tiles,
                             int32_t* tiles_dev /* [n][max_tiles][2] */, int32_t* summary_dev /* [n][4] */,
                             int32_t* visit_cells_dev /* [n][max_tiles] */, int32_t* cells_dev /* [n][max_tiles][64][2] */, void* stream);

/* The seed trajectories of n_routes routes, in trajs_final's format, from what mmd_grid_descend_samples wrote
 * (mmd_amd/world_routes.py::seed_trajectory is the same definition on the host, bit for bit).  Every operation is one fp32 rounding,
 * with no fused multiply-add.  Route q with status 0 has K = n_tiles visits and N = 64 K points, i = 64 k + j:
 *   p[i]   = lo + ((float)cell + 0.5f) * pitch per axis, pitch = |hi - lo| / (float)n: the centre of cells_dev[q][k][j]; its texel is
 *            that cell.  p[0] = start_points_dev[q] and p[N - 1] = goal_points_dev[q], which stay fixed.
 *   smooth_iters Jacobi iterations, every interior i from the values of the iteration before: c = 0.5f * (p[i - 1] + p[i + 1]) per axis;
 *            (ix, iy) = the texel of c (mmd_sdf_grid_lookup's sequence); p'[i] = c iff grid[ix][iy][0] > clearance (strict: a NaN
 *            rejects) and (ix, iy) is a cell of lattice tile tiles_dev[q][i / 64]; else p'[i] = p[i].
 *   v[i]   = (p[i + 1] - p[i - 1]) / two_dt per axis (correctly rounded), 0 at i = 0 and i = N - 1.
 *   seeds_dev[q][i] = (p.x, p.y, v.x, v.y); rows behind N are 0.
 *   clear_min_dev[q] = the least grid[texel of p[i]][0] over the final points, least in the order of the values' bits (-0 below +0, a
 *            NaN beyond the infinity of its sign): one defined word whatever the texture holds.
 * A route whose status is not 0, or whose n_tiles is below 1, gets all-zero rows and clear_min 0, and reads no texel; n_tiles above
 * max_tiles counts as max_tiles.  The seed keeps the clearance at its support points, in their own tiles; it says nothing about the
 * segments between them.  One workgroup per route; the result does not depend on the launch shape.
 * Error returns, before anything is launched: nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE; NULL or non-finite limits or a zero
 * extent; a clearance that is not finite; two_dt not finite or <= 0; smooth_iters or n_routes negative; tile below 1; max_tiles outside
 * 1 .. MMD_ROUTE_SEED_MAX_TILES; a NULL lattice_origin or one beyond +-2^30; with n_routes > 0, a NULL grid, cells, tiles, summary,
 * start or goal points, seeds or clear_min.  n_routes == 0 returns 0 and launches nothing. */
int mmd_route_seeds(const float* grid_dev, int nx, int ny, const float lo[2], const float hi[2], float clearance,
                    const int32_t* cells_dev /* [n][max_tiles][64][2] */, const int32_t* tiles_dev /* [n][max_tiles][2] */,
                    const int32_t* summary_dev /* [n][4] */, int n_routes, int tile, const int32_t lattice_origin[2], int max_tiles,
                    const float* start_points_dev /* [n][2] */, const float* goal_points_dev /* [n][2] */, int smooth_iters, float two_dt,
                    float* seeds_dev /* [n][max_tiles * 64][4] */, float* clear_min_dev /* [n] */, void* stream);

/* World fleets: the next sub-goal and the window of n_queries robots, each read off the converged field of its goal, one lane per query
 * (mmd_amd/fleet_subgoals.py::window_goal is the same definition on the host, where its two facts -- the walk's box lies inside the
 * window, and a call covers at least min(d, max_steps, reach) steps -- are argued).  Query q starts at cell c0 = starts_dev[q] in field
 * field_dev[q], whose goal cell is g = goals_dev[field_dev[q]], all device data.  From cell c with d = dist[c], while d > 0, fewer than
 * max_steps steps are taken, and the chosen next cell n has max(|n.x - c0.x|, |n.y - c0.y|) <= reach: the candidates are the neighbours
 * that lie inside the grid and hold exactly d - 1, the x-candidate the first of +x, -x and the y-candidate the first of +y, -y; n is the
 * x-candidate if |g.x - c.x| >= |g.y - c.y|, else the y-candidate, and the other axis's candidate where that axis has none (open ground
 * gives a diagonal staircase, not an L).  The walk ends before a step that would leave the box.
 *   cells_dev[q]   = the last cell reached (c0 itself when d == 0 at the start)
 *   origins_dev[q] = min(max(c0 - window / 2, 0), n - window) per axis: the origin cell of the robot's window of `window` cells per side
 *   summary_dev[q] = (steps, remaining, status, arrived), remaining = dist[c0] - steps, arrived = 1 iff status is 0 and remaining is 0:
 *     0  ok
 *     1  c0 holds MMD_GRID_DIST_UNREACHED: steps = remaining = -1, cell and origin (0, 0)
 *     2  stuck: no neighbour holds d - 1 (the field was not converged); the walk stops there, the outputs are what it covered
 *     4  c0 lies outside the grid, or the field index outside [0, n_fields): steps = remaining = -1, cell and origin (0, 0)
 * Every word of the three outputs is written for every query.  The loop runs at most min(max_steps, dist[c0]) times whatever the field
 * and the goals hold.  Error returns, before anything is launched: nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE; a negative n_fields
 * or n_queries; window outside 1 .. min(nx, ny); reach outside 1 .. window / 2 - 1; max_steps below 1; with n_queries > 0, a NULL dist
 * or goals (with n_fields > 0), starts, field indices, cells, origins or summary.  n_queries == 0 returns 0 and launches nothing. */
int mmd_grid_window_goals(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev /* [n][2] */,
                          const int32_t* field_dev /* [n] */, const int32_t* goals_dev /* [n_fields][2] */, int n_queries, int reach,
                          int max_steps, int window, int32_t* cells_dev /* [n][2] */, int32_t* origins_dev /* [n][2] */,
                          int32_t* summary_dev /* [n][4] */, void* stream);

/* mmd_grid_window_goals with the support cells of the walk's cell path (mmd_amd/fleet_subgoals.py::window_goal_samples is the same
 * definition on the host).  The walk, cells_dev, origins_dev and summary_dev are mmd_grid_window_goals', word for word.  The cell path
 * is c_0 = c0 .. c_steps = the last cell reached, and
 *   samples_dev[q][j] = c[(j * steps + 31) / 63], j = 0 .. 63 (integer division; mmd_grid_descend_samples' spacing for a visit of
 *                       steps + 1 cells): monotone in j, j = 0 the start and j = 63 the sub-goal cell; with steps = 0 all 64 are c0.
 * A query whose status is not 0 (a stuck walk included) gets 64 zero rows.  Every word of the four outputs is written for every query.
 * One lane per query walks the field twice, with no buffer proportional to the path: the first walk fixes `steps`, the second emits the
 * samples as it passes them.  Each walk's loop runs at most min(max_steps, dist[c0]) times whatever the field and the goals hold; a step
 * lands on a cell that holds one less than the one before, so steps < nx * ny <= 2^22 and 63 * steps stays inside an int32.
 * Error returns, before anything is launched: those of mmd_grid_window_goals, and a NULL samples with n_queries > 0.  n_queries == 0
 * returns 0 and launches nothing. */
int mmd_grid_window_goal_samples(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev /* [n][2] */,
                                 const int32_t* field_dev /* [n] */, const int32_t* goals_dev /* [n_fields][2] */, int n_queries, int reach,
                                 int max_steps, int window, int32_t* cells_dev /* [n][2] */, int32_t* origins_dev /* [n][2] */,
                                 int32_t* summary_dev /* [n][4] */, int32_t* samples_dev /* [n][64][2] */, void* stream);

/* The seed trajectories of n_robots robots of a fleet, in trajs_final's format, from what mmd_grid_window_goal_samples wrote
 * (mmd_amd/fleet_subgoals.py::window_seed is the same definition on the host, bit for bit): mmd_route_seeds' seed of one visit whose tile
 * is the robot's own window, the cells [origins_dev[r], origins_dev[r] + window) per axis.  Every operation is one fp32 rounding, with no
 * fused multiply-add.  Robot r with status 0 (summary_dev[r][2]) has 64 points:
 *   p[j]   = lo + ((float)cell + 0.5f) * pitch per axis, pitch = |hi - lo| / (float)n: the centre of samples_dev[r][j].
 *            p[0] = start_points_dev[r] and p[63] = goal_points_dev[r], which stay fixed.
 *   smooth_iters Jacobi iterations, every interior j from the values of the iteration before: c = 0.5f * (p[j - 1] + p[j + 1]) per axis;
 *            (ix, iy) = the texel of c (mmd_sdf_grid_lookup's sequence); p'[j] = c iff grid[ix][iy][0] > clearance (strict: a NaN
 *            rejects) and (ix, iy) is a cell of the robot's window; else p'[j] = p[j].
 *   v[j]   = (p[j + 1] - p[j - 1]) / two_dt per axis (correctly rounded), 0 at j = 0 and j = 63.
 *   seeds_dev[r][j] = (p.x, p.y, v.x, v.y)
 *   clear_min_dev[r] = the least grid[texel of p[j]][0] over the final points, in mmd_route_seeds' order of the values' bits.
 * The window test is a guard for hand-built samples: the samples of a fleet's walk lie in the box of radius `reach` round the start,
 * the box lies in the window, and the window is convex, so a midpoint of two points in it never leaves it.  Samples and origins are
 * device data and may hold any words: a sample is only converted to a float, the texel index is clamped to the grid whatever a point
 * holds, and the window test is taken in 64 bits.  A robot whose status is not 0 gets 64 zero rows and clear_min 0, and reads no
 * texel.  One wave per robot, a point per lane in registers, the neighbours read across lanes: no LDS and no barrier.
 * Error returns, before anything is launched: nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE; NULL or non-finite limits or a zero
 * extent; a clearance that is not finite; two_dt not finite or <= 0; smooth_iters or n_robots negative; window below 1; with
 * n_robots > 0, a NULL grid, samples, origins, summary, start or goal points, seeds or clear_min.  n_robots == 0 returns 0 and launches
 * nothing. */
int mmd_window_seeds(const float* grid_dev, int nx, int ny, const float lo[2], const float hi[2], float clearance,
                     const int32_t* samples_dev /* [n][64][2] */, const int32_t* origins_dev /* [n][2] */,
                     const int32_t* summary_dev /* [n][4] */, int n_robots, int window, const float* start_points_dev /* [n][2] */,
                     const float* goal_points_dev /* [n][2] */, int smooth_iters, float two_dt, float* seeds_dev /* [n][64][4] */,
                     float* clear_min_dev /* [n] */, void* stream);

/* World fleets: the sub-goals of one epoch kept apart (mmd_amd/fleet_subgoals.py::subgoals_apart is the definition on the host, and
 * subgoals_apart_sweeps(s) the state after s sweeps; the argument stands in that module's docstring).  Query q TAKES PART iff
 * mmd_grid_window_goals' status for it is 0; its walk is that call's cell path c_q[0 .. walked_q], c_q[0] the start.  Two cells conflict
 * iff dx^2 + dy^2 < sep^2.  Robots are taken in index order, a lower index has priority: the blockers of robot r are the chosen cells of
 * the taking-part robots j < r and the START cells of the taking-part robots j > r, and
 *   k_r = the largest k in [1, walked_r] whose cell c_r[k] conflicts with no blocker, 0 if there is none (the largest feasible index, not
 *         the longest feasible prefix: a walk may pass a blocker);  the chosen cell is c_r[k_r].
 * THE FACT: if the start cells of the taking-part robots are pairwise at least sep apart, so are the chosen cells, and every clear is 1
 * (k = 0 always serves: robots with priority avoided r's start, the others' starts are apart from it by assumption).  mmd_grid_window_goals'
 * progress bound does NOT hold for k_r: a robot may be held back to k = 0.
 * The choice is computed as a fixed point.  A sweep gives every robot, all at once, the k of the rule above from the k of the robots
 * j < r of the sweep before (two buffers, one launch per sweep, one wave per robot; nothing inside a sweep waits on another workgroup and
 * the result does not depend on the order of the workgroups).  The dependence is strictly lower-triangular: the fixed point is unique,
 * it is the definition's, n_queries sweeps always reach it, and changed == 0 proves it is reached.
 *   restart != 0: walks every query, stores the cell paths in work_dev, sets every k to walked; then n_sweeps sweeps.
 *   restart == 0: n_sweeps more sweeps on work_dev as the previous call on the same arguments left it.
 * Either way the call then writes, for the state it reached, every word of every output for every query:
 *   cells_dev[q]   = c_q[k_q]                      origins_dev[q] = mmd_grid_window_goals'
 *   summary_dev[q] = (k_q, dist[c0] - k_q, 0, dist[c0] == k_q): mmd_grid_window_goals' format, so mmd_window_seeds reads it unchanged
 *   extra_dev[q]   = (walked_q, clear_q), clear_q = 1 iff the last sweep found that the chosen cell conflicts with no blocker (0 before
 *                    any sweep; at the fixed point it can be 0 only with k_q = 0)
 *   samples_dev[q][j] = c_q[(j * k_q + 31) / 63], j = 0 .. 63: mmd_grid_window_goal_samples' spacing on the shortened path; NULL: not written
 *   changed_dev[0] = the number of robots whose k moved in the call's last sweep (after a restart with n_sweeps == 0: the number of
 *                    queries that take part)
 * A query that does not take part gets mmd_grid_window_goals' words, extra (its summary's steps, 0) and zero samples, and blocks nobody.
 * The call does not synchronise: the convergence policy is the caller's.  work_dev: mmd_grid_window_apart_work_bytes(n_queries,
 * max_steps) bytes, 16-byte aligned; a restart initialises it, between a restart and its continuations the caller leaves it alone.
 * Error returns, before anything is launched: those of mmd_grid_window_goals; sep outside 1 .. MMD_WINDOW_APART_MAX_SEP; max_steps above
 * MMD_WINDOW_APART_MAX_STEPS; a negative n_sweeps; with n_queries > 0, a NULL, misaligned or short workspace, or a NULL cells, origins,
 * summary, extra or changed.  n_queries == 0 returns 0 and launches nothing.  mmd_grid_window_apart_work_bytes returns 0 for a size the
 * call refuses (and for n_queries == 0). */
#define MMD_WINDOW_APART_MAX_STEPS 4095
#define MMD_WINDOW_APART_MAX_SEP 1024
size_t mmd_grid_window_apart_work_bytes(int n_queries, int max_steps);
int mmd_grid_window_goals_apart(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* starts_dev /* [n][2] */,
                                const int32_t* field_dev /* [n] */, const int32_t* goals_dev /* [n_fields][2] */, int n_queries, int reach,
                                int max_steps, int window, int sep, int restart, int n_sweeps, void* work_dev, size_t work_bytes,
                                int32_t* cells_dev /* [n][2] */, int32_t* origins_dev /* [n][2] */, int32_t* summary_dev /* [n][4] */,
                                int32_t* extra_dev /* [n][2] */, int32_t* samples_dev /* [n][64][2] or NULL */,
                                int32_t* changed_dev /* [1] */, void* stream);

/* World fleets: standing robots step aside for the robots they hold back, and those walk in the same epoch
 * (mmd_amd/fleet_subgoals.py::subgoals_aside is the definition on the host; safety and containment are argued in that module's docstring;
 * csrc/window_aside.hip).  The call continues mmd_grid_window_goals_apart: apart_work_dev is that call's workspace for the same n_queries
 * and max_steps AT ITS FIXED POINT (changed == 0), which gives every query's walk c_q[0 .. walked_q] and k_q; it is only read.
 *   stands_j   j takes part and k_j == 0;      held_r   stands_r and walked_r >= 1
 *   clears(j)  the r with held_r, r != j, stands_j, c_j[0] in conflict with c_r[1], and (not held_j or r < j);  j YIELDS iff it is not empty
 *   side step  of a yielder j, the yielders taken in index order: l(c) is the 4-connected BFS distance from c_j[0] over the cells of the grid
 *              within Chebyshev distance aside_reach of it that j's own field dist[field[j]] reaches; among the cells with
 *              1 <= l(c) <= aside_steps that conflict with no final cell of another taking-part robot (a yielder i > j still on its start)
 *              and with no cell of the walk of any r in clears(j), the least (l(c), dist[field[j]][c], ix, iy); none: j stays
 *   release    r with held_r that did not move aside and lies in clears(j) of some j that did, in index order: mmd_grid_window_goals_apart's
 *              rule on c_r against the final cells of all others (a released robot of higher index still on its start) gives k'_r
 * THE FACTS: start cells pairwise sep apart give final cells pairwise sep apart; a side cell lies within aside_reach <= reach of the start,
 * hence in the robot's window.  No liveness is claimed.
 * The choice is a fixed point of sweeps (two buffers; per sweep one launch of one 256-thread workgroup per robot for the side steps --
 * LDS: the patch of (2 aside_reach + 3)^2 uint16 levels -- and one of one wave per robot for the release, which reads the side steps just
 * written).  A yielder depends on the yielders below it only, a released robot on the side steps and on the released robots below it:
 * the fixed point is unique, it is the definition's, 2 n_queries sweeps always reach it, and changed == 0 proves it is reached.
 *   restart != 0: derives the roles from the apart workspace and resets the state (nobody moved, nobody released); then n_sweeps sweeps.
 *   restart == 0: n_sweeps more sweeps on work_dev as the previous call on the same arguments left it.
 * Either way the call then writes, for the state it reached, every word of every output for every query:
 *   a robot that moved aside   cells = the side cell c, summary = (l(c), dist[field][c], 0, dist[field][c] == 0)
 *   a released robot           cells = c_r[k'_r], summary = (k'_r, dist[c0] - k'_r, 0, dist[c0] == k'_r)
 *   everyone else              mmd_grid_window_goals_apart's cells and summary
 *   origins_dev, extra_dev     mmd_grid_window_goals_apart's words
 *   aside_dev[q] = (role bits, l): 1 HELD, 2 YIELDS, 4 MOVED, 8 RELEASED; l = 0 unless MOVED; (0, 0) for a query that takes no part
 *   changed_dev[0] = the number of side steps plus the number of k that moved in the call's last sweep (after a restart with
 *                    n_sweeps == 0: the number of queries that take part)
 * Field values are taken as distances in [0, 2^22): the tie on l is broken by min(max(value, 0), 2^22 - 1).
 * The call does not synchronise.  work_dev: mmd_grid_window_aside_work_bytes(n_queries) bytes, 16-byte aligned; a restart initialises it.
 * Error returns, before anything is launched: the ranges of mmd_grid_window_goals_apart; aside_reach outside
 * 1 .. min(reach, MMD_WINDOW_ASIDE_MAX_REACH); aside_steps outside 1 .. MMD_WINDOW_ASIDE_MAX_STEPS; a negative n_sweeps; with
 * n_queries > 0, a NULL dist (with n_fields > 0) or field, a NULL, misaligned or short workspace of either kind, or a NULL output.
 * n_queries == 0 returns 0 and launches nothing.  mmd_grid_window_aside_work_bytes returns 0 for a size the call refuses (and for 0). */
#define MMD_WINDOW_ASIDE_MAX_REACH 63
#define MMD_WINDOW_ASIDE_MAX_STEPS 4095
size_t mmd_grid_window_aside_work_bytes(int n_queries);
int mmd_grid_window_goals_aside(const int32_t* dist_dev, int nx, int ny, int n_fields, const int32_t* field_dev /* [n] */, int n_queries,
                                int reach, int max_steps, int window, int sep, int aside_reach, int aside_steps, int restart, int n_sweeps,
                                const void* apart_work_dev, size_t apart_work_bytes, void* work_dev, size_t work_bytes,
                                int32_t* cells_dev /* [n][2] */, int32_t* origins_dev /* [n][2] */, int32_t* summary_dev /* [n][4] */,
                                int32_t* extra_dev /* [n][2] */, int32_t* aside_dev /* [n][2] */, int32_t* changed_dev /* [1] */,
                                void* stream);

/* World fleets: one window set for a whole run, moved between epochs (csrc/fleet_epoch.hip).
 *
 * mmd_sdf_grid_windows for windows that mostly stay where they are: the same clamped gather, the same arguments and the same words
 * written, but window k is left alone -- no texel loaded, none stored -- where held_dev[k] == origins_dev[k] (both words).  held_dev
 * [n_windows][2]: the origins the slices of windows_dev hold now, device data; NULL: every window is cut.  The call only reads held_dev;
 * it must not be origins_dev's memory written by another launch in flight (the caller keeps two origin buffers, this move's and the
 * last one's).  A workgroup's test is two wave-uniform 8-byte loads.  Error returns, before anything is launched:
 * mmd_sdf_grid_windows'.  n_windows == 0 returns 0 and launches nothing. */
int mmd_sdf_grid_windows_moved(const float* world_grid_dev, int wnx, int wny, const int32_t* origins_dev /* [n][2] */,
                               const int32_t* held_dev /* [n][2] or NULL */, int n_windows, int nx, int ny,
                               float* windows_dev /* [n][nx][ny][4] */, void* stream);

/* Everything a many-robot sampler's state takes from an epoch's targets, from device data alone: one wave per robot, lane = time step.
 * cells_dev, origins_dev, summary_dev: mmd_grid_window_goals' words (any words: they are converted and compared, never used as an
 * index).  points_dev: the robots' current points, robot r's two floats at points_dev + r * points_stride (2 for a packed [n][2]; 128
 * for the last points of paths [n][64][2]; even and at least 2); goal_points_dev [n][2]: their exact goal points; line_a_dev [64]: the
 * line parameters a_t (numpy.linspace(0, 1, 64) in float32).  Per robot r and axis k, every operation rounded once and none contracted:
 *   offsets_dev[r][k]   = (float)(((double)origin * offset_terms[0] + offset_terms[1 + k]) - offset_terms[3 + k])
 *                         -- offset_terms = (cell size, the world's origin x, y, the tile's lower limit x, y), doubles
 *   subgoals_dev[r][k]  = goal_points_dev[r][k] where summary[r][3] == 1, else centre_terms[k] + ((float)cell + 0.5f) * centre_terms[2 + k]
 *                         -- centre_terms = (the world's lower limit x, y, its pitch x, y), floats
 *   hard_first_dev[r]   = normalised (points[r] - offsets[r], 0, 0),  hard_last_dev[r] = normalised (subgoals[r] - offsets[r], 0, 0),
 *                         normalised(x)[c] = ((x[c] - norm_min[c]) / norm_range[c]) * 2 - 1 with a correctly rounded divide
 *   lines_dev[r][t][k]  = points[r][k] * (1 - a_t) + subgoals[r][k] * a_t
 * Every word of the five outputs is written for every robot.  offsets_dev, subgoals_dev and lines_dev are 8-byte aligned, hard_first_dev
 * and hard_last_dev 16-byte aligned, as are the inputs by their rows (cells, origins, points and goal points 8 bytes, summary 16).  Error
 * returns, before anything is launched: a negative n_robots; points_stride odd or below 2; NULL offset_terms, centre_terms, norm_min or
 * norm_range; with n_robots > 0, a NULL or misaligned pointer among the device arguments.  n_robots == 0 returns 0 and launches nothing. */
int mmd_fleet_epoch_frames(const int32_t* cells_dev /* [n][2] */, const int32_t* origins_dev /* [n][2] */,
                           const int32_t* summary_dev /* [n][4] */, const float* points_dev /* [n] rows of points_stride floats */,
                           int points_stride, const float* goal_points_dev /* [n][2] */, int n_robots, const double offset_terms[5],
                           const float centre_terms[4],
                           const float norm_min[4], const float norm_range[4], const float* line_a_dev /* [64] */,
                           float* offsets_dev /* [n][2] */, float* subgoals_dev /* [n][2] */, float* hard_first_dev /* [n][4] */,
                           float* hard_last_dev /* [n][4] */, float* lines_dev /* [n][64][2] */, void* stream);

/* World fleets: the report of a whole run (mmd_amd/fleet_report.py::run_report is the definition on the host: the same integers and the
 * same float32 bits, `length` apart).  paths_dev [n][L][2]: global points, column by column; grid_dev: any texture [nx][ny][4] over
 * lo .. hi; goals_dev [n][2].  A texel is mmd_sdf_grid_lookup's, a value channel 0 of the texel, the norm sqrt(fma(dy, dy, dx * dx)), and
 * every other operation is rounded once.  A point with a coordinate that is not finite is BAD and takes part in nothing else, nor does a
 * segment with a bad end.  Segment t runs from a = p[t] to b = p[t + 1]; its interior points are q_j = a + (b - a) * ((float)j /
 * (float)(n_interp + 1)), j = 1 .. n_interp (an interior point that is not finite is not checked).
 * report_dev, int32 words, MMD_FLEET_REPORT_HEADER + 11 n (+ L with column_conflicts), 8-byte aligned:
 *   header   [0 .. 1] conflict_count, 64 bits: the pairs i < j with ||p_i[t] - p_j[t]|| < rr_margin, summed over the columns t
 *            [2 .. 3] the first conflict, 64 bits: t << 24 | i << 12 | j, the least (t, then i, then j); all ones if there is none
 *            [4] robots_hit  [5] robots_in_conflict  [6] robots_arrived  [7] 0
 *   conflicts [n]        per robot the (t, other robot) in conflict
 *   column_conflicts [L] per column its pairs in conflict; only with column_conflicts == 1
 *   then ten arrays [n]: points_hit (waypoints with value < margin), interp_hit (interior points likewise), first_hit (the least t whose
 *            waypoint or one of whose segment's interior points is hit, -1 if none), bad_points, outside (finite waypoints not in
 *            lo <= p <= hi; they read the clamped border texel and still take part), arrival (the least c with every column t >= c
 *            finite and ||p[t] - goal|| <= goal_tol; L if the last column is not), clear_min (float: the least value over all points
 *            checked in the order of the values' bits, a NaN beyond the infinity of its sign; +inf if there are none), length (float: the
 *            sum of the segment lengths, per lane in column order, then the wave's butterfly), max_step (float: the longest segment, 0 if
 *            there is none), end_error (float: ||p[L - 1] - goal||, the NaN 0x7fc00000 if that point or the goal is bad)
 * One wave per robot for the per-robot words; all pairs of robots on LDS tiles of 32 robots x 64 columns for the conflicts (no n x n
 * buffer); integer atomics only, so every word but `length` is independent of scheduling, and `length` is a fixed order.  The call
 * writes every word it describes and does not synchronise.
 * Error returns, before anything is launched and with the report untouched: n_robots outside 0 .. MMD_FLEET_REPORT_MAX_ROBOTS; length
 * outside 2 .. MMD_FLEET_REPORT_MAX_LENGTH; nx or ny below 1 or above MMD_OCCUPANCY_MAX_SIDE; NULL or non-finite limits or a zero extent;
 * a margin or rr_margin that is not finite; n_interp outside 0 .. MMD_FLEET_REPORT_MAX_INTERP; goal_tol negative or not finite;
 * column_conflicts not 0 or 1; with n_robots > 0, NULL or misaligned paths (8 bytes), grid (16), goals (8) or report (8).
 * n_robots == 0 returns 0, launches nothing and writes nothing. */
#define MMD_FLEET_REPORT_MAX_ROBOTS 4096
#define MMD_FLEET_REPORT_MAX_LENGTH 65535
#define MMD_FLEET_REPORT_MAX_INTERP 63
#define MMD_FLEET_REPORT_HEADER 8
#define MMD_FLEET_REPORT_CONFLICT_COUNT 0
#define MMD_FLEET_REPORT_FIRST_KEY 2
#define MMD_FLEET_REPORT_ROBOTS_HIT 4
#define MMD_FLEET_REPORT_ROBOTS_IN_CONFLICT 5
#define MMD_FLEET_REPORT_ROBOTS_ARRIVED 6
int mmd_fleet_run_report(const float* paths_dev /* [n][L][2] */, int n_robots, int length, const float* grid_dev /* [nx][ny][4] */, int nx,
                         int ny, const float lo[2], const float hi[2], const float* goals_dev /* [n][2] */, float margin, float rr_margin,
                         int n_interp, float goal_tol, int column_conflicts, int32_t* report_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMD_AMD_H */
