"""Data-parallel multi-robot guided sampling: the build's restructuring of the reference's sequential per-robot
planner calls (scripts/inference/inference_multi_agent.py:225-237, cbs.py:316-324) into ONE batched sampling call
per planning round, sharded over GPUs by robot.

Robots are independent inside a sampling call (other robots enter only as frozen constraint points), so
rank g owns robots [g*n_local, (g+1)*n_local) and the only exchange is ONE all-gather per round of the chosen best
paths [n_local, H, 2] -> [N, H, 2] (RCCL over xGMI on GPUs, gloo in the CPU tests), after which every rank rebuilds
its robots' soft-constraint table on device (mmd_soft_constraints_from_paths: N - 1 slots per robot; or, with
constraint_table="binned", mmd_bin_constraints_from_paths: per time step and map cell the robots near the cell -- O(N) work and
memory per round instead of O(N^2), the same bits).  With the cell table the rest of the round is O(N) too: the best-path pick counts
on a cell table of the gathered paths (mmd_count_collisions_binned), and MultiRobotSampler.plan -- rounds until the paths stop
colliding -- reads a device-side conflict report of them (mmd_path_conflicts_binned) at the start of every round.  plan_rounds(repair=True)
also acts on the report: every conflict becomes a hard constraint point of both its robots (constraints.RoundConstraints, built on the
device from the round's collision table), kept over the rounds of the call in front of the soft group, as CBS does down a branch;
plan_rounds(local_rounds=True) re-plans from the previous round's samples with a few noising and denoising steps instead of from noise.
plan_rounds_subset(replan="conflicted" | "independent") re-samples, from round 1 on, only the robots in conflict, or an independent set of them
(multi_agent.select_replan): the others keep their paths and samples bit for bit.  A subset round is an ordinary round of the permuted
instance paths_all[perm], in which the selected robots are a prefix and a rank's selected robots a block of it (replan_round).
Every robot here lives on the model's one tile; world.WorldRobotSampler is the same loop for robots that each carry an offset into a larger world.

How the class is laid out: one sampling call (_run) behind sample, sample_local, replan_round and the loop; three places where a round meets
the other robots, each written once for robots [robot0, robot0 + n) of an instance `paths`, so that the full round and the subset round run
the same code -- the guide table (set_other_paths -> _set_inter_robot_table), the collision cell table (_collision_table, cached, and
replan_round's uncached one -> _build_collision_table) and the pick (best_paths -> _pick -> _in_shared_frame); and the loop
(plan_rounds_subset), whose rounds are _full_round and _subset_round.  _set_inter_robot_table, _build_collision_table and _in_shared_frame are
the hooks a subclass with per-robot frames overrides.
"""
import ctypes as C
from dataclasses import dataclass
from math import ceil

import torch

from . import synth
from .constraints import (VERTEX_CONSTRAINT_RADIUS, RoundConstraints, binned_collision_table, binned_constraints_from_paths,
                          soft_constraints_from_paths)
from .diffusion_model import ddpm_sample_fn
from .guides import GuideManagerTrajectoriesWithVelocity
from .normalization import TrajectoryDatasetFacade

H, D = 64, 4


def shard_range(n_robots, rank, world_size):
    """Contiguous block of robots owned by `rank` (n_robots must divide evenly)."""
    if n_robots % world_size:
        raise ValueError(f"{n_robots} robots do not shard evenly over {world_size} ranks")
    n_local = n_robots // world_size
    return rank * n_local, n_local


def all_gather_paths(paths_local, world_size, group=None, force_collective=False):
    """[n_local,H,2] -> [n_local*world_size,H,2], rank-major (== robot order).  One collective per planning round.
    `force_collective` runs the collective even in a one-rank group (the hardware test of the RCCL branch)."""
    import torch.distributed as dist
    if world_size == 1 and not force_collective:
        # a single-rank sampler never issues a collective, whether or not a (larger) process group exists around it
        return paths_local
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("all_gather_paths: world_size > 1 needs an initialised torch.distributed process group")
    if dist.get_world_size(group) != world_size:
        raise ValueError(f"all_gather_paths: world_size={world_size} but the process group has "
                         f"{dist.get_world_size(group)} ranks")
    if paths_local.is_cuda and dist.get_backend(group) == "gloo":
        # gloo has no device collectives: stage through the host (CPU tests / single-GPU rehearsal of the N>1 path)
        parts = [torch.empty_like(paths_local, device="cpu") for _ in range(world_size)]
        dist.all_gather(parts, paths_local.cpu().contiguous(), group=group)
        return torch.cat(parts, dim=0).to(paths_local.device)
    out = torch.empty((world_size * paths_local.shape[0],) + tuple(paths_local.shape[1:]), dtype=paths_local.dtype,
                      device=paths_local.device)
    dist.all_gather_into_tensor(out, paths_local.contiguous(), group=group)
    return out


@dataclass
class PlanResult:
    """What MultiRobotSampler.plan / plan_rounds return."""
    paths_local: torch.Tensor        # [n_local, H, 2] un-normalised best paths of this rank's robots
    trajs: torch.Tensor              # [n_local * B, H, D] normalised samples of the last round run (None: no round was run)
    n_rounds: int                    # sampling rounds run
    conflict_counts: list            # one int per conflict report: at the start of every round run, then of the returned paths
    robot_counts: torch.Tensor       # int32 [N] on the device: (t, other robot) collisions of every robot, of the returned paths
    conflict_free: bool              # conflict_counts[-1] == 0
    first_conflict: tuple            # (t, a, b, pa, pb, mid) of the returned paths' first conflict, or None
    # plan_rounds(repair=True): int32 [n_local] on the device, hard points that found their block full; world.WorldRobotSampler: the
    # framed table's dropped points of the last round
    dropped_constraints: torch.Tensor = None
    # plan_rounds_subset(replan != "all"): the robots sampled per round run, over all ranks ([N, n_selected, ...]), else None.  Set on the
    # result, not a field: the positional layout of the fields above is what callers construct
    replanned_counts = None


class _RoundPickRequest:
    """A round's mmd_round_pick and the tensors it points at (MultiRobotSampler._round_pick_request)."""
    __slots__ = ("struct", "paths", "idx", "n_free", "scratch", "paths_all", "alpha")


class MultiRobotSampler:
    def __init__(self, model, starts, goals, env_id="EnvEmpty2D", n_samples=64, rank=0, world_size=1,
                 norm_mins=synth.NORM_MINS, norm_maxs=synth.NORM_MAXS, n_guide_steps=20,
                 start_guide_steps_fraction=0.5, n_diffusion_steps_without_noise=1,
                 weight_grad_cost_soft_constraints=2e-2, radius=VERTEX_CONSTRAINT_RADIUS, device="cuda", group=None,
                 n_streams=0, inter_robot=True, constraint_table="dense"):
        if constraint_table not in ("dense", "binned"):
            raise ValueError(f"constraint_table must be 'dense' or 'binned', got {constraint_table!r}")
        # "dense": the all-pairs table; "binned": the cell table (constraints.binned_constraints_from_paths), for rounds of hundreds of robots
        self.constraint_table = constraint_table
        self.model = model
        self.n_robots = starts.shape[0]
        self.rank, self.world_size, self.group = rank, world_size, group
        self.robot0, self.n_local = shard_range(self.n_robots, rank, world_size)
        self.n_samples = n_samples
        self.device = torch.device(device)
        self.dataset = TrajectoryDatasetFacade(norm_mins, norm_maxs)
        self.env_id = env_id
        self.guide = GuideManagerTrajectoriesWithVelocity(self.dataset, env_id=env_id, n_robots=self.n_local,
                                                          robot_env_ids=self._robot_env_ids(self.robot0, self.n_local), device=device,
                                                          window_set=self._robot_window_set())
        self._subset_guides = {}        # replan_round: a guide per subset size, on the same map (the resident SDF texture is shared)
        sl = slice(self.robot0, self.robot0 + self.n_local)
        self._ends = (starts[sl], goals[sl])      # plan(): the straight lines the first round starts from
        st = torch.as_tensor(starts[sl], dtype=torch.float32)
        go = torch.as_tensor(goals[sl], dtype=torch.float32)
        z = torch.zeros_like(st)
        nz = self.dataset.normalizer
        self.hard_conds = {0: nz.normalize(torch.cat((st, z), -1)).to(self.device),
                           H - 1: nz.normalize(torch.cat((go, z), -1)).to(self.device)}
        self.n_guide_steps = n_guide_steps
        self.t_start_guide = ceil(start_guide_steps_fraction * model.n_diffusion_steps)
        self.n_extra = n_diffusion_steps_without_noise
        self.w_soft, self.radius = weight_grad_cost_soft_constraints, radius
        self.n_streams = n_streams      # mmd_sampler_desc.n_streams (0 = the library's choice: 2 chunks above 512 trajectories)
        # False: no inter-robot term (BASELINE config 2: every robot guided by the map, the workspace and the GP prior alone) --
        # plan_round then needs no exchange step either
        self.inter_robot = inter_robot
        self._collision = None          # "binned": (paths_all, its collision table), kept from set_other_paths for best_paths
        self.round_constraints = None   # plan_rounds(repair=True): the call's constraints.RoundConstraints
        self.last_idx = self.last_n_free = None     # best_paths: the pick per local robot and how many of its samples were free
        self.last_conflict_list = None              # plan(list_cap > 0): the first records of the final report

    # ---- the three places where a round meets the other robots: each takes (paths, robot0, n), so that the full round and the subset
    # ---- round (replan_round) run the same code; a subclass with frames (world.WorldRobotSampler) overrides only the three hooks, and
    # ---- _robot_env_ids where its robots read maps of their own
    def _robot_env_ids(self, robot0, n):
        """hook: the map names of robots [robot0, robot0 + n) for a guide's robot_env_ids, or None: every robot on the sampler's env_id"""
        return None

    def _robot_window_set(self):
        """hook: a window set of the local robots' own (map_textures.WorldWindowSet) for the guide, in place of map names, or None"""
        return None

    def _build_collision_table(self, paths, robot0, n):
        """hook: the collision cell table (every time step listed) of `paths` [N, H, 2] (contiguous) for robots [robot0, robot0 + n)"""
        return binned_collision_table(paths, robot0, n, self.radius)

    def _collision_table(self, paths_all):
        """The collision cell table of paths_all (every time step listed): built once per round, by set_other_paths or by the first
        best_paths that needs it."""
        if self._collision is None or self._collision[0] is not paths_all:
            self._collision = (paths_all, self._build_collision_table(paths_all.contiguous(), self.robot0, self.n_local))
        return self._collision[1]

    def _report_on_own_table(self):
        """Whether plan()'s conflict report reads this sampler's _collision_table (a subclass whose table is not the default one:
        world.WorldRobotSampler) instead of the default table multi_agent.path_conflicts builds for itself.  The same integers either way."""
        return False

    def set_other_paths(self, paths_all):
        """paths_all [N,H,2] un-normalised best paths of ALL robots (this device) or None (no inter-robot term).  With the cell table
        the collision table of the same paths is built here too and kept for best_paths (which rebuilds it for another tensor: do not
        modify paths_all in place in between)."""
        self._collision = None
        if paths_all is None or self.n_robots < 2:
            self.guide.reset_extra_costs()
            return
        self._set_inter_robot_table(self.guide, paths_all.contiguous(), self.robot0, self.n_local)
        if self.constraint_table == "binned":
            self._collision_table(paths_all)

    def _set_inter_robot_table(self, guide, paths, robot0, n):
        """hook: the inter-robot table of `paths` [N, H, 2] (contiguous) for robots [robot0, robot0 + n) on `guide`, in place of whatever
        constraints it had: the cell table or the all-pairs table, by constraint_table, with the sampler's radius and weight."""
        guide.reset_extra_costs()
        if self.constraint_table == "binned":
            guide.set_binned_constraints(binned_constraints_from_paths(paths, robot0, n, self.radius, self.w_soft))
        else:
            guide.set_packed_constraints(soft_constraints_from_paths(paths, robot0, n, self.radius, self.w_soft))

    def sample(self, seed=None, x_init=None, step_noise=None, return_chain=False):
        """One guided sampling round for the local robots: [n_local*B, H, D] normalised trajectories.  The in-kernel
        Philox noise is keyed by (seed, global trajectory index): every rank passes the SAME seed and gets exactly the
        rows the unsharded run would produce."""
        return self._run(self.hard_conds, self.n_local, self.guide, self.robot0, seed, x_init=x_init, step_noise=step_noise,
                         return_chain=return_chain)

    def sample_local(self, prev_trajs, n_noising_steps=3, n_denoising_steps=3, seed=None):
        """A local re-plan round (the X-variants of CBS, cbs.py:424-430, mpd.py:460-517): forward-noise the previous round's normalised
        samples prev_trajs [n_local*B, H, D] n_noising_steps, then n_denoising_steps guided steps (+ the steps without noise) instead
        of the whole loop from noise.  Both draws are keyed by (seed, global trajectory index), as in `sample`."""
        return self._run(self.hard_conds, self.n_local, self.guide, self.robot0, seed, prev_trajs, n_noising_steps, n_denoising_steps)

    def _run(self, hard_conds, n_robots, guide, robot0, seed, prev_trajs=None, n_noising_steps=3, n_denoising_steps=3, x_init=None,
             step_noise=None, return_chain=False, round_pick=None):
        """The one sampling call, for robots [robot0, robot0 + n_robots) of an instance with their hard conditions and their guide:
        `sample` (from noise, or from x_init) when prev_trajs is None, else `sample_local` from prev_trajs [n_robots * B, H, D].
        round_pick (_round_pick_request): the call also picks these robots' best samples (_sample_and_pick)"""
        shared = dict(n_samples=self.n_samples, n_robots=n_robots, horizon=H, sample_fn=ddpm_sample_fn, guide=guide,
                      n_guide_steps=self.n_guide_steps, t_start_guide=self.t_start_guide, noise_std_extra_schedule_fn=lambda t: 0.5,
                      n_diffusion_steps_without_noise=self.n_extra, seed=seed, traj_index_base=robot0 * self.n_samples,
                      device=self.device, n_streams=self.n_streams)
        if round_pick is not None:
            shared["round_pick"] = round_pick
        if prev_trajs is None:
            return self.model.run_inference(None, hard_conds, return_chain=return_chain, warm_start_path_b=x_init, step_noise=step_noise,
                                            **shared)
        return self.model.run_local_inference(prev_trajs, n_noising_steps, n_denoising_steps, None, hard_conds, **shared)

    def unnormalize(self, trajs_normalized):
        nz = self.dataset.normalizer
        mins, maxs = nz.mins.to(trajs_normalized.device), nz.maxs.to(trajs_normalized.device)
        return (torch.clip(trajs_normalized, -1, 1) + 1) / 2.0 * (maxs - mins) + mins

    def best_paths(self, trajs_normalized, paths_all=None, collision_table=None):
        """Selection for the exchange step, on the device: samples that collide with the map or leave the joint limits
        are dropped first (PlanningTask.get_trajs_collision_and_free, tasks.py:236-311, as MPD.__call__ does at
        mpd.py:357-382); among the free ones the pick is the first sample with the fewest robot-robot collisions against
        the other robots' current best paths (CBS 'least_collisions', cbs.py:446-458; with constraint_table="binned" counted on a cell
        table of paths_all, the same counts), or the cheapest one (path length +
        smoothness, mpd.py:366-370) when no paths are known yet.  A robot without any free sample falls back to the same
        criterion over all its samples (`self.last_n_free` tells).  collision_table: a collision cell table of paths_all the caller
        already has (plan_rounds(repair=True)): the counts are read from it.  Returns un-normalised positions [n_local,H,2]."""
        if collision_table is None and paths_all is not None and self.n_robots >= 2 and self.constraint_table == "binned":
            collision_table = self._collision_table(paths_all)     # the same integers from the cell lists instead of all N robots
        paths, self.last_idx, self.last_n_free = self._pick(trajs_normalized, self.guide, self.robot0, self.n_local, paths_all,
                                                            collision_table)
        return paths

    def _pick(self, trajs_normalized, guide, robot0, n_robots, paths_all, collision_table):
        """`best_paths` for robots [robot0, robot0 + n_robots) of the instance paths_all -> (paths [n_robots, H, 2], idx, n_free); the
        counts come from collision_table (a cell table of paths_all for these robots) where one is given, else from paths_all.  The map
        and the joint limits are checked in the robots' own frame; the collisions are counted, and the picks returned, in the frame the
        robots share (_in_shared_frame)"""
        from . import postprocess as post
        t = self.unnormalize(trajs_normalized).contiguous()
        r = post.postprocess_batch(guide, t, n_robots=n_robots, smooth=False)
        t = self._in_shared_frame(t, robot0, n_robots)
        if paths_all is None or self.n_robots < 2:
            idx, n_free = post.select_best(r.free_mask, n_robots, cost_a=r.path_length, cost_b=r.smoothness)
        else:
            from .multi_agent import count_collisions, count_collisions_binned
            if collision_table is not None:
                counts = count_collisions_binned(t, collision_table, n_robots)
            else:
                counts = count_collisions(t, paths_all, robot0, n_robots)
            idx, n_free = post.select_best(r.free_mask, n_robots, counts=counts.view(-1))
        tv = t.view(n_robots, self.n_samples, H, D)
        return tv[torch.arange(n_robots, device=t.device), idx.long()][..., :2].contiguous(), idx, n_free

    def _in_shared_frame(self, t, robot0, n_robots):
        """hook: the un-normalised samples t [n_robots * B, H, D] (contiguous) of robots [robot0, robot0 + n_robots) in the frame the
        robots share.  Here every robot lives in that frame: t itself, no copy and no launch"""
        return t

    # ---- a full round's sampling and pick: one native call (mmd_p_sample_loop_pick) where the round is the plain one ----
    _native_pick = True         # private switch: False keeps every round on sample + best_paths (the A/B of tests/test_gpu_round_pick.py)

    def _takes_native_pick(self, collision_table):
        """THE place that says which full rounds sample and pick in one native call: the dense table, no collision table handed in
        (plan_rounds(repair=True) counts on its own), and the sampling, the pick and the frame all the base class's -- a subclass that
        overrides any of them (world.WorldRobotSampler: per-robot frames) keeps sample + best_paths, as do the cell-table rounds, the
        repair rounds and the subset rounds (replan_round)."""
        cls, base = type(self), MultiRobotSampler
        own = ("_in_shared_frame", "_pick", "best_paths", "unnormalize", "sample", "sample_local", "_run")
        return (self._native_pick and self.constraint_table == "dense" and collision_table is None
                and getattr(self.model, "takes_round_pick", False)          # (a model whose p_sample_loop knows the request)
                and all(getattr(cls, name) is getattr(base, name) for name in own))

    def _round_pick_request(self, paths_all):
        """The mmd_round_pick of this rank's robots against paths_all (None, or fewer than two robots: the cost rule), with fresh outputs:
        .paths [n_local, H, 2], .idx, .n_free (what _pick returns), .struct for the call.  Everything the struct points at is held here."""
        from . import _lib, postprocess as post
        from .multi_agent import RR_MARGIN
        n, dev = self.n_local * self.n_samples, self.device
        rp = _RoundPickRequest()
        rp.paths = torch.empty((self.n_local, H, 2), dtype=torch.float32, device=dev)
        rp.idx = torch.empty(self.n_local, dtype=torch.int32, device=dev)
        rp.n_free = torch.empty(self.n_local, dtype=torch.int32, device=dev)
        rp.scratch = torch.empty(2 * n, dtype=torch.float32, device=dev)
        rp.paths_all = paths_all.contiguous() if paths_all is not None and self.n_robots >= 2 else None
        host = getattr(self, "_pick_host", None)
        if host is None:            # once per sampler: the normaliser's limits on the host, postprocess_batch's default alpha table (as _pick calls it)
            nz = self.dataset.normalizer
            host = self._pick_host = ([float(v) for v in nz.mins.float().cpu()], [float(v) for v in nz.maxs.float().cpu()],
                                      post.interpolation_alphas(5))
        rp.alpha = host[2]
        s = rp.struct = _lib.RoundPick()
        s.paths_all_dev = rp.paths_all.data_ptr() if rp.paths_all is not None else None
        s.n_all, s.robot0 = self.n_robots, self.robot0
        s.norm_min, s.norm_max = (C.c_float * 4)(*host[0]), (C.c_float * 4)(*host[1])
        s.num_interpolation, s.alpha = len(rp.alpha), rp.alpha.ctypes.data_as(C.POINTER(C.c_float))
        s.margin, s.rr_margin = post.ROBOT_RADIUS, RR_MARGIN
        s.q_min, s.q_max = (C.c_float * 2)(*post.Q_MIN), (C.c_float * 2)(*post.Q_MAX)
        s.paths_out_dev, s.idx_out_dev, s.n_free_out_dev = rp.paths.data_ptr(), rp.idx.data_ptr(), rp.n_free.data_ptr()
        s.scratch_dev = rp.scratch.data_ptr()
        return rp

    def _pick_native(self, trajs_normalized, paths_all=None):
        """_pick of this rank's robots on the dense table as the one native pass alone (mmd_round_pick_paths) -> (paths, idx, n_free),
        the same bits; what _sample_and_pick's call enqueues behind the sampling loop."""
        from . import _lib
        rp = self._round_pick_request(paths_all)
        _lib.launch("mmd_round_pick_paths", trajs_normalized, C.byref(self.guide.desc()), C.byref(rp.struct),
                    _lib.require_gpu(trajs_normalized, "trajs_normalized"), self.n_local, self.n_samples)
        return rp.paths, rp.idx, rp.n_free

    def _sample_and_pick(self, others, collision_table, seed, prev_trajs=None, n_noising_steps=3, n_denoising_steps=3):
        """A full round's sampling (from noise, or from prev_trajs as sample_local does) and its pick -> (trajs, paths_local), with
        last_idx / last_n_free filled: one native call where _takes_native_pick says so, else sample / sample_local + best_paths."""
        if self._takes_native_pick(collision_table):
            rp = self._round_pick_request(others)
            trajs = self._run(self.hard_conds, self.n_local, self.guide, self.robot0, seed, prev_trajs, n_noising_steps, n_denoising_steps,
                              round_pick=rp)
            self.last_idx, self.last_n_free = rp.idx, rp.n_free
            return trajs, rp.paths
        if prev_trajs is None:
            trajs = self.sample(seed=seed)              # (the public methods: a subclass may put its own sampling there)
        else:
            trajs = self.sample_local(prev_trajs, n_noising_steps, n_denoising_steps, seed=seed)
        return trajs, self.best_paths(trajs, others, collision_table=collision_table)

    def plan_round(self, paths_local, seed=None):
        """all-gather -> constraint table -> guided sampling -> new local best paths."""
        paths_all = all_gather_paths(paths_local, self.world_size, self.group) if self.inter_robot else None
        self.set_other_paths(paths_all)
        return self._sample_and_pick(paths_all, None, seed)

    def _subset_guide(self, n_robots):
        """the guide of a subset round: n_robots robots on the sampler's map, kept by size; `self.guide` and its tables are not touched"""
        g = self._subset_guides.get(n_robots)
        if g is None:
            g = self._subset_guides[n_robots] = GuideManagerTrajectoriesWithVelocity(self.dataset, env_id=self.env_id, n_robots=n_robots,
                                                                                     robot_env_ids=self._robot_env_ids(self.robot0, n_robots),
                                                                                     device=self.device)
        return g

    def selected_local_ids(self, selection):
        """int64 device tensor: this rank's selected robots, as indices into its own robots, ascending.  `selection` is
        multi_agent.select_replan's for this rank's shard (a collision table of robot0 = self.robot0, n_local = self.n_local)."""
        _, sel_before, n_sel_local, _ = selection.read_header()
        return selection.perm[sel_before:sel_before + n_sel_local].long() - self.robot0

    def replan_round(self, paths_all, selection, seed, prev_trajs=None, n_noising_steps=3, n_denoising_steps=3):
        """plan_round for this rank's SELECTED robots only (multi_agent.select_replan on this rank's collision table of paths_all), the
        other robots' paths held: the round of the permuted instance paths_all[perm], in which the selected robots are the prefix and
        this rank's the block [sel_before, sel_before + n_sel_local) -- the table (dense or cell) on the permuted paths, sampling with
        the global trajectory index sel_before * B (from noise, or with prev_trajs, the selected robots' [n_sel_local * B, H, D] rows,
        as sample_local does), the pick against the permuted paths.  The rows are those the full round of the permuted instance gives
        these robots, whatever the sharding.  -> (trajs_sub [n_sel_local * B, H, D], best_sub [n_sel_local, H, 2], local_ids: the
        selected robots as indices into this rank's robots, on the device).  Nothing selected here: no launch, empty tensors."""
        _, sel_before, n_sel, _ = selection.read_header()
        local_ids = self.selected_local_ids(selection)
        if n_sel == 0:
            return (torch.empty((0, H, D), dtype=torch.float32, device=self.device),
                    torch.empty((0, H, 2), dtype=torch.float32, device=self.device), local_ids)
        paths_perm = paths_all.index_select(0, selection.perm.long()).contiguous()
        hard_conds = {row: v.index_select(0, local_ids) for row, v in self.hard_conds.items()}
        guide = self._subset_guide(n_sel)
        self._set_inter_robot_table(guide, paths_perm, sel_before, n_sel)
        # (a table of its own, not cached: _collision stays the caller's)
        table = self._build_collision_table(paths_perm, sel_before, n_sel) if self.constraint_table == "binned" else None
        trajs = self._run(hard_conds, n_sel, guide, sel_before, seed, prev_trajs, n_noising_steps, n_denoising_steps)
        best, idx, n_free = self._pick(trajs, guide, sel_before, n_sel, paths_perm, table)
        if self.last_idx is not None and self.last_idx.shape[0] == self.n_local:
            # the robots not re-planned keep their entries
            self.last_idx = self.last_idx.clone().index_copy_(0, local_ids, idx.to(self.last_idx.dtype))
            self.last_n_free = self.last_n_free.clone().index_copy_(0, local_ids, n_free.to(self.last_n_free.dtype))
        return trajs, best, local_ids

    def _run_device(self):
        """the device the samples live on: self.device with its index resolved ("cuda" is the current device)"""
        d = self.device
        return torch.device(d.type, torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d

    def plan(self, paths_local=None, max_rounds=8, seed=0, list_cap=0):
        """Rounds of plan_round until the gathered best paths are free of robot-robot conflicts, at most max_rounds of them.  Round k
        (seed + k): all-gather the paths, report their conflicts on the device (multi_agent.path_conflicts; the count crosses in one
        device -> host copy, the only synchronisation the loop adds), stop if k > 0 and there are none or if k == max_rounds, else
        build the table(s), sample and pick.  After the last round run, the returned paths are gathered once more for the final report:
        conflict_free, robot_counts and first_conflict describe what is returned.  Every rank computes the same report from the same
        gathered paths, so the ranks stop together without another collective.  paths_local defaults to this rank's straight lines
        start -> goal.  list_cap > 0 also keeps the first records of the final report (`self.last_conflict_list`, [list_cap, 12] words).
        plan_rounds is the same loop with the opt-in ways to act on the report.  -> PlanResult."""
        return self.plan_rounds(paths_local, max_rounds, seed, list_cap)

    def plan_rounds(self, paths_local=None, max_rounds=8, seed=0, list_cap=0, repair=False, hard_slots=32,
                    weight_grad_cost_constraints=2e-1, t_pad=2, local_rounds=False, n_noising_steps=3, n_denoising_steps=3):
        """plan()'s loop -- with repair and local_rounds off, exactly plan() -- and two independent ways to act on the report (below);
        plan_rounds_subset is this call with a third, the choice of the robots a round re-plans, and plan_rounds_seeded any of them with
        round 0 started from given trajectories.  -> PlanResult."""
        return MultiRobotSampler.plan_rounds_subset(self, paths_local, max_rounds, seed, list_cap, repair, hard_slots,
                                                    weight_grad_cost_constraints, t_pad, local_rounds, n_noising_steps, n_denoising_steps)

    def plan_rounds_seeded(self, init_trajs, paths_local=None, max_rounds=8, seed=0, list_cap=0, repair=False, hard_slots=32,
                           weight_grad_cost_constraints=2e-1, t_pad=2, local_rounds=False, n_noising_steps=3, n_denoising_steps=3,
                           replan="all", independent_iters=8):
        """plan_rounds_subset (this sampler's: a subclass's refusals and results hold) whose round 0 starts from given trajectories.
        init_trajs: normalised trajectories [n_local * B, H, D] (float32, contiguous, on the sampler's device): round 0 samples with
        sample_local(init_trajs, n_noising_steps, n_denoising_steps, seed) instead of sample(seed) from noise.  Later rounds are what
        they are without it: from noise, or with local_rounds=True from the round before.  paths_local is still what round 0's tables
        are built on (a caller with seed trajectories passes their positions).  init_trajs=None is plan_rounds_subset, bit for bit; a
        wrong type, shape, dtype, device or layout raises ValueError before any launch.  -> PlanResult."""
        if init_trajs is not None:
            want = (self.n_local * self.n_samples, H, D)
            if not (isinstance(init_trajs, torch.Tensor) and tuple(init_trajs.shape) == want and init_trajs.dtype == torch.float32
                    and init_trajs.device == self._run_device() and init_trajs.is_contiguous()):
                got = (tuple(init_trajs.shape), init_trajs.dtype, init_trajs.device) if isinstance(init_trajs, torch.Tensor) else type(init_trajs)
                raise ValueError(f"plan_rounds_seeded: init_trajs must be a contiguous float32 tensor {want} on {self._run_device()}, got {got}")
        self._init_trajs = init_trajs              # read by the loop's round 0 only, and only during this call
        try:
            return self.plan_rounds_subset(paths_local, max_rounds, seed, list_cap, repair, hard_slots, weight_grad_cost_constraints, t_pad,
                                           local_rounds, n_noising_steps, n_denoising_steps, replan, independent_iters)
        finally:
            self._init_trajs = None

    def plan_rounds_subset(self, paths_local=None, max_rounds=8, seed=0, list_cap=0, repair=False, hard_slots=32,
                           weight_grad_cost_constraints=2e-1, t_pad=2, local_rounds=False, n_noising_steps=3, n_denoising_steps=3,
                           replan="all", independent_iters=8):
        """plan()'s loop -- with repair and local_rounds off and replan="all", exactly plan() -- and three ways to act on the report.

        repair=True (convert_conflicts_to_constraints, mmd/common/conflict_conversion.py:41-55; cbs.py:407-413): the round's collision
        cell table is built once and serves the report, the pick and the hard points -- every record (t, a, b, mid) gives a and b the
        point mid, the constraint radius, range (t - t_pad, t + t_pad), in a hard group of weight weight_grad_cost_constraints and at
        most hard_slots points per time step, in front of the soft group.  The hard group accumulates over the rounds of this call
        (`self.round_constraints`; PlanResult.dropped_constraints counts the points that found it full).  It needs the dense table with
        the inter-robot term: constraint_table="binned" or inter_robot=False raise.
        local_rounds=True: rounds k >= 1 re-plan from round k - 1's samples (sample_local: n_noising_steps forward, n_denoising_steps
        back) instead of from noise.
        replan: which robots a round k >= 1 samples (round 0 samples every robot: straight lines are not samples).  "all": every robot.
        "conflicted": the robots of the report's conflicts.  "independent": an independent set of the conflict graph, independent_iters
        iterations of multi_agent.select_replan -- every re-planned robot is guided against neighbours that keep their paths this
        round.  Such a round builds its collision table once, selects on the device, reads the selection's 16-byte header (the one
        device -> host copy it adds) and runs replan_round; robots not selected keep their path, their samples and their last_idx /
        last_n_free entries bit for bit.  Every rank computes the same selection from the same gathered paths: no new collective, and a
        rank with nothing selected still takes part in the all-gather.  PlanResult.replanned_counts lists the robots sampled per
        round.  It needs the inter-robot term and does not combine with repair (the round table is laid out per local robot and does
        not follow a permutation).  -> PlanResult."""
        from .multi_agent import path_conflicts, read_summary
        if replan not in ("all", "conflicted", "independent"):
            raise ValueError(f"plan_rounds_subset: replan must be 'all', 'conflicted' or 'independent', got {replan!r}")
        subset = replan != "all"
        if subset and not self.inter_robot:
            raise ValueError(f"plan_rounds_subset(replan={replan!r}) needs inter_robot=True: without the inter-robot term no robot is in conflict with another")
        if subset and repair:
            raise ValueError(f"plan_rounds_subset(replan={replan!r}) does not combine with repair=True: the round table is laid out per local robot "
                             "and does not follow a permutation")
        if repair and (self.constraint_table == "binned" or not self.inter_robot):
            raise ValueError("plan_rounds(repair=True) needs constraint_table='dense' and inter_robot=True: the library takes hard groups only in "
                             "the dense table, not next to a cell table")
        if paths_local is None:
            import numpy as np
            st, go = (np.asarray(torch.as_tensor(v).cpu().numpy(), dtype=np.float32) for v in self._ends)
            paths_local = torch.from_numpy(synth.straight_line_paths(st, go, H)).to(self.device)
        rc = None
        if repair and self.n_robots >= 2:
            rc = self.round_constraints = RoundConstraints(self.n_robots, self.robot0, self.n_local, hard_slots, self.radius,
                                                           weight_grad_cost_constraints, self.w_soft, device=self.device)
        trajs, counts, k = None, [], 0
        replanned = [] if subset else None
        while True:
            paths_all = all_gather_paths(paths_local, self.world_size, self.group).contiguous()
            select = subset and k > 0 and self.n_robots >= 2
            # one table a round: report, hard points, pick; or report and selection
            table = self._collision_table(paths_all) if rc is not None or select or self._report_on_own_table() else None
            summ, robots, lst = path_conflicts(paths_all, list_cap=list_cap, table=table)
            count, first = read_summary(summ)
            counts.append(count)
            if k == max_rounds or (k > 0 and count == 0):
                break
            if select:
                paths_local, n_sampled = self._subset_round(paths_all, table, robots, replan, independent_iters, seed + k, paths_local, trajs,
                                                            local_rounds, n_noising_steps, n_denoising_steps)
            else:
                prev = getattr(self, "_init_trajs", None) if k == 0 else trajs if local_rounds else None      # (plan_rounds_seeded's)
                trajs, paths_local = self._full_round(paths_all, table, rc, t_pad, seed + k, prev, n_noising_steps, n_denoising_steps)
                n_sampled = self.n_robots
                if subset:
                    trajs = trajs.clone()       # the buffer later rounds scatter into (and not a view of the sampling chain)
            if subset:
                replanned.append(n_sampled)
            k += 1
        self.last_conflict_list = lst
        res = PlanResult(paths_local, trajs, k, counts, robots, count == 0, first, rc.dropped if rc is not None else None)
        res.replanned_counts = replanned
        return res

    def _full_round(self, paths_all, table, rc, t_pad, seed, prev_trajs, n_noising_steps, n_denoising_steps):
        """A round of the loop that samples every local robot: the inter-robot table of paths_all, or with rc (repair) the round's
        conflicts (read off `table`) as hard points in front of it; sampling from noise, or from prev_trajs as sample_local does; the
        pick (counted on `table` where there is one) -> (trajs, paths_local)"""
        others = paths_all if self.inter_robot else None
        if rc is not None:
            rc.append_conflicts(paths_all, table, t_pad=t_pad)
            rc.set_soft(paths_all)
            self.guide.set_packed_constraints(rc.tensors())
        else:
            self.set_other_paths(others)
        return self._sample_and_pick(others, table, seed, prev_trajs, n_noising_steps, n_denoising_steps)

    def _subset_round(self, paths_all, table, robot_counts, replan, independent_iters, seed, paths_local, trajs, local_rounds,
                      n_noising_steps, n_denoising_steps):
        """A round of the loop that samples only the robots multi_agent.select_replan selects from the round's table and report
        (replan_round; with local_rounds from their rows of trajs, else from noise) and scatters their samples into trajs
        [n_local * B, H, D], in place, and their picks into a copy of paths_local -> (paths_local, robots selected over all ranks)"""
        from .multi_agent import select_replan
        B = self.n_samples
        selection = select_replan(paths_all, table, robot_counts, replan, independent_iters)
        n_selected = selection.read_header()[0]
        ids = self.selected_local_ids(selection)
        prev = trajs.view(self.n_local, B, H, D).index_select(0, ids).view(-1, H, D) if local_rounds else None
        trajs_sub, best_sub, ids = self.replan_round(paths_all, selection, seed, prev, n_noising_steps, n_denoising_steps)
        if ids.numel():
            paths_local = paths_local.clone().index_copy_(0, ids, best_sub)       # (paths_all may be this very tensor)
            trajs.view(self.n_local, B, H, D).index_copy_(0, ids, trajs_sub.view(-1, B, H, D))
        self._collision = None
        return paths_local, n_selected
