"""Many-robot rounds in a world larger than one tile: per-robot frames.

The model plans on its own tile, [-1, 1]^2 (the span of the normaliser); MultiRobotSampler puts every robot on that one tile.  Here robot
r plans in that same frame but carries an offset that places its window in a global frame -- global = local + offset[r] -- and the robots
interact in the global frame: starts, goals, the gathered best paths, the pick's collision counts and the conflict report are all global.
Nothing of the model or the guided step changes (translation invariance is what the method already relies on when it composes tile
models); the only new device code is the framed all-pairs table (constraints.framed_constraints_from_paths,
mmd_framed_constraints_from_paths): robot r's block holds the other robots' points, shifted into r's frame, that fall into r's window
widened by 1.0625 x the constraint radius.  A trajectory is clipped to the normaliser's limits, so a point outside that window can never
act on it: the table is exact and its size follows the local density, not N.

WorldRobotSampler is MultiRobotSampler with the frame put into the three hooks through which a round meets the other robots: the guide
table (_set_inter_robot_table: the framed table), the collision cell table (_build_collision_table: laid over the world's limits) and the
samples the pick counts and returns (_in_shared_frame: positions + offset).  Every method body, the loop included, is the base class's.
"""
import numpy as np
import torch

from . import synth
from .constraints import (BIN_CELL_SLACK, VERTEX_CONSTRAINT_RADIUS, binned_collision_table, framed_constraints_from_paths,
                          framed_slot_bound)
from . import environments, map_textures
from .environments import LIMITS, map_has_obstacles, map_sdf
from .multi_robot import D, H, MultiRobotSampler, shard_range

WORLD_MAX_CELLS = 64             # per axis: what the library takes for a cell table (the default grid of constraints.bin_grid stops at 32)
TILE_PITCH = 2.0                 # the side of a tile: window origins on maps with obstacles are multiples of it
OBSTACLE_MARGIN = 0.16           # trials.get_start_goal_pos_random_in_env's obstacle_margin


def _f32(a, what, n=None):
    a = np.ascontiguousarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2 or (n is not None and a.shape[0] != n):
        raise ValueError(f"WorldRobotSampler: {what} must be [{'N' if n is None else n}, 2], got {a.shape}")
    return a


def world_limits(offsets, limits=LIMITS):
    """(lo, hi) of the box that holds every robot's window: the collision cell table of a world is laid over it"""
    off = np.asarray(offsets, dtype=np.float64).reshape(-1, 2)
    return (tuple(float(off[:, k].min() + limits[0][k]) for k in range(2)), tuple(float(off[:, k].max() + limits[1][k]) for k in range(2)))


def world_grid(limits, radius):
    """(nx, ny): the finest grid over `limits`, up to 64 cells per axis, whose cells are at least (1 + 1/16) x radius wide"""
    n = []
    for k in range(2):
        cells = min(WORLD_MAX_CELLS, int(np.floor((float(limits[1][k]) - float(limits[0][k])) / (BIN_CELL_SLACK * float(radius)))))
        if cells < 1:
            raise ValueError(f"world_grid: axis {k} cannot hold a cell of {BIN_CELL_SLACK} x radius")
        n.append(cells)
    return tuple(n)


def _checked_ends(starts, goals, offsets, lo, hi):
    """(starts, goals, offsets, local starts, local goals), float32 [N, 2] on the host: the one validation of WorldRobotSampler's
    constructor and of its move; lo, hi: the normaliser's position limits"""
    starts, goals, offsets = _f32(starts, "starts"), _f32(goals, "goals"), _f32(offsets, "offsets")
    n = starts.shape[0]
    if goals.shape[0] != n or offsets.shape[0] != n:
        raise ValueError(f"WorldRobotSampler: {n} starts, {goals.shape[0]} goals, {offsets.shape[0]} offsets")
    local_starts, local_goals = starts - offsets, goals - offsets                      # one fp32 subtraction per axis
    for name, p in (("start", local_starts), ("goal", local_goals)):
        bad = np.flatnonzero(~np.all((p >= lo) & (p <= hi), axis=1))
        if bad.size:
            r = int(bad[0])
            raise ValueError(f"WorldRobotSampler: the {name} of robot {r} is {p[r].tolist()} in its own frame, outside the normaliser's "
                             f"limits {lo.tolist()} .. {hi.tolist()}")
    return starts, goals, offsets, local_starts, local_goals


def _checked_slots(neighbor_slots, offsets, robot0, n_local, radius):
    """neighbor_slots for the host offsets [N, 2]: what the constructor was given, else (None) constraints.framed_slot_bound of them"""
    n = offsets.shape[0]
    if neighbor_slots is None:
        neighbor_slots = framed_slot_bound(offsets, robot0, n_local, LIMITS, radius) if n >= 2 else 1
    if n >= 2 and not 1 <= int(neighbor_slots) <= n - 1:
        raise ValueError(f"WorldRobotSampler: neighbor_slots must be in [1, {n - 1}], got {neighbor_slots}")
    return neighbor_slots


class WorldRobotSampler(MultiRobotSampler):
    """MultiRobotSampler for robots that each plan in the model's tile frame at their own offset in a global frame.  starts, goals [N, 2],
    the paths plan_round / plan take and return and PlanResult.paths_local are GLOBAL; offsets [N, 2] (every rank holds all of them);
    the hard conditions are start - offset and goal - offset, which must lie in the normaliser's position limits.  neighbor_slots: the
    slots per robot of the framed table (None: constraints.framed_slot_bound, computed once from the offsets).  constraint_table="dense"
    counts the pick's collisions over all pairs; "binned" reads them, and plan()'s report, off a collision cell table over the world's
    limits.  The guided step reads the framed all-pairs table either way.  env_id may name a world map (environments.register_world_map):
    robot r's map is then the window of the world's texture at offsets[r], which must lie on the world's cell grid and inside the world
    (environments.snap_to_world_map); robots at equal offsets share a resident slice.  own_windows=True (a world map only; a tile map ignores it)
    gives the sampler a window set of its own instead (map_textures.WorldWindowSet: slice r is local robot r's, storage and pointers
    stable), which `move` moves in place; release_windows() takes it out of the registry when the sampler is done with.  Starts and goals inside an obstacle are not refused.
    After every set_other_paths, `last_used` / `last_dropped` (int32 [n_local], on the device) tell the most slots a robot filled at one time step and the included points that found its block
    full.  `window` (an attribute, None = the default) is the culling window; a measurement may open it to compare with the all-pairs form.
    plan_rounds(repair=True), plan_rounds_subset(replan != "all") and replan_round are refused: the round table of repair has no frames, and
    the hooks here take the offsets in robot order, not in the order of a subset round's permuted instance."""

    def __init__(self, model, starts, goals, offsets, env_id="EnvEmpty2D", n_samples=64, rank=0, world_size=1,
                 norm_mins=synth.NORM_MINS, norm_maxs=synth.NORM_MAXS, n_guide_steps=20, start_guide_steps_fraction=0.5,
                 n_diffusion_steps_without_noise=1, weight_grad_cost_soft_constraints=2e-2, radius=VERTEX_CONSTRAINT_RADIUS,
                 device="cuda", group=None, n_streams=0, inter_robot=True, constraint_table="dense", own_windows=False, neighbor_slots=None):
        self._limits = (np.asarray(norm_mins, np.float32)[:2], np.asarray(norm_maxs, np.float32)[:2])
        self._fixed_slots = neighbor_slots               # what `move` keeps; None: the bound of every move's offsets
        starts, goals, offsets, local_starts, local_goals = _checked_ends(starts, goals, offsets, *self._limits)
        n = starts.shape[0]
        robot0, n_local = shard_range(n, rank, world_size)
        neighbor_slots = _checked_slots(neighbor_slots, offsets, robot0, n_local, radius)
        # a world map: every robot reads its own window of it; offsets off the cell grid or outside the world raise here, before any device work
        self._window_ids = self._windows = self._held_origins = None
        if environments.is_world_map(env_id):
            origins = environments.world_map_window_origins(env_id, offsets)
            if own_windows:
                # a window set of this sampler's own (slice r is local robot r's), which `move` moves in place
                self._windows = map_textures.WorldWindowSet(env_id, n_local, device)
            else:
                self._window_ids = [environments.world_window_name(env_id, org) for org in origins]
        try:
            super().__init__(model, local_starts, local_goals, env_id=env_id, n_samples=n_samples, rank=rank, world_size=world_size,
                             norm_mins=norm_mins, norm_maxs=norm_maxs, n_guide_steps=n_guide_steps,
                             start_guide_steps_fraction=start_guide_steps_fraction,
                             n_diffusion_steps_without_noise=n_diffusion_steps_without_noise,
                             weight_grad_cost_soft_constraints=weight_grad_cost_soft_constraints, radius=radius, device=device, group=group,
                             n_streams=n_streams, inter_robot=inter_robot, constraint_table=constraint_table)
            if self._windows is not None:
                self._move_windows(origins[self.robot0:self.robot0 + self.n_local])
        except BaseException:
            WorldRobotSampler.release_windows(self)      # (a set registered for a sampler that was never built)
            raise
        sl = slice(self.robot0, self.robot0 + self.n_local)
        self._ends = (starts[sl], goals[sl])             # plan(): the straight lines of the GLOBAL ends
        self.neighbor_slots = int(neighbor_slots)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.world_limits = world_limits(offsets)
        self.world_grid = world_grid(self.world_limits, radius)
        self.window = None              # the culling window in a robot's frame; None: constraints.framed_window(LIMITS, radius)
        self.last_used = self.last_dropped = None

    # ---- one sampler for many sets of ends: the state a constructor takes from (starts, goals, offsets), set again in place ----------------
    def move(self, starts, goals, offsets):
        """Give the sampler the state a freshly constructed one would have for these starts, goals and offsets [N, 2] (N as constructed),
        with the constructor's validation and messages: the hard conditions, the ends of plan()'s straight lines, `offsets`,
        `world_limits`, `world_grid` and `neighbor_slots` (recomputed unless the constructor was given one).  On a world map the
        sampler must own its windows (own_windows=True): they are moved in place on the device, and only the slices whose origin
        changed are cut again; a sampler on the shared named set raises ValueError.  On a tile map any sampler moves.  `move` then
        `plan*` is the fresh sampler's `plan*`, bit for bit.  Everything is validated before anything is changed."""
        if self._window_ids is not None:
            raise ValueError(f"WorldRobotSampler.move: the sampler reads the shared named windows of the world map {self.env_id!r}; "
                             "construct it with own_windows=True to move it")
        starts, goals, offsets, local_starts, local_goals = _checked_ends(starts, goals, offsets, *self._limits)
        if starts.shape[0] != self.n_robots:
            raise ValueError(f"WorldRobotSampler.move: {starts.shape[0]} robots given to a sampler of {self.n_robots}")
        neighbor_slots = _checked_slots(self._fixed_slots, offsets, self.robot0, self.n_local, self.radius)
        limits = world_limits(offsets)
        grid = world_grid(limits, self.radius)
        sl = slice(self.robot0, self.robot0 + self.n_local)
        origins = environments.world_map_window_origins(self.env_id, offsets)[sl] if self._windows is not None else None
        st, go = torch.from_numpy(local_starts[sl]), torch.from_numpy(local_goals[sl])
        z = torch.zeros_like(st)
        nz = self.dataset.normalizer
        self.hard_conds = {0: nz.normalize(torch.cat((st, z), -1)).to(self.device), H - 1: nz.normalize(torch.cat((go, z), -1)).to(self.device)}
        self._set_frames((starts[sl], goals[sl]), torch.from_numpy(offsets).to(self.device), neighbor_slots, limits, grid)
        if origins is not None:
            self._move_windows(origins)

    def _move_on_device(self, ends, offsets_host, origins_host, offsets_dev, hard_first_dev, hard_last_dev, origins_dev=None):
        """`move` for a caller that has the state on the device already (world_fleet.WorldFleet, from mmd_fleet_epoch_frames): the host
        ends (starts, goals) of plan()'s lines, the host offsets [N, 2] (for the slot bound and the world's limits) and origins [N, 2],
        and on the sampler's device the offsets float32 [N, 2], the normalised hard conditions float32 [n_local, 4] of rows 0 and 63
        and, on a world map, the origins int32 [n_local, 2].  One process (n_local == N).  The in-limits check is not made: the caller
        has proved it (a fleet's targets: world_fleet's CONTAINMENT).  Nothing is uploaded."""
        neighbor_slots = _checked_slots(self._fixed_slots, offsets_host, self.robot0, self.n_local, self.radius)
        limits = world_limits(offsets_host)
        grid = world_grid(limits, self.radius)
        self.hard_conds = {0: hard_first_dev, H - 1: hard_last_dev}
        self._set_frames(ends, offsets_dev, neighbor_slots, limits, grid)
        if self._windows is not None:
            self._move_windows(origins_host, origins_dev)

    def _set_frames(self, ends, offsets_dev, neighbor_slots, limits, grid):
        self._ends = ends
        self.neighbor_slots = int(neighbor_slots)
        self.offsets = offsets_dev
        self.world_limits, self.world_grid = limits, grid
        self._collision = None
        self.last_used = self.last_dropped = None

    def _move_windows(self, origins_host, origins_dev=None):
        """Move the sampler's own window set to the local robots' origins (int32 [n_local, 2] on the host; origins_dev: the same words on
        the device where the caller has them).  The slices that move are counted on the host, against the origins of the last move."""
        origins_host = np.ascontiguousarray(origins_host, dtype=np.int32)
        if origins_dev is None:
            origins_dev = torch.from_numpy(origins_host).to(self._windows.device)
        held = self._held_origins
        n_moved = self.n_local if held is None else int((origins_host != held).any(1).sum())
        self._windows.move(origins_dev, n_moved)
        self._held_origins = origins_host.copy()

    def release_windows(self):
        """Take the sampler's own window set (own_windows=True) out of map_textures' registry: update_world_map no longer reaches it.
        The sampler keeps its tensors and still plans.  Nothing on a sampler without a set of its own."""
        if self._windows is not None:
            self._windows.release()

    def _robot_window_set(self):
        return self._windows

    # ---- the three places where the frame enters a round: MultiRobotSampler's hooks -------------------------------------------------------
    def _robot_env_ids(self, robot0, n):
        """On a world map (environments.register_world_map) robot r's map is its window of the world, environments.world_window_name(env_id,
        offsets[r]); on a tile map every robot's window shows that tile (None)"""
        return None if self._window_ids is None else self._window_ids[robot0:robot0 + n]

    def _build_collision_table(self, paths, robot0, n):
        """The collision cell table of the global paths over the world's limits (a robot outside them lands in a border cell: the cell
        index is clamped, which keeps neighbours in neighbouring cells)."""
        return binned_collision_table(paths, robot0, n, self.radius, limits=self.world_limits, grid=self.world_grid)

    def _report_on_own_table(self):
        return self.constraint_table == "binned" and self.n_robots >= 2

    def set_other_paths(self, paths_all):
        """MultiRobotSampler.set_other_paths on GLOBAL best paths: the framed table of the local robots for the guided step, and with
        constraint_table="binned" the world collision table for best_paths.  `last_used` / `last_dropped` are None where no table is built."""
        self.last_used = self.last_dropped = None
        super().set_other_paths(paths_all)

    def _set_inter_robot_table(self, guide, paths, robot0, n):
        """The framed all-pairs table, whatever constraint_table says (that chooses the pick's and the report's table only)"""
        guide.reset_extra_costs()
        cons = framed_constraints_from_paths(paths, self.offsets, robot0, n, self.neighbor_slots, self.radius, self.w_soft, self.window)
        guide.set_packed_constraints(cons[:5])
        self.last_used, self.last_dropped = cons[5], cons[6]

    def _in_shared_frame(self, t, robot0, n_robots):
        """The samples shifted to the global frame, for everything between robots: a copy, positions + offset, one fp32 add"""
        tg = t.view(n_robots, self.n_samples, H, D).clone()
        tg[..., :2] += self.offsets[robot0:robot0 + n_robots, None, None, :]
        return tg.view(-1, H, D)

    # ---- the loop: MultiRobotSampler's, through the methods above -------------------------------------------------------------------
    def plan_rounds(self, paths_local=None, max_rounds=8, seed=0, list_cap=0, repair=False, hard_slots=32,
                    weight_grad_cost_constraints=2e-1, t_pad=2, local_rounds=False, n_noising_steps=3, n_denoising_steps=3):
        return WorldRobotSampler.plan_rounds_subset(self, paths_local, max_rounds, seed, list_cap, repair, hard_slots,
                                                    weight_grad_cost_constraints, t_pad, local_rounds, n_noising_steps, n_denoising_steps)

    def plan_rounds_subset(self, paths_local=None, max_rounds=8, seed=0, list_cap=0, repair=False, hard_slots=32,
                           weight_grad_cost_constraints=2e-1, t_pad=2, local_rounds=False, n_noising_steps=3, n_denoising_steps=3,
                           replan="all", independent_iters=8):
        """MultiRobotSampler.plan_rounds_subset on global paths.  PlanResult.dropped_constraints is `last_dropped` of the last round run
        (a device tensor, or None when no table was built).  plan_rounds_seeded's init_trajs are normalised trajectories in the robots'
        own frames (trajs_from_global makes them from global seeds)."""
        if repair:
            raise ValueError("WorldRobotSampler: repair=True is not supported: the round table is built without per-robot frames")
        if replan != "all":
            raise ValueError(f"WorldRobotSampler: replan={replan!r} is not supported: the per-robot frames do not follow the permutation of a subset round")
        res = MultiRobotSampler.plan_rounds_subset(self, paths_local, max_rounds, seed, list_cap, repair, hard_slots,
                                                   weight_grad_cost_constraints, t_pad, local_rounds, n_noising_steps, n_denoising_steps,
                                                   replan, independent_iters)
        res.dropped_constraints = self.last_dropped
        return res

    def trajs_from_global(self, seeds):
        """init_trajs of plan_rounds_seeded from seed trajectories in the global frame: seeds float32 [n_local, 64, 4] (positions and velocities,
        trajs_final's format; world_fleet.device_window_seeds') of this rank's robots -> normalised [n_local * n_samples, H, D] on the
        sampler's device.  Per robot: its offset subtracted from x and y (one fp32 subtraction each), dataset.normalize_trajectories,
        a clip to [-1, 1] (a seed's velocity may exceed the normaliser's limits; positions inside the window are not moved), and the
        row repeated n_samples times, robot-major.  Torch operations on the device; no host copy."""
        seeds = torch.as_tensor(seeds)
        if tuple(seeds.shape) != (self.n_local, H, D) or seeds.dtype != torch.float32:
            raise ValueError(f"WorldRobotSampler.trajs_from_global: seeds must be float32 [{self.n_local}, {H}, {D}], got {seeds.dtype} "
                             f"{tuple(seeds.shape)}")
        local = seeds.to(self.device).clone()
        local[..., :2] -= self.offsets[self.robot0:self.robot0 + self.n_local, None, :]
        normed = torch.clip(self.dataset.normalize_trajectories(local), -1.0, 1.0)
        return normed[:, None].expand(self.n_local, self.n_samples, H, D).reshape(-1, H, D).contiguous()

    def replan_round(self, *args, **kwargs):
        raise ValueError("WorldRobotSampler: replan_round is not supported: the per-robot frames do not follow the permutation of a subset round")


def random_world_instance(n_robots, extent, seed, env_id="EnvEmpty2D", min_separation=0.15, max_draws=200000):
    """A random many-robot instance in a square world of side `extent`, centred on the origin -> (starts, goals, offsets), float32
    [n_robots, 2] each, starts and goals global.  Per robot, from numpy.random.Generator(PCG64(seed)) as
    trials.get_start_goal_pos_random_in_env draws: a window origin such that the window offset + [-1, 1]^2 lies inside the world
    (continuous on a map without obstacles, snapped to the tile pitch 2.0 on a map with them, so that the tiles do not overlap), then a
    start and a goal uniform in +-0.95 of the window; the draw is accepted iff both are more than OBSTACLE_MARGIN away from the map's
    obstacles (environments.map_sdf) and the start (the goal) is more than min_separation away from every earlier robot's start (goal),
    measured globally.  Raises RuntimeError after max_draws draws."""
    env_id = getattr(env_id, "__name__", env_id)
    if not extent >= TILE_PITCH:
        raise ValueError(f"random_world_instance: a world of side {extent} cannot hold a window of side {TILE_PITCH}")
    rng = np.random.Generator(np.random.PCG64(seed))
    snapped = map_has_obstacles(env_id)
    tiles = int(np.floor(extent / TILE_PITCH))
    half = np.float32((extent - TILE_PITCH) / 2.0)
    starts, goals, offsets = (np.zeros((0, 2), np.float32) for _ in range(3))
    draws = 0
    while len(starts) < n_robots:
        if draws >= max_draws:
            raise RuntimeError(f"random_world_instance: {n_robots} robots not placed in a world of side {extent} on {env_id} after "
                               f"{max_draws} draws (min_separation={min_separation}); {len(starts)} placed")
        draws += 1
        if snapped:
            off = (rng.integers(0, tiles, (1, 2)).astype(np.float32) * np.float32(TILE_PITCH) - np.float32((tiles - 1) * TILE_PITCH / 2.0))
        else:
            off = (rng.random((1, 2), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)) * half
        off = off.astype(np.float32)
        ends = (rng.random((2, 2), dtype=np.float32) * np.float32(1.9) - np.float32(0.95)).astype(np.float32)      # local start, goal
        if snapped and not bool((map_sdf(ends, env_id) > OBSTACLE_MARGIN).all()):
            continue
        st, go = ends[:1] + off, ends[1:] + off
        if len(starts) and not (np.all(np.sqrt(np.sum((st - starts) ** 2, axis=1)) > min_separation)
                                and np.all(np.sqrt(np.sum((go - goals) ** 2, axis=1)) > min_separation)):
            continue
        starts, goals, offsets = np.concatenate([starts, st]), np.concatenate([goals, go]), np.concatenate([offsets, off])
    return starts, goals, offsets


def random_world_map_instance(name, n_robots, seed, min_separation=0.15, max_draws=200000):
    """A random many-robot instance on the world map `name` (environments.register_world_map) -> (starts, goals, offsets), float32
    [n_robots, 2] each, starts and goals global.  Drawn as random_world_instance draws, from numpy.random.Generator(PCG64(seed)): per
    robot a window origin uniform over the valid origin cells of the world (so the offset lies on the cell grid and the window inside the
    world), then a start and a goal uniform in +-0.95 of the window; the draw is accepted iff the world texture's nearest-cell value
    (environments.world_map_sdf on the host texture) at both global points exceeds OBSTACLE_MARGIN and the start (the goal) is more than
    min_separation away from every earlier robot's start (goal).  Raises RuntimeError after max_draws draws."""
    shape = environments.world_map_occupancy(name).shape
    nx, ny = environments.grid_shape()
    rng = np.random.Generator(np.random.PCG64(seed))
    starts, goals, offsets = (np.zeros((0, 2), np.float32) for _ in range(3))
    draws = 0
    while len(starts) < n_robots:
        if draws >= max_draws:
            raise RuntimeError(f"random_world_map_instance: {n_robots} robots not placed on the world map {name!r} after {max_draws} draws "
                               f"(min_separation={min_separation}); {len(starts)} placed")
        draws += 1
        cells = np.stack([rng.integers(0, shape[0] - nx + 1, (1,)), rng.integers(0, shape[1] - ny + 1, (1,))], axis=1)
        off = environments.snap_to_world_map(name, (cells * environments.SDF_CELL_SIZE + np.asarray(environments.world_map_origin(name))
                                                    - np.asarray(LIMITS[0])))
        ends = (rng.random((2, 2), dtype=np.float32) * np.float32(1.9) - np.float32(0.95)).astype(np.float32)      # local start, goal
        st, go = ends[:1] + off, ends[1:] + off
        if not bool((environments.world_map_sdf(np.concatenate([st, go]), name) > OBSTACLE_MARGIN).all()):
            continue
        if len(starts) and not (np.all(np.sqrt(np.sum((st - starts) ** 2, axis=1)) > min_separation)
                                and np.all(np.sqrt(np.sum((go - goals) ** 2, axis=1)) > min_separation)):
            continue
        starts, goals, offsets = np.concatenate([starts, st]), np.concatenate([goals, go]), np.concatenate([offsets, off])
    return starts, goals, offsets
