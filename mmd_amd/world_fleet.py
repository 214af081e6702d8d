"""World fleets: N robots, each from anywhere to anywhere on a world map, planned together as a receding-horizon loop.

WorldRobotSampler plans many robots at once but wants every robot's start and goal in one window; world_routes takes one robot across
the world alone.  Here the two meet.  Every robot has the exact distance field of its goal over the whole world grid (built once, one
field per distinct goal cell).  An epoch reads every robot's next sub-goal and window off those fields in one launch
(mmd_grid_window_goals, device_window_goals), plans all robots together from their positions to their sub-goals with a
WorldRobotSampler on the windows, and moves the robots to the ends of the returned paths; the loop ends when every robot stands on
its goal.

The numpy function window_goal IS the definition of the sub-goal and the window; the kernel (csrc/window_goals.hip) computes the same
integers, and the tests hold it to equality.

  c0 = start, d0 = dist[c0], h = window // 2
  walk    from c = c0 with d = dist[c], while d > 0 and steps < max_steps: the candidates are the neighbours of c inside the grid that
          hold exactly d - 1, the x-candidate the first of +x, -x, the y-candidate the first of +y, -y; the next cell n is the
          x-candidate if |g.x - c.x| >= |g.y - c.y| (g the field's goal cell), else the y-candidate, and the other axis's candidate where
          that axis has none; the walk ends before a step with max(|n.x - c0.x|, |n.y - c0.y|) > reach.
  cell    the last cell reached;  steps the steps taken;  remaining = d0 - steps (every candidate lies on a shortest path)
  origin  clip(c0 - h, 0, n - window) per axis: the window of `window` cells per side that the robot plans in

The step rule prefers the axis along which the goal is farther, so that open ground gives a diagonal staircase towards the goal and not
the L of a fixed neighbour order: sub-goals of robots that cross then spread over the box instead of lining up on its border rows.

Two facts, for 1 <= reach <= h - 1, window <= min(nx, ny) and max_steps >= 1 (tests/test_world_fleet_host.py checks both by brute force):

CONTAINMENT.  Every cell c inside the grid with max(|c.x - c0.x|, |c.y - c0.y|) <= reach lies in [origin, origin + window) per axis,
with c - origin >= h - reach and origin + window - c >= h - reach on every side on which the window was not clamped to the world's edge.
Per axis, with o = c0 - h before the clip: c - o >= h - reach >= 1 and o + window - c >= window - h - reach >= h - reach >= 1
(window - h >= h).  A clip at the low edge raises the origin to 0 <= c and only widens the high side; a clip at the high edge lowers
origin + window to n > c and only widens the low side.  So the start, the sub-goal and every cell of the walk lie in the window, at
least (h - reach) cells from each side that faces more world.

PROGRESS.  On a converged field (status OK) with d0 > 0, steps >= min(d0, max_steps, reach): a step moves one cell along one axis, so
after k steps the walk is within Chebyshev distance k of c0, and a step can leave the box only if k + 1 > reach.  The walk therefore
ends by d == 0 (steps = d0), by steps == max_steps, or with steps >= reach.  The next call starts from `cell`, where the same field
holds `remaining`, so calls repeated from the cell reached arrive after at most ceil(d0 / min(max_steps, reach)) calls (epoch_bound).
"""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, environments, map_textures
from .world import OBSTACLE_MARGIN, WorldRobotSampler
from .world_routes import (ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, UNREACHED, _int32_dev, _points, cell_centres,
                           device_distance_field, world_cells)

_STATUS_NAMES = {ROUTE_OK: "ok", ROUTE_UNREACHED: "unreached", ROUTE_STUCK: "stuck", ROUTE_OUTSIDE: "outside"}


# ---- the definition, on the host ---------------------------------------------------------------------------------------------------------
def _checked_walk_args(what, shape, reach, max_steps, window):
    reach, max_steps, window = int(reach), int(max_steps), int(window)
    if not (1 <= window <= min(shape) and 1 <= reach <= window // 2 - 1 and max_steps >= 1):
        raise ValueError(f"{what}: reach = {reach} (1 to window // 2 - 1), max_steps = {max_steps} (at least 1), window = {window} "
                         f"(at most min(nx, ny) = {min(shape)})")
    return reach, max_steps, window


def window_goal(dist, start, goal, reach, max_steps, window=400):
    """(cell (ix, iy), origin (i0, j0), steps, remaining, status): the next sub-goal and the window of a robot at the cell `start`, from
    the converged field dist [nx, ny] of the goal cell `goal` (the module's docstring).  status: ROUTE_OK; ROUTE_OUTSIDE (the start is not
    a cell of the grid) and ROUTE_UNREACHED (dist[start] is UNREACHED): steps = remaining = -1, cell and origin (0, 0); ROUTE_STUCK (no
    neighbour holds d - 1: the field was not converged; the outputs are what the walk covered)."""
    dist = np.asarray(dist)
    nx, ny = dist.shape
    reach, max_steps, window = _checked_walk_args("window_goal", (nx, ny), reach, max_steps, window)
    x0, y0 = int(start[0]), int(start[1])
    gx, gy = int(goal[0]), int(goal[1])
    if not (0 <= x0 < nx and 0 <= y0 < ny):
        return (0, 0), (0, 0), -1, -1, ROUTE_OUTSIDE
    d0 = int(dist[x0, y0])
    if d0 == UNREACHED:
        return (0, 0), (0, 0), -1, -1, ROUTE_UNREACHED
    origin = (min(max(x0 - window // 2, 0), nx - window), min(max(y0 - window // 2, 0), ny - window))
    ix, iy, d, steps, status = x0, y0, d0, 0, ROUTE_OK
    while d > 0 and steps < max_steps:
        holds = lambda jx, jy: 0 <= jx < nx and 0 <= jy < ny and int(dist[jx, jy]) == d - 1                          # noqa: E731
        along_x = [(ix + s, iy) for s in (1, -1) if holds(ix + s, iy)]
        along_y = [(ix, iy + s) for s in (1, -1) if holds(ix, iy + s)]
        if not along_x and not along_y:
            status = ROUTE_STUCK
            break
        first, second = (along_x, along_y) if abs(gx - ix) >= abs(gy - iy) else (along_y, along_x)
        jx, jy = (first or second)[0]
        if max(abs(jx - x0), abs(jy - y0)) > reach:
            break
        ix, iy, d, steps = jx, jy, d - 1, steps + 1
    return (ix, iy), origin, steps, d0 - steps, status


def window_goals(dist, starts, fields, goals, reach, max_steps, window=400):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4] = (steps, remaining, status, arrived)): window_goal for query q from
    starts[q] in field dist[fields[q]] of the goal cell goals[fields[q]]; dist [n_fields, nx, ny], goals [n_fields, 2].  A field index
    outside [0, n_fields) gives ROUTE_OUTSIDE.  arrived = 1 iff the status is ROUTE_OK and remaining == 0."""
    dist = np.asarray(dist)
    starts, goals = np.asarray(starts, np.int64).reshape(-1, 2), np.asarray(goals, np.int64).reshape(-1, 2)
    fields = np.asarray(fields, np.int64).reshape(-1)
    _checked_walk_args("window_goals", dist.shape[1:], reach, max_steps, window)
    n = len(starts)
    cells, origins, summary = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32), np.zeros((n, 4), np.int32)
    for q in range(n):
        f = int(fields[q])
        if 0 <= f < dist.shape[0]:
            cells[q], origins[q], steps, remaining, status = window_goal(dist[f], starts[q], goals[f], reach, max_steps, window)
        else:
            steps, remaining, status = -1, -1, ROUTE_OUTSIDE
        summary[q] = (steps, remaining, status, int(status == ROUTE_OK and remaining == 0))
    return cells, origins, summary


def epoch_bound(d0, reach, max_steps):
    """The calls of window_goal, each from the cell the one before reached, that bring a robot d0 steps from its goal onto it, at most:
    ceil(d0 / min(max_steps, reach)) (PROGRESS, above)"""
    return -(-int(d0) // min(int(max_steps), int(reach)))


# ---- the same on the device ----------------------------------------------------------------------------------------------------------------
def _window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window):
    """device_window_goals' launch -> one int32 tensor [8 n] on the device: cells [n, 2], then origins [n, 2], then summary [n, 4]"""
    if dist_dev.dim() != 3 or dist_dev.dtype != torch.int32 or not dist_dev.is_cuda or not dist_dev.is_contiguous():
        raise ValueError("device_window_goals: dist must be a contiguous int32 CUDA(HIP) tensor [n_fields, nx, ny]")
    reach, max_steps, window = _checked_walk_args("device_window_goals", tuple(dist_dev.shape[1:]), reach, max_steps, window)
    starts_dev = _int32_dev(starts, (-1, 2), dist_dev.device, "device_window_goals: starts")
    n = starts_dev.shape[0]
    fields_dev = _int32_dev(fields, (n,), dist_dev.device, "device_window_goals: fields")
    goals_dev = _int32_dev(goals, (int(dist_dev.shape[0]), 2), dist_dev.device, "device_window_goals: goals")
    words = torch.empty(8 * n, dtype=torch.int32, device=dist_dev.device)        # (the summary rows start 16 n bytes in: aligned as int4)
    at = lambda k: C.c_void_p(words.data_ptr() + 4 * k)                          # noqa: E731
    _lib.launch("mmd_grid_window_goals", dist_dev, C.c_void_p(dist_dev.data_ptr()), int(dist_dev.shape[1]), int(dist_dev.shape[2]),
                int(dist_dev.shape[0]), C.c_void_p(starts_dev.data_ptr()), C.c_void_p(fields_dev.data_ptr()), C.c_void_p(goals_dev.data_ptr()),
                n, reach, max_steps, window, at(0), at(2 * n), at(4 * n))
    return words


def _split_words(words):
    n = words.shape[0] // 8
    return words[:2 * n].reshape(n, 2), words[2 * n:4 * n].reshape(n, 2), words[4 * n:].reshape(n, 4)


def device_window_goals(dist_dev, starts, fields, goals, reach, max_steps, window=400):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4]) on dist_dev's device: window_goals() for every query in one launch
    (mmd_grid_window_goals), word for word.  dist_dev: any int32 fields [n_fields, nx, ny] (device_distance_field's, or hand-built
    ones); goals [n_fields, 2]: the fields' goal cells.  The three results are views of one tensor."""
    return _split_words(_window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window))


# ---- the fleet -----------------------------------------------------------------------------------------------------------------------------
class EpochTargets(NamedTuple):
    """What one epoch plans towards (WorldFleet.epoch_targets), numpy on the host."""
    cells: np.ndarray           # int32 [N, 2]: the sub-goal cells in the world
    origins: np.ndarray         # int32 [N, 2]: the windows' origin cells
    offsets: np.ndarray         # float32 [N, 2]: the windows' offsets (environments.world_map_window_offsets)
    points: np.ndarray          # float32 [N, 2]: the sub-goal points, global: the cell's centre, or the robot's exact goal once `arrived`
    summary: np.ndarray         # int32 [N, 4]: (steps, remaining, status, arrived)


class FleetResult(NamedTuple):
    """What WorldFleet.run returns."""
    paths: torch.Tensor         # float32 [N, E * 64, 2] on the device, global: epoch e's paths are columns [64 e, 64 e + 64)
    arrived: np.ndarray         # bool [N]: the robot stands on its exact goal point
    epochs: list                # per epoch {"conflict_counts", "summary", "offsets"}: the PlanResult's counts, the epoch's targets


class WorldFleet:
    """N robots from global starts to global goals [N, 2] anywhere on the world map `name` (environments.register_world_map), planned
    together epoch by epoch; one process (rank 0 of 1).  The constructor builds, once, the distance field of every distinct goal cell
    over the whole world grid on the resident world texture (device_distance_field, region None): 4 * nx * ny bytes per distinct goal,
    16.8 MB on a 2048-side world.  ValueError names the robot whose start or goal lies outside the world or on a cell that is not
    routable at `clearance`, or whose goal cannot be reached from its start.

    reach, max_steps: window_goal's, in cells; reach <= 199 on the model's 400-cell window.  Further keyword arguments go to every
    epoch's WorldRobotSampler (n_samples, constraint_table, ...).  `positions` (float32 [N, 2], global) are the robots' current points.

    Out of scope here: an arrived robot is sampled like any other, between two ends pinned to its goal point, not held still; an epoch
    starts from noise, not from the cell path; every epoch builds a sampler of its own, the windows of one long-lived sampler are not
    moved in place; the fleet is not sharded over ranks; repair= and replan=, which WorldRobotSampler refuses."""

    def __init__(self, model, name, starts, goals, clearance=OBSTACLE_MARGIN, reach=180, max_steps=360, device="cuda",
                 **world_robot_sampler_kwargs):
        self.model, self.name, self.device = model, name, environments.resolved_device(device)
        self.clearance = float(clearance)
        self.sampler_kwargs = dict(world_robot_sampler_kwargs)
        for refused in ("rank", "world_size", "group", "env_id"):
            if refused in self.sampler_kwargs:
                raise ValueError(f"WorldFleet: {refused}= is not taken: a fleet runs in one process on the world map it was given")
        self.shape = tuple(environments.world_map_occupancy(name).shape)
        self.window = int(environments.grid_shape()[0])
        self.reach, self.max_steps, _ = _checked_walk_args("WorldFleet", self.shape, reach, max_steps, self.window)
        self.limits = environments.world_map_limits(name)
        s_pts, self.goal_points = _points(starts), _points(goals)
        n = s_pts.shape[0]
        if n == 0 or self.goal_points.shape[0] != n:
            raise ValueError(f"WorldFleet: {n} starts and {self.goal_points.shape[0]} goals (equal and at least 1)")
        s_cells, g_cells = (self._cells(pts, what) for pts, what in ((s_pts, "start"), (self.goal_points, "goal")))
        self.field_goals, which = np.unique(g_cells, axis=0, return_inverse=True)
        self.fields = which.reshape(-1).astype(np.int32)
        tex = map_textures.device_world_texture(name, self.device)
        self.dist, _ = device_distance_field(tex, self.field_goals, self.clearance)
        # one gather and one copy: is every end routable, and how far is every start from its goal
        both = torch.from_numpy(np.concatenate([s_cells, g_cells]).astype(np.int64)).to(self.device)
        free = tex[both[:, 0], both[:, 1], 0] > np.float32(self.clearance)
        f_dev = torch.from_numpy(self.fields.astype(np.int64)).to(self.device)
        d0 = self.dist[f_dev, both[:n, 0], both[:n, 1]]
        free, d0 = free.cpu().numpy(), d0.cpu().numpy()
        for r in range(n):
            for what, ok, cell in (("start", free[r], s_cells[r]), ("goal", free[n + r], g_cells[r])):
                if not ok:
                    raise ValueError(f"WorldFleet: the {what} of robot {r} on {name!r}, cell {cell.tolist()}, is not routable at clearance "
                                     f"{self.clearance}")
            if d0[r] == UNREACHED:
                raise ValueError(f"WorldFleet: robot {r} on {name!r}: the goal cell {g_cells[r].tolist()} cannot be reached from the start "
                                 f"cell {s_cells[r].tolist()} at clearance {self.clearance}")
        self._fields_dev = f_dev.to(torch.int32)             # an epoch's launch uploads the robots' cells only
        self._goals_dev = torch.from_numpy(self.field_goals.astype(np.int32)).to(self.device)
        self.n_robots = n
        self.start_distances = d0.astype(np.int64)
        self.positions = s_pts.copy()

    def _cells(self, points, what):
        """world_cells of the robots' points, with its refusal (a point that is not finite or lies outside the world) naming the robot"""
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(~((points >= np.asarray(self.limits[0], np.float32)) & (points <= np.asarray(self.limits[1], np.float32))).all(1))
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"WorldFleet: the {what} of robot {k}, {points[k].tolist()}, lies outside the world map {self.name!r}, "
                             f"{self.limits[0]} .. {self.limits[1]}")
        return world_cells(self.name, points)

    def epoch_bound(self):
        """The epochs that bring every robot from its START onto its goal, at most (epoch_bound over the fields; at least 1: the epoch
        that moves a robot from its start point to its goal point inside one cell)"""
        return max(1, max(epoch_bound(d, self.reach, self.max_steps) for d in self.start_distances.tolist()))

    def epoch_targets(self, positions):
        """EpochTargets of the robots at the global points `positions` [N, 2]: one mmd_grid_window_goals launch and one device -> host
        copy.  A robot's cell is world_cells' texel of its point; its sub-goal point is the centre of the sub-goal cell by cell_centres'
        fp32 sequence, or, once the sub-goal cell is the goal's (`arrived`), the caller's exact goal point."""
        pts = _points(positions)
        if pts.shape[0] != self.n_robots:
            raise ValueError(f"WorldFleet.epoch_targets: {pts.shape[0]} positions for {self.n_robots} robots")
        c0 = self._cells(pts, "position")
        words = _window_goals_words(self.dist, c0, self._fields_dev, self._goals_dev, self.reach, self.max_steps, self.window)
        cells, origins, summary = (a.copy() for a in _split_words(words.cpu().numpy()))
        bad = np.flatnonzero(summary[:, 2] != ROUTE_OK)
        if bad.size:
            r = int(bad[0])
            raise RuntimeError(f"WorldFleet: robot {r} on {self.name!r} at cell {c0[r].tolist()}: sub-goal status "
                               f"{_STATUS_NAMES.get(int(summary[r, 2]), int(summary[r, 2]))}")
        points = np.ascontiguousarray(cell_centres(cells, self.limits[0], self.limits[1], self.shape), dtype=np.float32)
        arrived = summary[:, 3] == 1
        points[arrived] = self.goal_points[arrived]
        return EpochTargets(cells, origins, environments.world_map_window_offsets(self.name, origins), points, summary)

    def step(self, seed, max_rounds=8):
        """One epoch: the targets of the current positions, a WorldRobotSampler from the positions to the sub-goal points on the windows,
        its plan(max_rounds, seed), and the robots moved to the last points of the returned paths, as they are.  The epoch's window map
        set is released afterwards (map_textures.release_sdf_textures).  -> (PlanResult, EpochTargets)"""
        targets = self.epoch_targets(self.positions)
        sampler = WorldRobotSampler(self.model, self.positions, targets.points, targets.offsets, env_id=self.name, device=self.device,
                                    **self.sampler_kwargs)
        try:
            res = sampler.plan(max_rounds=max_rounds, seed=seed)
        finally:
            map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), self.device)
        self.positions = np.ascontiguousarray(res.paths_local[:, -1, :].cpu().numpy(), dtype=np.float32)
        return res, targets

    def run(self, max_epochs=None, max_rounds=8, seed=0):
        """Epochs (epoch e with seed + e) until every robot has arrived, at most max_epochs of them (None: epoch_bound(), which suffices
        from the starts).  A robot that has arrived keeps taking part, from its goal point to its goal point, so that the others stay
        constrained by it.  -> FleetResult"""
        if max_epochs is None:
            max_epochs = self.epoch_bound()
        paths, epochs = [], []
        arrived = np.zeros(self.n_robots, bool)
        for e in range(int(max_epochs)):
            res, targets = self.step(seed + e, max_rounds)
            paths.append(res.paths_local)
            epochs.append({"conflict_counts": list(res.conflict_counts), "summary": targets.summary, "offsets": targets.offsets})
            arrived = targets.summary[:, 3] == 1             # the epoch's sub-goal was the goal point: the robot now stands on it
            if arrived.all():
                break
        if not paths:
            raise ValueError(f"WorldFleet.run: max_epochs = {max_epochs} (at least 1)")
        return FleetResult(torch.cat(paths, dim=1), arrived, epochs)
