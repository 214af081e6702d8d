"""World fleets: N robots, each from anywhere to anywhere on a world map, planned together as a receding-horizon loop.

WorldRobotSampler plans many robots at once but wants every robot's start and goal in one window; world_routes takes one robot across
the world alone.  Here the two meet.  Every robot has the exact distance field of its goal over the whole world grid (built once, one
field per distinct goal cell).  An epoch reads every robot's next sub-goal and window off those fields in one launch
(mmd_grid_window_goals, device_window_goals), plans all robots together from their positions to their sub-goals with a
WorldRobotSampler on the windows, and moves the robots to the ends of the returned paths; the loop ends when every robot stands on
its goal.

The numpy function window_goal IS the definition of the sub-goal and the window; the kernel (csrc/window_goals.hip) computes the same
integers, and the tests hold it to equality.  Every definition below stands on one function, _walks, which walks every query once and
keeps its cell path; _path_samples gives the support cells of paths cut at k, _blockers a robot's blockers.

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

An epoch may start from its walk instead of from noise (WorldFleet(seed_epochs=True)).  window_goal_samples keeps 64 support cells of the
walk's cell path and window_seed turns them into a smoothed chain of points with velocities inside the robot's window; these two numpy
functions are definitions as well, and mmd_grid_window_goal_samples (csrc/window_goals.hip: one body with mmd_grid_window_goals' kernel)
and mmd_window_seeds (csrc/window_seeds.hip) compute the same integers and the same float32 bits.

SEPARATION (WorldFleet(separation=), opt-in).  An epoch pins both ends of every path, and each walk ignores every other robot: two plain
sub-goals may be one cell, or closer than the robot-robot margin, and then the epoch has a conflict pinned at t = 63 that no sampling
resolves, and the next epoch has it pinned at t = 0.  subgoals_apart IS the definition of the sub-goals kept `sep` cells apart; the
kernels (csrc/window_apart.hip) compute the same integers.

  taking part  query q iff window_goal's status for it is ROUTE_OK; its walk is _walks' cell path c_q[0 .. walked_q], c_q[0] the start
  conflict     two cells with dx^2 + dy^2 < sep^2, in integers
  blockers     of robot r, the robots taken in index order (a lower index has priority): the CHOSEN cells of the taking-part robots
               j < r and the START cells of the taking-part robots j > r
  k_r          the largest k in [1, walked_r] whose cell c_r[k] conflicts with no blocker, 0 if there is none: the largest feasible index,
               not the longest feasible prefix (a walk may pass a blocker; the sampler's soft constraints handle the way round it)
  outputs      cell c_r[k_r]; origin window_goal's; summary (k_r, d0 - k_r, status, d0 == k_r), window_goals' format;
               extra (walked_r, clear_r), clear_r = 1 iff the chosen cell conflicts with no blocker

APART.  If the start cells of the taking-part robots are pairwise at least sep apart, so are the chosen cells, and every clear is 1.
k = 0 is always feasible for robot r: the robots with priority chose against r's start, and the robots below r are counted at their
starts, which are apart from r's by assumption; so the chosen cell of r, c_r[k_r] with k_r >= 1 by the rule or c_r[0] by this, conflicts
with no blocker.  A chosen cell avoids every earlier choice by construction, and every later choice avoids it, because it is an
earlier choice for them.  The ends of one epoch are the starts of the next, so the invariant carries through a run
(tests/test_world_fleet_apart_host.py checks it by brute force over whole runs).  With starts already in conflict the rule still
answers; clear = 0 marks a robot left on a start that conflicts (only with k = 0).

PROGRESS does NOT hold under separation, and epoch_bound with it: a robot may be held back to k = 0 for as long as others stand in its
way.  What holds is termination.  remaining never rises, so in every epoch either some robot's remaining falls (some k > 0), which can
happen only finitely often, or every k is 0; then every robot stays on its cell, the next epoch's inputs are this epoch's, and the
state repeats for good: if a robot is still off its goal the epoch is STALLED, and WorldFleet.run stops there.  A robot that walks onto
its goal in this epoch has k > 0: it moves, its start cell may be what held another robot back, and the epoch is not stalled.

The same choice as a fixed point, for the device (subgoals_apart_sweeps).  Start from k_r = walked_r; in one sweep every robot applies
the rule to the k that the robots j < r held after the sweep before, all at once (Jacobi, two buffers).  k_r depends only on the robots
j < r: after sweep s the robots 0 .. s - 1 hold the definition's k (robot 0 depends on starts alone; induction), so the fixed point is
unique, it is subgoals_apart's result, n sweeps always reach it, and a sweep in which no k moved (changed == 0) proves it is reached,
because a sweep is a function of the state before it.

STEPPING ASIDE (WorldFleet(step_aside=True), opt-in, on top of the separation).  A walk is a fixed descent of its goal's field and cannot
go round another robot, so a robot that stands still -- it has arrived, or it is itself held -- is a wall for every walk that passes
within sep cells of it, and the run ends stalled.  subgoals_aside IS the definition of an epoch in which such a robot steps aside and
the robot it held walks at once; the kernels (csrc/window_aside.hip) compute the same integers.

  phase 1    subgoals_apart, unchanged: k_r, walked_r, the walks c_r[0 .. walked_r], cell_r = c_r[k_r] of every query that takes part
  roles      stands_j: j takes part and k_j == 0.  held_r: stands_r and walked_r >= 1.  clears(j): the r with held_r, r != j, stands_j,
             c_j[0] in conflict with c_r[1], and (not held_j or r < j); j YIELDS iff clears(j) is not empty.  A standing robot that is not
             held (it has arrived, or walked = 0) yields to anyone, a held robot only to held robots of lower index.
  phase 2    the yielders in ascending index.  l_j(c) is the 4-connected BFS distance from c_j[0] over the cells of the grid within
             Chebyshev distance aside_reach of it that j's OWN field reaches (it is finite exactly on the routable cells connected to the
             goal, the start among them: no texture is needed).  The candidates are the cells with 1 <= l_j(c) <= aside_steps that
             conflict with (a) no cell_i of a taking-part i != j that does not yield, (b) no final cell of a yielder i < j, (c) no start
             of a yielder i > j, (d) no cell c_r[0 .. walked_r] of any r in clears(j); the choice is the least
             (l_j(c), own field at c, ix, iy), and with no candidate the robot stays.
  phase 3    released: the r with held_r that did not move aside and lie in clears(j) of some j that did.  In ascending index r applies
             subgoals_apart's rule to its walk once more, against the final cells of all other taking-part robots as they stand then
             (a released robot of higher index still on its start).  Without this phase the yielder walks back in the next epoch before
             the held robot has moved.
  outputs    moved aside: cell = the side cell, summary (l, own field there, status, own field there == 0); released: cell c_r[k'],
             summary (k', d0 - k', status, d0 == k'); everyone else phase 1's words; origins and extra are phase 1's;
             aside = (role bits, l): ASIDE_HELD 1, ASIDE_YIELDS 2, ASIDE_MOVED 4, ASIDE_RELEASED 8, l = 0 unless MOVED

SAFETY.  If the start cells of the taking-part robots are pairwise sep apart, so are the final cells.  The invariant is that the robots'
CURRENT cells are pairwise apart.  It holds after phase 1 (APART).  Phase 2 moves yielder j to a cell that conflicts with no current cell
of another robot, for (a), (b) and (c) together are exactly those: a robot that does not yield is on cell_i, a yielder below j on its final
cell, a yielder above j on its start, which is its cell_i because it stands.  Phase 3 moves a released robot to c_r[k'], k' >= 1, which
conflicts with no current cell of another robot, or leaves it where it is.  Every move keeps the invariant, and the cells after the last
move are the final cells (a robot that moved aside is never released, so each robot moves at most once, but the argument does not need
it).  The ends of one epoch are the starts of the next, so the fact carries through a run (tests/test_world_fleet_aside_host.py checks
it by brute force over whole runs).
CONTAINMENT.  The side cell lies in the box of radius aside_reach <= reach round the start, hence in the window (CONTAINMENT above).
CLEARED.  The side cell conflicts with no cell of the walk of any r in clears(j) (class d): from its start r walks the same cells in the
next epoch, and none of them conflicts with j's new place.
No liveness is claimed.  The targets are a function of the robots' cells alone, so a run whose tuple of start cells occurred before would
repeat for good: that epoch is reported CYCLING and the run stops there; observed on the 24-robot batches of the tests (40 x 30 cells,
sep 3, box 5, 10 steps, seeds 0 .. 19): 19 of 20 open, 18 of 20 door and 9 of 20 serpentine runs arrive, each of which stalls without
the rule; the rest cycle, and one stalls.  At the fleet's own scale (400 x 400 open cells, sep 23, reach 180, 32 robots, box 48) the one
of six seeds that stalls arrives with one side step.  Planning quality with trained weights is not known.

On the device the order among yielders and among released robots is a fixed point of Jacobi sweeps: a yielder reads the side steps that the
yielders below it held after the sweep before, a released robot the side steps of this sweep and the k of the released robots below it;
both depend on lower indices only (and the release on all side steps), so the fixed point is unique, it is subgoals_aside's result,
2 n sweeps always reach it (n settle the side steps, n more the release), and changed == 0 proves it.

SUBGOAL_SEPARATION = 23 is the least separation that keeps two end points RR_MARGIN = 0.105 apart when each lies anywhere in its cell
of 0.005: centres 23 cells apart leave the points at least 23 - sqrt(2) = 21.59 cells = 0.1079 apart; 22 gives 0.1029, too little.

THE REPORT OF A RUN (run_report, opt-in; nothing above reads it).  run_report IS the definition of what a whole run's paths [N, L, 2] are
worth against the map (waypoints and n_interp interior points of every segment), against each other (every pair at every column) and
against their goals; mmd_fleet_run_report (csrc/fleet_report.hip) computes the same integers and the same float32 bits into one buffer,
which device_run_report and WorldFleet.report read with one copy.  It samples; it proves nothing between its samples.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, environments, map_textures, synth
from .multi_agent import ROBOT_RADIUS, RR_MARGIN
from .world import OBSTACLE_MARGIN, WorldRobotSampler
from .world_routes import (ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, SEED_POINTS, UNREACHED, _int32_dev, _points, cell_centres,
                           device_distance_field, sample_offsets, seed_trajectory, world_cells)

_STATUS_NAMES = {ROUTE_OK: "ok", ROUTE_UNREACHED: "unreached", ROUTE_STUCK: "stuck", ROUTE_OUTSIDE: "outside"}


# ---- the definition, on the host ---------------------------------------------------------------------------------------------------------
def _checked_walk_args(what, shape, reach, max_steps, window):
    reach, max_steps, window = int(reach), int(max_steps), int(window)
    if not (1 <= window <= min(shape) and 1 <= reach <= window // 2 - 1 and max_steps >= 1):
        raise ValueError(f"{what}: reach = {reach} (1 to window // 2 - 1), max_steps = {max_steps} (at least 1), window = {window} "
                         f"(at most min(nx, ny) = {min(shape)})")
    return reach, max_steps, window


def _walk(dist, start, goal, d0, reach, max_steps):
    """(the cell path [c_0 = start, .., c_steps], status) of window_goal's walk from a cell of the grid that holds d0 != UNREACHED"""
    nx, ny = dist.shape
    (x0, y0), (gx, gy) = start, goal
    ix, iy, d, status = x0, y0, d0, ROUTE_OK
    path = [(ix, iy)]
    while d > 0 and len(path) - 1 < max_steps:
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
        ix, iy, d = jx, jy, d - 1
        path.append((ix, iy))
    return path, status


def _walks(what, dist, starts, fields, goals, reach, max_steps, window):
    """(window_goals' three arrays, [the cell path c_0 = start .. c_steps of every query whose status is ROUTE_OK, else None]): every
    query walked once, under the caller's name `what`"""
    dist = np.asarray(dist)
    starts, goals = np.asarray(starts, np.int64).reshape(-1, 2), np.asarray(goals, np.int64).reshape(-1, 2)
    fields = np.asarray(fields, np.int64).reshape(-1)
    n_fields, nx, ny = dist.shape
    reach, max_steps, window = _checked_walk_args(what, (nx, ny), reach, max_steps, window)
    n = len(starts)
    cells, origins, summary, paths = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32), np.zeros((n, 4), np.int32), [None] * n
    for q in range(n):
        f, (x0, y0) = int(fields[q]), (int(starts[q][0]), int(starts[q][1]))
        steps, remaining, status = -1, -1, ROUTE_OUTSIDE
        if 0 <= f < n_fields and 0 <= x0 < nx and 0 <= y0 < ny:
            d0, status = int(dist[f, x0, y0]), ROUTE_UNREACHED
            if d0 != UNREACHED:
                path, status = _walk(dist[f], (x0, y0), (int(goals[f][0]), int(goals[f][1])), d0, reach, max_steps)
                steps, remaining = len(path) - 1, d0 - (len(path) - 1)
                cells[q], origins[q] = path[-1], (min(max(x0 - window // 2, 0), nx - window), min(max(y0 - window // 2, 0), ny - window))
                paths[q] = path if status == ROUTE_OK else None
        summary[q] = (steps, remaining, status, int(status == ROUTE_OK and remaining == 0))
    return (cells, origins, summary), paths


def _path_samples(paths, ks):
    """int32 [n, 64, 2]: the support cells of the paths cut at ks, samples[q, j] = c_q[sample_offsets(ks[q] + 1)[j]] over c_q[0 .. ks[q]];
    zeros where there is no path"""
    samples = np.zeros((len(paths), SEED_POINTS, 2), np.int32)
    for q, path in enumerate(paths):
        if path is not None:
            samples[q] = np.asarray(path[:ks[q] + 1], np.int32)[sample_offsets(ks[q] + 1)]
    return samples


def window_goal(dist, start, goal, reach, max_steps, window=400):
    """(cell (ix, iy), origin (i0, j0), steps, remaining, status): the next sub-goal and the window of a robot at the cell `start`, from
    the converged field dist [nx, ny] of the goal cell `goal` (the module's docstring).  status: ROUTE_OK; ROUTE_OUTSIDE (the start is not
    a cell of the grid) and ROUTE_UNREACHED (dist[start] is UNREACHED): steps = remaining = -1, cell and origin (0, 0); ROUTE_STUCK (no
    neighbour holds d - 1: the field was not converged; the outputs are what the walk covered)."""
    return window_goal_samples(dist, start, goal, reach, max_steps, window)[:5]


def window_goals(dist, starts, fields, goals, reach, max_steps, window=400):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4] = (steps, remaining, status, arrived)): window_goal for query q from
    starts[q] in field dist[fields[q]] of the goal cell goals[fields[q]]; dist [n_fields, nx, ny], goals [n_fields, 2].  A field index
    outside [0, n_fields) gives ROUTE_OUTSIDE.  arrived = 1 iff the status is ROUTE_OK and remaining == 0."""
    return _walks("window_goals", dist, starts, fields, goals, reach, max_steps, window)[0]


def window_goal_samples(dist, start, goal, reach, max_steps, window=400):
    """(cell, origin, steps, remaining, status, samples int32 [64, 2]): window_goal with the support cells of the walk's cell path.  The
    first five results are window_goal's.  The cell path is c_0 = start .. c_steps = cell, and
    samples[j] = c[sample_offsets(steps + 1)[j]] = c[(j * steps + 31) // 63]: the route seeds' spacing (world_routes.sample_offsets),
    samples[0] the start and samples[63] the sub-goal cell, every cell of the path while steps <= 63.  With a status other than ROUTE_OK
    (a stuck walk included) there are no samples: all zero, as descend_samples gives none."""
    nx, ny = np.asarray(dist).shape
    (cells, origins, summary), paths = _walks("window_goal", np.asarray(dist).reshape(1, nx, ny), [[int(start[0]), int(start[1])]], [0],
                                              [[int(goal[0]), int(goal[1])]], reach, max_steps, window)
    steps, remaining, status = (int(v) for v in summary[0, :3])
    return (tuple(int(v) for v in cells[0]), tuple(int(v) for v in origins[0]), steps, remaining, status,
            _path_samples(paths, summary[:, 0])[0])


def window_goals_samples(dist, starts, fields, goals, reach, max_steps, window=400):
    """(cells, origins, summary, samples int32 [n, 64, 2]): window_goal_samples for every query; the first three results are window_goals'
    word for word."""
    plain, paths = _walks("window_goals", dist, starts, fields, goals, reach, max_steps, window)
    return plain + (_path_samples(paths, plain[2][:, 0]),)


def window_seed(tex, lo, hi, samples, origin, window, start_point, goal_point, clearance=OBSTACLE_MARGIN, smooth_iters=64, dt=5.0 / 64):
    """(seed float32 [64, 4], clear_min float32): the seed trajectory of one robot's epoch, in trajs_final's format and in the global frame,
    from window_goal_samples' samples [64, 2] on the texture tex [nx, ny, 4] over lo .. hi.  By definition the route seed
    (world_routes.seed_trajectory) of one visit whose "tile" is the robot's window, the cells [origin, origin + window) per axis: the
    cells' centres with the caller's exact start and goal points at the ends, smooth_iters Jacobi iterations that move a support point
    to the midpoint of its neighbours iff the midpoint's texel exceeds the clearance and lies in the window, central-difference
    velocities over 2 dt, and the least texel value over the final points.
    The in-window test is a guard.  For the samples of a fleet's walk it never rejects: every sample lies in the box of radius `reach`
    round the start, the box lies in the window (CONTAINMENT), the ends lie in their cells, and the window's points are a convex set, so
    a midpoint of two points of the window is one.  It matters only for hand-built samples, which it keeps where they are."""
    return seed_trajectory(tex, lo, hi, np.asarray(samples, np.int32).reshape(1, SEED_POINTS, 2), [[0, 0]], window, origin, start_point,
                           goal_point, clearance, smooth_iters, dt)


def epoch_bound(d0, reach, max_steps):
    """The calls of window_goal, each from the cell the one before reached, that bring a robot d0 steps from its goal onto it, at most:
    ceil(d0 / min(max_steps, reach)) (PROGRESS, above)"""
    return -(-int(d0) // min(int(max_steps), int(reach)))


# ---- sub-goals kept apart: the definition ------------------------------------------------------------------------------------------------
SUBGOAL_SEPARATION = 23         # cells; the least separation that keeps two end points RR_MARGIN apart, each anywhere in its cell (docstring)


def _checked_sep(what, sep):
    if int(sep) != sep or not 1 <= int(sep) <= _lib.WINDOW_APART_MAX_SEP:
        raise ValueError(f"{what}: sep = {sep} (a whole number of cells, 1 to {_lib.WINDOW_APART_MAX_SEP})")
    return int(sep)


def _apart_choice(path, blockers, sep):
    """(k, clear) of one robot: the largest k in [1, walked] whose cell conflicts with no blocker, else 0; clear: the chosen cell conflicts
    with none.  Two cells conflict iff dx^2 + dy^2 < sep^2."""
    cells, others = np.asarray(path, np.int64).reshape(-1, 1, 2), np.asarray(blockers, np.int64).reshape(1, -1, 2)
    free = (((cells - others) ** 2).sum(-1) >= sep * sep).all(1)             # per cell of the path: it conflicts with no blocker
    feasible = np.flatnonzero(free[1:])
    return (int(feasible[-1]) + 1, 1) if feasible.size else (0, int(free[0]))


def _blockers(paths, taking, ks, r):
    """the blockers of robot r: the cells at ks of the taking-part robots j < r and the start cells of the taking-part robots j > r"""
    return [paths[j][ks[j]] for j in taking if j < r] + [paths[j][0] for j in taking if j > r]


def _apart_outputs(plain, paths, ks, clear):
    """(cells, origins, summary, extra) of the choice ks (per taking-part query) on window_goals' outputs `plain`"""
    cells, origins, summary = (a.copy() for a in plain)
    extra = np.stack([summary[:, 0], np.zeros(len(summary), np.int32)], 1).astype(np.int32)
    for q, path in enumerate(paths):
        if path is not None:
            d0 = int(summary[q, 0]) + int(summary[q, 1])
            cells[q] = path[ks[q]]
            summary[q] = (ks[q], d0 - ks[q], ROUTE_OK, int(d0 == ks[q]))
            extra[q, 1] = clear[q]
    return cells, origins, summary, extra


def subgoals_apart(dist, starts, fields, goals, reach, max_steps, sep, window=400):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4], extra int32 [n, 2]): window_goals with the sub-goals kept `sep`
    cells apart (the module's docstring, SEPARATION).  Query q takes part iff window_goals' status for it is ROUTE_OK; the robots are taken
    in index order, robot r against the chosen cells of the taking-part robots j < r and the start cells of the taking-part robots j > r,
    and takes the largest k in [1, walked] whose cell conflicts with none of them, else 0.  summary = (k, d0 - k, status, arrived) in
    window_goals' format, extra = (walked, clear).  A query that does not take part keeps window_goals' words, with extra (steps, 0)."""
    return subgoals_apart_samples(dist, starts, fields, goals, reach, max_steps, sep, window)[:4]


def subgoals_apart_sweeps(dist, starts, fields, goals, reach, max_steps, sep, n_sweeps, window=400, with_samples=False):
    """(cells, origins, summary, extra, changed[, samples]): subgoals_apart's choice as a fixed point, after n_sweeps sweeps from k = walked.
    In one sweep every robot applies subgoals_apart's rule to the k that the robots j < r held after the sweep before, all at once;
    `changed` is the number of robots whose k moved in the last sweep, `clear` what the last sweep found.  Before any sweep nothing is
    known: clear = 0 and changed = the number of queries that take part.  changed == 0 proves the fixed point, which is subgoals_apart's
    result; n sweeps always reach it (the module's docstring)."""
    sep = _checked_sep("subgoals_apart_sweeps", sep)
    if int(n_sweeps) < 0:
        raise ValueError(f"subgoals_apart_sweeps: n_sweeps = {n_sweeps} (>= 0)")
    plain, paths = _walks("window_goals", dist, starts, fields, goals, reach, max_steps, window)
    taking = [q for q, p in enumerate(paths) if p is not None]
    ks = {q: len(paths[q]) - 1 for q in taking}
    clear, changed = {q: 0 for q in taking}, len(taking)
    for _ in range(int(n_sweeps)):
        new = {}
        for r in taking:
            new[r], clear[r] = _apart_choice(paths[r], _blockers(paths, taking, ks, r), sep)
        changed = sum(new[q] != ks[q] for q in taking)
        ks = new
    return _apart_outputs(plain, paths, ks, clear) + (changed,) + ((_path_samples(paths, ks),) if with_samples else ())


def subgoals_apart_samples(dist, starts, fields, goals, reach, max_steps, sep, window=400):
    """(cells, origins, summary, extra, samples int32 [n, 64, 2]): subgoals_apart with the support cells of the shortened walks,
    samples[j] = c[(j * k + 31) // 63] over c[0 .. k]: window_goal_samples' spacing.  A query that does not take part gets zeros."""
    sep = _checked_sep("subgoals_apart", sep)
    plain, paths = _walks("window_goals", dist, starts, fields, goals, reach, max_steps, window)
    taking = [q for q, p in enumerate(paths) if p is not None]
    ks, clear = {}, {}
    for r in taking:
        ks[r], clear[r] = _apart_choice(paths[r], _blockers(paths, taking, ks, r), sep)
    return _apart_outputs(plain, paths, ks, clear) + (_path_samples(paths, ks),)


# ---- standing robots step aside: the definition --------------------------------------------------------------------------------------------
ASIDE_HELD, ASIDE_YIELDS, ASIDE_MOVED, ASIDE_RELEASED = 1, 2, 4, 8              # the role bits of aside[:, 0]


def _checked_aside(what, reach, aside_reach, aside_steps):
    if (int(aside_reach) != aside_reach or int(aside_steps) != aside_steps or not 1 <= int(aside_reach) <= min(int(reach), _lib.WINDOW_ASIDE_MAX_REACH)
            or not 1 <= int(aside_steps) <= _lib.WINDOW_ASIDE_MAX_STEPS):
        raise ValueError(f"{what}: aside_reach = {aside_reach} (1 to min(reach, {_lib.WINDOW_ASIDE_MAX_REACH}) = "
                         f"{min(int(reach), _lib.WINDOW_ASIDE_MAX_REACH)}), aside_steps = {aside_steps} (1 to {_lib.WINDOW_ASIDE_MAX_STEPS})")
    return int(aside_reach), int(aside_steps)


def _aside_levels(own, start, aside_reach, aside_steps):
    """{cell: l} for the cells with l <= aside_steps: l the 4-connected BFS distance from `start` over the cells of the grid that the field
    `own` [nx, ny] reaches and that lie within Chebyshev distance aside_reach of the start (the whole path stays among them)"""
    nx, ny = own.shape
    levels, front = {tuple(start): 0}, [tuple(start)]
    for l in range(1, aside_steps + 1):
        nxt = []
        for (x, y) in front:
            for c in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if (c not in levels and 0 <= c[0] < nx and 0 <= c[1] < ny and max(abs(c[0] - start[0]), abs(c[1] - start[1])) <= aside_reach
                        and int(own[c]) != UNREACHED):
                    levels[c] = l
                    nxt.append(c)
        front = nxt
        if not front:
            break
    return levels


def subgoals_aside(dist, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window=400):
    """(cells, origins, summary, extra, aside int32 [n, 2] = (role bits, l)): subgoals_apart, and then the standing robots step aside for
    the robots they hold back, and those walk in the same epoch (the module's docstring, STEPPING ASIDE).  The first four results are in
    subgoals_apart's formats; origins and extra are subgoals_apart's words.  Role bits: ASIDE_HELD 1, ASIDE_YIELDS 2, ASIDE_MOVED 4,
    ASIDE_RELEASED 8; l is the length of the side step, 0 unless MOVED.  A robot that moved: cell = its side cell,
    summary = (l, dist_own[side], ROUTE_OK, dist_own[side] == 0); a released robot: summary = (k', d0 - k', ROUTE_OK, d0 == k'),
    cell = c_r[k']; every other query keeps subgoals_apart's words.  aside_reach in 1 .. min(reach, 63), aside_steps in 1 .. 4095."""
    sep = _checked_sep("subgoals_aside", sep)
    plain, paths = _walks("window_goals", dist, starts, fields, goals, reach, max_steps, window)
    aside_reach, aside_steps = _checked_aside("subgoals_aside", reach, aside_reach, aside_steps)
    dist, fields = np.asarray(dist), np.asarray(fields, np.int64).reshape(-1)
    taking = [q for q, p in enumerate(paths) if p is not None]
    ks, clear = {}, {}
    for r in taking:                                         # phase 1: subgoals_apart
        ks[r], clear[r] = _apart_choice(paths[r], _blockers(paths, taking, ks, r), sep)
    cells, origins, summary, extra = _apart_outputs(plain, paths, ks, clear)
    aside = np.zeros((len(paths), 2), np.int32)
    conflict = lambda a, b: (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 < sep * sep                                       # noqa: E731
    stands = [j for j in taking if ks[j] == 0]
    held = [r for r in stands if len(paths[r]) >= 2]
    clears = {j: [r for r in held if r != j and conflict(paths[j][0], paths[r][1]) and (j not in held or r < j)] for j in stands}
    final = {q: paths[q][ks[q]] for q in taking}             # every robot's final cell, as the phases move them
    moved = {}
    for j in (j for j in stands if clears[j]):               # phase 2: the yielders, in ascending index
        own = dist[fields[j]]
        blockers = [final[i] for i in taking if i != j] + [c for r in clears[j] for c in paths[r]]
        best = min(((l, int(own[c]), c[0], c[1]) for c, l in _aside_levels(own, paths[j][0], aside_reach, aside_steps).items()
                    if l >= 1 and not any(conflict(c, b) for b in blockers)), default=None)
        if best is not None:
            moved[j], final[j] = best[0], (best[2], best[3])
            cells[j], summary[j] = final[j], (best[0], best[1], ROUTE_OK, int(best[1] == 0))
    released = [r for r in held if r not in moved and any(r in clears[j] for j in moved)]
    for r in released:                                       # phase 3: the released robots walk, in ascending index
        k, _ = _apart_choice(paths[r], [final[i] for i in taking if i != r], sep)
        d0 = int(summary[r, 0]) + int(summary[r, 1])
        final[r] = paths[r][k]
        cells[r], summary[r] = final[r], (k, d0 - k, ROUTE_OK, int(d0 == k))
    for q in taking:
        aside[q] = (ASIDE_HELD * (q in held) | ASIDE_YIELDS * bool(clears.get(q)) | ASIDE_MOVED * (q in moved) | ASIDE_RELEASED * (q in released),
                    moved.get(q, 0))
    return cells, origins, summary, extra, aside


# ---- the report of a run: the definition ---------------------------------------------------------------------------------------------------
REPORT_MAX_ROBOTS, REPORT_MAX_LENGTH, REPORT_MAX_INTERP = 4096, 65535, 63       # MMD_FLEET_REPORT_MAX_*
REPORT_HEADER = 8                                                              # MMD_FLEET_REPORT_HEADER: int32 words before the arrays
_INT_WORDS = ("points_hit", "interp_hit", "first_hit", "bad_points", "outside", "arrival")       # the report's arrays behind the conflicts,
_FLOAT_WORDS = ("clear_min", "length", "max_step", "end_error")                                  # in the buffer's order
_NAN_BITS, _INF_BITS = 0x7fc00000, 0x7f800000


class RunReport(NamedTuple):
    """What run_report, device_run_report and WorldFleet.report return: numpy on the host.  Per robot [N]:"""
    points_hit: np.ndarray      # int32: waypoints whose value is < margin
    interp_hit: np.ndarray      # int32: interior points whose value is < margin
    first_hit: np.ndarray       # int32: the least t whose waypoint, or an interior point of segment t, is hit; -1 if none
    bad_points: np.ndarray      # int32: waypoints with a coordinate that is not finite
    outside: np.ndarray         # int32: finite waypoints outside lo .. hi (they read the clamped border texel and still take part)
    arrival: np.ndarray         # int32: the least c with every column t >= c finite and within goal_tol of the goal; L if the last is not
    conflicts: np.ndarray       # int32: the (t, other robot) in collision
    clear_min: np.ndarray       # float32: the least value over all points checked (a NaN beyond the infinity of its sign); +inf if none
    length: np.ndarray          # float32: the sum of the segment lengths
    max_step: np.ndarray        # float32: the longest segment; 0 if there is none
    end_error: np.ndarray       # float32: ||p[L - 1] - goal||; NaN if that point or the goal is bad
    # per run
    conflict_count: int         # the pairs i < j in collision, summed over the columns: half the sum of `conflicts`
    first_conflict: tuple       # (t, i, j), the least t, then i, then j; (-1, -1, -1) if there is none
    robots_hit: int
    robots_in_conflict: int
    robots_arrived: int
    column_conflicts: np.ndarray = None         # int32 [L]: the pairs in collision per column; None unless asked for


def torch_norm2(dx, dy):
    """sqrt(fma(dy, dy, dx * dx)) in float32, csrc/collision_dev.h's torch_norm2 bit for bit: the product dx * dx rounded to float32, the
    fma's exact sum formed in float64 with its error term (TwoSum) and rounded to odd, so that the cast to float32 is the fma's one
    rounding (53 >= 2 * 24 + 2 bits); an infinite or NaN sum stays what it is."""
    dx, dy = np.atleast_1d(np.asarray(dx, np.float32)), np.atleast_1d(np.asarray(dy, np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        c, y = (dx * dx).astype(np.float64), dy.astype(np.float64)
        p = y * y
        s = np.ascontiguousarray(p + c)
        b = s - p
        e = (p - (s - b)) + (c - b)
        odd = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(odd, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return np.sqrt(s.astype(np.float32))


def _order_key(bits):
    """csrc/seed_dev.h's order_key on int32 bits: an int32 that orders like the float (a NaN beyond the infinity of its sign); its own inverse"""
    return bits ^ ((bits >> 31) & 0x7fffffff)


def _checked_report_args(what, n, length, tex_shape, lo, hi, margin, rr_margin, n_interp, goal_tol):
    """(margin, rr_margin, goal_tol as float32, n_interp as int) after the refusals that run_report and device_run_report share; goal_tol
    None: the texture's cell pitch, the larger axis's"""
    f = np.float32
    if len(tex_shape) != 3 or tex_shape[2] != 4:
        raise ValueError(f"{what}: a texture [nx, ny, 4], got {tuple(tex_shape)}")
    if not (1 <= n <= REPORT_MAX_ROBOTS and 2 <= length <= REPORT_MAX_LENGTH):
        raise ValueError(f"{what}: paths [N, L, 2] with N = {n} (1 .. {REPORT_MAX_ROBOTS}) and L = {length} (2 .. {REPORT_MAX_LENGTH})")
    lo, hi = np.asarray(lo, f).reshape(-1), np.asarray(hi, f).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        dim = np.abs(hi - lo)
    if lo.shape != (2,) or hi.shape != (2,) or not (np.isfinite(lo).all() and np.isfinite(dim).all() and (dim > 0).all()):
        raise ValueError(f"{what}: limits {lo.tolist()} .. {hi.tolist()} (two finite points, a non-zero extent per axis)")
    n_interp = int(n_interp)
    if goal_tol is None:
        goal_tol = max(dim[0] / f(tex_shape[0]), dim[1] / f(tex_shape[1]))
    with np.errstate(over="ignore"):
        margin, rr_margin, goal_tol = f(margin), f(rr_margin), f(goal_tol)
    if not (np.isfinite(margin) and np.isfinite(rr_margin) and np.isfinite(goal_tol) and goal_tol >= 0 and 0 <= n_interp <= REPORT_MAX_INTERP):
        raise ValueError(f"{what}: margin = {margin} and rr_margin = {rr_margin} (finite), goal_tol = {goal_tol} (finite, >= 0), "
                         f"n_interp = {n_interp} (0 .. {REPORT_MAX_INTERP})")
    return margin, rr_margin, goal_tol, n_interp


def segment_lengths(paths):
    """float32 [N, L - 1]: torch_norm2(p[t + 1] - p[t]) of paths [N, L, 2], 0 for a segment with a bad end: the terms of run_report's
    `length` and `max_step`"""
    p = np.asarray(paths, np.float32)
    fin = np.isfinite(p).all(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        d = p[:, 1:] - p[:, :-1]
    return np.where(fin[:, 1:] & fin[:, :-1], torch_norm2(d[..., 0].reshape(-1), d[..., 1].reshape(-1)).reshape(d.shape[:2]), np.float32(0))


def run_report(paths, tex, lo, hi, goals, margin, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
    """RunReport of paths float32 [N, L, 2] (global points; N in 1 .. 4096, L in 2 .. 65535) on any texture tex [nx, ny, 4] over lo .. hi,
    with goals float32 [N, 2]: THE DEFINITION of mmd_fleet_run_report's words.

    Every decision is float32, operation by operation.  A texel is environments._texel_indices' (mmd_sdf_grid_lookup's sequence), a value
    channel 0 of the texel, the norm torch_norm2.  A point with a coordinate that is not finite is BAD: it is counted in bad_points and
    takes part in nothing else, nor does a segment with a bad end.  Segment t runs from a = p[t] to b = p[t + 1]; its interior points are
    q_j = a + (b - a) * (float32(j) / float32(n_interp + 1)), j = 1 .. n_interp (n_interp in 0 .. 63): subtract, multiply, add, three
    roundings; an interior point that is not finite (the difference overflowed) is not checked and not counted.  A waypoint or interior
    point is HIT iff its value is < margin (strict; a NaN value is no hit); a pair of robots is in conflict at column t iff both points
    are finite and torch_norm2(p_i[t] - p_j[t]) < rr_margin; a robot stands on its goal at column t iff the point is finite and
    torch_norm2(p[t] - goal) <= goal_tol.  goal_tol=None: the texture's cell pitch (the larger axis's) -- the map resolves positions no
    finer, and a path's end is exact only on worlds whose arithmetic is.  `length` is the float64 sum of segment_lengths' float32 terms,
    rounded to float32; the device adds the same terms in float32 in a fixed order, so `length` alone is equal only within L * 2^-24.

    The paths are taken as given.  In a FleetResult column 64 e + 63 and column 64 (e + 1) are the same instant: the report sees a
    segment of length zero there, and a conflict at that instant counts in both columns.

    What this does NOT prove: a segment is sampled at n_interp points, not swept, so an obstacle thinner than the spacing of the samples
    can lie between two of them; and robot against robot is tested at the waypoints only, not between them."""
    f = np.float32
    p = np.ascontiguousarray(environments._host_array(paths), dtype=f)
    tex = np.ascontiguousarray(environments._host_array(tex), dtype=f)
    if p.ndim != 3 or p.shape[2] != 2:
        raise ValueError(f"run_report: paths [N, L, 2], got {p.shape}")
    n, length = p.shape[:2]
    margin, rr_margin, goal_tol, n_interp = _checked_report_args("run_report", n, length, tex.shape, lo, hi, margin, rr_margin, n_interp, goal_tol)
    g = np.ascontiguousarray(environments._host_array(goals), dtype=f)
    if g.shape != (n, 2):
        raise ValueError(f"run_report: goals [{n}, 2], got {g.shape}")
    lo32, hi32 = np.asarray(lo, f).reshape(2), np.asarray(hi, f).reshape(2)
    key_inf = np.int32(_INF_BITS)

    def values(points, shape):
        ix, iy, _ = environments._texel_indices(points.reshape(-1, 2), lo, hi, tex.shape[:2])
        return np.ascontiguousarray(tex[ix, iy, 0]).reshape(shape)

    def keys(v, taking):
        return np.where(taking, _order_key(v.view(np.int32)), key_inf)

    with np.errstate(over="ignore", invalid="ignore"):
        fin = np.isfinite(p).all(-1)                                             # [N, L]
        val = values(p, (n, length))
        hit = fin & (val < margin)
        outside = fin & ~((p >= lo32) & (p <= hi32)).all(-1)
        clear_key = keys(val, fin).min(1)
        seg = fin[:, :-1] & fin[:, 1:]
        d = p[:, 1:] - p[:, :-1]
        seg_hit, interp_hit = hit.copy(), np.zeros(n, np.int64)
        for j in range(1, n_interp + 1):
            q = p[:, :-1] + d * (f(j) / f(n_interp + 1))
            taking = seg & np.isfinite(q).all(-1)
            qv = values(q, (n, length - 1))
            q_hit = taking & (qv < margin)
            interp_hit += q_hit.sum(1)
            seg_hit[:, :-1] |= q_hit
            clear_key = np.minimum(clear_key, keys(qv, taking).min(1))
        lengths = segment_lengths(p)
        off_goal = ~(fin & (torch_norm2((p[..., 0] - g[:, None, 0]).reshape(-1), (p[..., 1] - g[:, None, 1]).reshape(-1)).reshape(n, length) <= goal_tol))
        last = p[:, -1] - g
        end_error = np.where(fin[:, -1] & np.isfinite(g).all(1), torch_norm2(last[:, 0], last[:, 1]), np.array(_NAN_BITS, np.int32).view(f))
        # robot against robot, a block of columns at a time
        conflicts, columns, first = np.zeros(n, np.int64), np.zeros(length, np.int64), (-1, -1, -1)
        upper = np.triu(np.ones((n, n), bool), 1)
        block = max(1, (1 << 21) // (n * n))
        for t0 in range(0, length if n > 1 else 0, block):
            pt = p[:, t0:t0 + block].transpose(1, 0, 2)                          # [B, N, 2]
            ft = fin[:, t0:t0 + block].T
            dd = pt[:, :, None, :] - pt[:, None, :, :]
            h = (torch_norm2(dd[..., 0].reshape(-1), dd[..., 1].reshape(-1)).reshape(dd.shape[:3]) < rr_margin) & ft[:, :, None] & ft[:, None, :]
            h &= ~np.eye(n, dtype=bool)
            conflicts += h.sum((0, 2))
            pairs = h & upper
            columns[t0:t0 + block] = pairs.sum((1, 2))
            if first[0] < 0 and pairs.any():
                first = tuple(int(v) + (t0 if k == 0 else 0) for k, v in enumerate(np.argwhere(pairs)[0]))
    points_hit = hit.sum(1)
    arrival = np.where(off_goal.any(1), length - off_goal[:, ::-1].argmax(1), 0)
    i32 = lambda a: np.asarray(a).astype(np.int32)                               # noqa: E731
    return RunReport(i32(points_hit), i32(interp_hit), i32(np.where(seg_hit.any(1), seg_hit.argmax(1), -1)), i32((~fin).sum(1)),
                     i32(outside.sum(1)), i32(arrival), i32(conflicts), _order_key(clear_key.astype(np.int32)).view(f),
                     lengths.astype(np.float64).sum(1).astype(f), lengths.max(1).astype(f), end_error.astype(f),
                     int(columns.sum()), first, int((points_hit + interp_hit > 0).sum()), int((conflicts > 0).sum()),
                     int((arrival < length).sum()), i32(columns) if column_conflicts else None)


# ---- the same on the device ----------------------------------------------------------------------------------------------------------------
def _checked_launch_args(what, dist_dev, reach, max_steps, window):
    """(reach, max_steps, window) as ints, after the checks of dist_dev and of the walk's arguments under the name `what`: the first
    refusals of every sub-goal launch, before anything is uploaded"""
    if dist_dev.dim() != 3 or dist_dev.dtype != torch.int32 or not dist_dev.is_cuda or not dist_dev.is_contiguous():
        raise ValueError(f"{what}: dist must be a contiguous int32 CUDA(HIP) tensor [n_fields, nx, ny]")
    return _checked_walk_args(what, tuple(dist_dev.shape[1:]), reach, max_steps, window)


def _walk_launch_args(what, dist_dev, starts, fields, goals, reach, max_steps, window):
    """(the eleven leading arguments of the three sub-goal entry points, n, the uploaded starts, fields and goals behind three of them:
    hold them until the launch); reach, max_steps and window are _checked_launch_args' """
    starts_dev = _int32_dev(starts, (-1, 2), dist_dev.device, f"{what}: starts")
    n = starts_dev.shape[0]
    fields_dev = _int32_dev(fields, (n,), dist_dev.device, f"{what}: fields")
    goals_dev = _int32_dev(goals, (int(dist_dev.shape[0]), 2), dist_dev.device, f"{what}: goals")
    lead = (C.c_void_p(dist_dev.data_ptr()), int(dist_dev.shape[1]), int(dist_dev.shape[2]), int(dist_dev.shape[0]),
            C.c_void_p(starts_dev.data_ptr()), C.c_void_p(fields_dev.data_ptr()), C.c_void_p(goals_dev.data_ptr()), n, reach, max_steps, window)
    return lead, n, (starts_dev, fields_dev, goals_dev)


def _window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window, with_samples=False, what="device_window_goals"):
    """device_window_goals' launch -> (one int32 tensor [8 n] on the device: cells [n, 2], then origins [n, 2], then summary [n, 4]; None).
    with_samples: device_window_goal_samples' launch (mmd_grid_window_goal_samples) -> (that tensor, samples int32 [n, 64, 2])"""
    lead, n, _uploads = _walk_launch_args(what, dist_dev, starts, fields, goals, *_checked_launch_args(what, dist_dev, reach, max_steps, window))
    words = torch.empty(8 * n, dtype=torch.int32, device=dist_dev.device)        # (the summary rows start 16 n bytes in: aligned as int4)
    at = lambda k: C.c_void_p(words.data_ptr() + 4 * k)                          # noqa: E731
    if not with_samples:
        _lib.launch("mmd_grid_window_goals", dist_dev, *lead, at(0), at(2 * n), at(4 * n))
        return words, None
    samples = torch.empty(n, SEED_POINTS, 2, dtype=torch.int32, device=dist_dev.device)
    _lib.launch("mmd_grid_window_goal_samples", dist_dev, *lead, at(0), at(2 * n), at(4 * n), C.c_void_p(samples.data_ptr()))
    return words, samples


def _split_words(words, apart=False, aside=False):
    """(cells [n, 2], origins [n, 2], summary [n, 4][, extra [n, 2][, aside [n, 2]]]), views of a sub-goal launch's words, a tensor or its
    numpy copy: [8 n], or with `apart` mmd_grid_window_goals_apart's [10 n + 1], with extra and changed behind, or with `aside`
    mmd_grid_window_goals_aside's [12 n + 1], with extra, aside and changed behind"""
    n = (words.shape[0] - 1) // (12 if aside else 10) if apart or aside else words.shape[0] // 8
    out = words[:2 * n].reshape(n, 2), words[2 * n:4 * n].reshape(n, 2), words[4 * n:8 * n].reshape(n, 4)
    return out + ((words[8 * n:10 * n].reshape(n, 2),) if apart or aside else ()) + ((words[10 * n:12 * n].reshape(n, 2),) if aside else ())


def device_window_goals(dist_dev, starts, fields, goals, reach, max_steps, window=400):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4]) on dist_dev's device: window_goals() for every query in one launch
    (mmd_grid_window_goals), word for word.  dist_dev: any int32 fields [n_fields, nx, ny] (device_distance_field's, or hand-built
    ones); goals [n_fields, 2]: the fields' goal cells.  The three results are views of one tensor."""
    return _split_words(_window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window)[0])


def device_window_goal_samples(dist_dev, starts, fields, goals, reach, max_steps, window=400):
    """(cells, origins, summary, samples int32 [n, 64, 2]) on dist_dev's device: window_goals_samples() for every query in one launch
    (mmd_grid_window_goal_samples), word for word.  The first three are device_window_goals' (views of one tensor); dist_dev: any int32
    fields, as there.  The samples of a query whose status is not ROUTE_OK are zero."""
    words, samples = _window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window, True, "device_window_goal_samples")
    return _split_words(words) + (samples,)


def device_window_seeds(tex_dev, lo, hi, samples, origins, summary, window, start_points, goal_points, clearance=OBSTACLE_MARGIN,
                        smooth_iters=64, dt=5.0 / 64):
    """(seeds float32 [n, 64, 4], clear_min float32 [n]) on tex_dev's device: window_seed() for every robot in one launch
    (mmd_window_seeds), bit for bit, from device_window_goal_samples' samples [n, 64, 2], origins [n, 2] and summary [n, 4] (or any
    contiguous int32 tensors of those shapes on the texture's device) on any texture [nx, ny, 4] over lo .. hi.  The seeds are global
    points, in trajs_final's format; every row of a robot whose status is not ROUTE_OK is zero, and so is its clear_min."""
    if tex_dev.dim() != 3 or tex_dev.shape[2] != 4:
        raise ValueError(f"device_window_seeds: a texture [nx, ny, 4], got {tuple(tex_dev.shape)}")
    tex_p = _lib.require_gpu(tex_dev, "texture")
    dev = tex_dev.device
    ok = lambda t, shape: (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and t.is_contiguous()      # noqa: E731
                           and tuple(t.shape[1:]) == shape)
    if not (ok(summary, (4,)) and summary.shape[0] >= 1 and ok(samples, (SEED_POINTS, 2)) and ok(origins, (2,))
            and samples.shape[0] == origins.shape[0] == summary.shape[0]):
        raise ValueError("device_window_seeds: samples [n, 64, 2], origins [n, 2] and summary [n, 4], contiguous int32 on the texture's "
                         "device, as device_window_goal_samples returns them")
    n = int(summary.shape[0])
    two_dt = float(np.float32(2.0 * float(dt)))
    if int(smooth_iters) < 0 or not (np.isfinite(two_dt) and two_dt > 0) or int(window) < 1:
        raise ValueError(f"device_window_seeds: smooth_iters = {smooth_iters} (>= 0), dt = {dt} (finite, > 0), window = {window} (>= 1)")
    pts = [torch.as_tensor(p, dtype=torch.float32).reshape(n, 2).contiguous().to(dev) for p in (start_points, goal_points)]
    seeds = torch.empty(n, SEED_POINTS, 4, dtype=torch.float32, device=dev)
    clear_min = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.launch("mmd_window_seeds", tex_dev, tex_p, int(tex_dev.shape[0]), int(tex_dev.shape[1]), (C.c_float * 2)(*map(float, lo)),
                (C.c_float * 2)(*map(float, hi)), float(clearance), C.c_void_p(samples.data_ptr()), C.c_void_p(origins.data_ptr()),
                C.c_void_p(summary.data_ptr()), n, int(window), C.c_void_p(pts[0].data_ptr()), C.c_void_p(pts[1].data_ptr()),
                int(smooth_iters), two_dt, C.c_void_p(seeds.data_ptr()), C.c_void_p(clear_min.data_ptr()))
    return seeds, clear_min


def device_epoch_frames(name, words, points, goal_points, norm_mins=synth.NORM_MINS, norm_maxs=synth.NORM_MAXS, line_a=None):
    """(offsets float32 [n, 2], sub-goal points [n, 2], hard conditions [n, 4] of row 0 and of row 63, straight lines [n, 64, 2]), views
    of one tensor on the words' device: everything a WorldRobotSampler's state takes from an epoch's targets on the world map `name`,
    in one launch (mmd_fleet_epoch_frames) and bit for bit what the host gives -- environments.world_map_window_offsets of the
    origins; world_routes.cell_centres of the cells, or goal_points[r] where summary[r, 3] == 1; the constructor's normalised
    (point - offset, 0, 0) of `points` and of the sub-goal points; synth.straight_line_paths(points, sub-goal points).
    words: int32 [8 n] on the device, a sub-goal launch's (cells, origins, summary) in _split_words' layout -- any words: nothing is
    indexed by them, and nothing is validated (WorldFleet has refused a robot whose status is not ROUTE_OK before this).  points:
    float32 on that device, [n, 2] in rows of any even stride (the last points paths[:, -1] of paths [n, 64, 2] are taken as they
    lie); goal_points float32 [n, 2], contiguous, on that device.  The constants the host definitions compute once are computed
    here by those same expressions; line_a: numpy.linspace(0, 1, 64, dtype=float32) on the device, uploaded here if not given."""
    if not (isinstance(words, torch.Tensor) and words.dtype == torch.int32 and words.is_cuda and words.dim() == 1 and words.is_contiguous()
            and words.shape[0] >= 8 and words.shape[0] % 8 == 0):
        raise ValueError("device_epoch_frames: words must be a contiguous int32 CUDA(HIP) tensor [8 n], n >= 1, as a sub-goal launch leaves it")
    n, dev = words.shape[0] // 8, words.device
    ok = lambda t: isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (n, 2)     # noqa: E731
    if not (ok(points) and points.stride(1) == 1 and points.stride(0) >= 2 and points.stride(0) % 2 == 0
            and points.data_ptr() % 8 == 0 and ok(goal_points) and goal_points.is_contiguous()):
        raise ValueError(f"device_epoch_frames: points (rows of an even stride) and goal_points (contiguous), float32 [{n}, 2] on {dev}")
    if line_a is None:
        line_a = torch.from_numpy(np.linspace(0.0, 1.0, SEED_POINTS, dtype=np.float32)).to(dev)
    lo, hi = (np.asarray(v, np.float32) for v in environments.world_map_limits(name))
    pitch = np.abs(hi - lo) / np.asarray(environments.world_map_occupancy(name).shape[:2], np.float32)        # cell_centres' pitch
    mins, maxs = np.asarray(norm_mins, np.float32), np.asarray(norm_maxs, np.float32)
    out = torch.empty(140 * n, dtype=torch.float32, device=dev)       # offsets 2 n, points 2 n, hard 4 n + 4 n, lines 128 n
    at = lambda k: C.c_void_p(out.data_ptr() + 4 * k)                 # noqa: E731
    word = lambda k: C.c_void_p(words.data_ptr() + 4 * k)             # noqa: E731
    _lib.launch("mmd_fleet_epoch_frames", words, word(0), word(2 * n), word(4 * n), C.c_void_p(points.data_ptr()), int(points.stride(0)),
                C.c_void_p(goal_points.data_ptr()), n,
                (C.c_double * 5)(environments.SDF_CELL_SIZE, *map(float, environments.world_map_origin(name)), *map(float, environments.LIMITS[0])),
                (C.c_float * 4)(*map(float, lo), *map(float, pitch)), (C.c_float * 4)(*map(float, mins)), (C.c_float * 4)(*map(float, maxs - mins)),
                C.c_void_p(line_a.data_ptr()), at(0), at(2 * n), at(4 * n), at(8 * n), at(12 * n))
    return (out[:2 * n].view(n, 2), out[2 * n:4 * n].view(n, 2), out[4 * n:8 * n].view(n, 4), out[8 * n:12 * n].view(n, 4),
            out[12 * n:].view(n, SEED_POINTS, 2))


def _subgoals_apart_words(dist_dev, starts, fields, goals, reach, max_steps, sep, window, sweeps, with_samples, what="device_subgoals_apart",
                          kept=None):
    """device_subgoals_apart's launches -> (one int32 tensor [10 n + 1] on the device: cells [n, 2], origins [n, 2], summary [n, 4],
    extra [n, 2], changed [1]; its last copy on the host, numpy; samples int32 [n, 64, 2] on the device or None; the sweeps run).
    kept: a dict that receives the workspace at its fixed point, its size, the launch's leading arguments with their uploads, and n, for
    the launch that continues from it (_subgoals_aside_words)"""
    reach, max_steps, window = _checked_launch_args(what, dist_dev, reach, max_steps, window)
    sep, sweeps = _checked_sep(what, sep), int(sweeps)
    if max_steps > _lib.WINDOW_APART_MAX_STEPS or sweeps < 1:
        raise ValueError(f"{what}: max_steps = {max_steps} (at most {_lib.WINDOW_APART_MAX_STEPS}), sweeps = {sweeps} (at least 1)")
    lead, n, _uploads = _walk_launch_args(what, dist_dev, starts, fields, goals, reach, max_steps, window)
    work_bytes = int(_lib.load().mmd_grid_window_apart_work_bytes(n, max_steps))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dist_dev.device)
    words = torch.empty(10 * n + 1, dtype=torch.int32, device=dist_dev.device)     # (the summary rows start 16 n bytes in: aligned as int4)
    samples = torch.empty(n, SEED_POINTS, 2, dtype=torch.int32, device=dist_dev.device) if with_samples else None
    at = lambda k: C.c_void_p(words.data_ptr() + 4 * k)                          # noqa: E731

    def launch(restart, n_sweeps):
        _lib.launch("mmd_grid_window_goals_apart", dist_dev, *lead, sep, restart, n_sweeps, C.c_void_p(work.data_ptr()), work_bytes, at(0),
                    at(2 * n), at(4 * n), at(8 * n), C.c_void_p(samples.data_ptr()) if with_samples else None, at(10 * n))
        return words.cpu().numpy()
    run = min(sweeps, n + 1)
    host = launch(1, run)
    while host[10 * n] != 0 and run < n + 1:                 # n sweeps reach the fixed point, one more reads changed == 0
        more = min(sweeps, n + 1 - run)
        host, run = launch(0, more), run + more
    if host[10 * n] != 0:
        raise RuntimeError(f"{what}: {int(host[10 * n])} robots still moved in sweep {run} of {n} robots: the workspace was disturbed")
    if kept is not None:
        kept.update(work=work, work_bytes=work_bytes, lead=lead, uploads=_uploads, n=n)
    return words, host, samples, run


def device_subgoals_apart(dist_dev, starts, fields, goals, reach, max_steps, sep, window=400, sweeps=4, with_samples=False):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4], extra int32 [n, 2][, samples int32 [n, 64, 2]], n_sweeps_run) on
    dist_dev's device: subgoals_apart() (with samples: subgoals_apart_samples()) for every query, word for word, by
    mmd_grid_window_goals_apart: a restart call with `sweeps` sweeps, then, while `changed` is not zero, `sweeps` more, at most n + 1 in
    all, the first call included (n reach the fixed point, the one after reads changed == 0).  No queries at all are refused, as
    device_window_goals refuses them.  Every call ends with one device -> host copy of all words, extra
    and changed, which live in one tensor: the common case costs one copy.  The first four results are views of that tensor."""
    words, _, samples, run = _subgoals_apart_words(dist_dev, starts, fields, goals, reach, max_steps, sep, window, sweeps, with_samples)
    return _split_words(words, apart=True) + ((samples,) if with_samples else ()) + (run,)


def _subgoals_aside_words(dist_dev, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window, sweeps,
                          what="device_subgoals_aside"):
    """device_subgoals_aside's launches -> (one int32 tensor [12 n + 1] on the device: cells [n, 2], origins [n, 2], summary [n, 4],
    extra [n, 2], aside [n, 2], changed [1]; its last copy on the host, numpy; the sweeps of phase 1; the sweeps run here).  Phase 1 is
    _subgoals_apart_words' loop to its fixed point, whose workspace mmd_grid_window_goals_aside then reads."""
    reach, max_steps, window = _checked_launch_args(what, dist_dev, reach, max_steps, window)
    sep = _checked_sep(what, sep)
    aside_reach, aside_steps = _checked_aside(what, reach, aside_reach, aside_steps)
    kept = {}
    _, _, _, apart_run = _subgoals_apart_words(dist_dev, starts, fields, goals, reach, max_steps, sep, window, sweeps, False, what, kept)
    n, lead, sweeps = kept["n"], kept["lead"], int(sweeps)
    work_bytes = int(_lib.load().mmd_grid_window_aside_work_bytes(n))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dist_dev.device)
    words = torch.empty(12 * n + 1, dtype=torch.int32, device=dist_dev.device)     # (the summary rows start 16 n bytes in: aligned as int4)
    at = lambda k: C.c_void_p(words.data_ptr() + 4 * k)                          # noqa: E731

    def launch(restart, n_sweeps):
        _lib.launch("mmd_grid_window_goals_aside", dist_dev, *lead[:4], lead[5], n, reach, max_steps, window, sep, aside_reach, aside_steps,
                    restart, n_sweeps, C.c_void_p(kept["work"].data_ptr()), kept["work_bytes"], C.c_void_p(work.data_ptr()), work_bytes, at(0),
                    at(2 * n), at(4 * n), at(8 * n), at(10 * n), at(12 * n))
        return words.cpu().numpy()
    cap = 2 * n + 1                                          # 2 n sweeps reach the fixed point, one more reads changed == 0
    run = min(sweeps, cap)
    host = launch(1, run)
    while host[12 * n] != 0 and run < cap:
        more = min(sweeps, cap - run)
        host, run = launch(0, more), run + more
    if host[12 * n] != 0:
        raise RuntimeError(f"{what}: {int(host[12 * n])} robots still moved in sweep {run} of {n} robots: the workspace was disturbed")
    return words, host, apart_run, run


def device_subgoals_aside(dist_dev, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window=400, sweeps=4):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4], extra int32 [n, 2], aside int32 [n, 2], n_sweeps_run) on dist_dev's
    device: subgoals_aside() for every query, word for word.  Phase 1 is device_subgoals_apart's loop; then
    mmd_grid_window_goals_aside on its workspace: a restart call with `sweeps` sweeps, then, while `changed` is not zero, `sweeps` more, at
    most 2 n + 1 in all (2 n reach the fixed point, the one after reads changed == 0); n_sweeps_run counts these, not phase 1's.  Every call
    of either entry point ends with one device -> host copy of all its words.  The five arrays are views of one tensor."""
    words, _, _, run = _subgoals_aside_words(dist_dev, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window, sweeps)
    return _split_words(words, aside=True) + (run,)


def device_run_report_words(paths_dev, tex_dev, lo, hi, goals, margin, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
    """mmd_fleet_run_report's launch -> its one buffer, int32 [8 + 11 N (+ L)] on the paths' device, in include/mmd_amd.h's layout
    (report_from_words reads a copy of it).  paths_dev: contiguous float32 [N, L, 2] on a GPU; tex_dev: any texture [nx, ny, 4] on that
    device; goals [N, 2]: a tensor there, or anything on the host, which is uploaded.  Nothing is copied back."""
    what = "device_run_report"
    if not (isinstance(paths_dev, torch.Tensor) and paths_dev.dim() == 3 and paths_dev.shape[2] == 2):
        raise ValueError(f"{what}: paths [N, L, 2], got {tuple(getattr(paths_dev, 'shape', ()))}")
    paths_p = _lib.require_gpu(paths_dev, "paths")
    if not isinstance(tex_dev, torch.Tensor) or tex_dev.device != paths_dev.device:
        raise ValueError(f"{what}: the texture must be a tensor on the paths' device {paths_dev.device}")
    n, length = int(paths_dev.shape[0]), int(paths_dev.shape[1])
    margin, rr_margin, goal_tol, n_interp = _checked_report_args(what, n, length, tuple(tex_dev.shape), lo, hi, margin, rr_margin, n_interp, goal_tol)
    tex_p = _lib.require_gpu(tex_dev, "texture")
    goals_dev = torch.as_tensor(goals, dtype=torch.float32)
    if tuple(goals_dev.shape) != (n, 2):
        raise ValueError(f"{what}: goals [{n}, 2], got {tuple(goals_dev.shape)}")
    goals_dev = goals_dev.contiguous().to(paths_dev.device)
    words = torch.empty(REPORT_HEADER + (len(_INT_WORDS) + 1 + len(_FLOAT_WORDS)) * n + (length if column_conflicts else 0), dtype=torch.int32,
                        device=paths_dev.device)
    _lib.launch("mmd_fleet_run_report", paths_dev, paths_p, n, length, tex_p, int(tex_dev.shape[0]), int(tex_dev.shape[1]),
                (C.c_float * 2)(*map(float, np.asarray(lo, np.float32).reshape(2))), (C.c_float * 2)(*map(float, np.asarray(hi, np.float32).reshape(2))),
                C.c_void_p(goals_dev.data_ptr()), float(margin), float(rr_margin), n_interp, float(goal_tol), int(bool(column_conflicts)),
                C.c_void_p(words.data_ptr()))
    return words


def report_from_words(words, n, length, column_conflicts=False):
    """RunReport of mmd_fleet_run_report's buffer, as a numpy int32 copy on the host"""
    w = np.ascontiguousarray(words, dtype=np.int32)
    n_cols = length if column_conflicts else 0
    if w.shape != (REPORT_HEADER + (len(_INT_WORDS) + 1 + len(_FLOAT_WORDS)) * n + n_cols,):
        raise ValueError(f"report_from_words: {w.shape} words for N = {n}, L = {length}, column_conflicts = {bool(column_conflicts)}")
    count, key = (int(v) for v in w[:4].view(np.uint64))
    first = (-1, -1, -1) if key == 0xFFFFFFFFFFFFFFFF else (key >> 24, (key >> 12) & 0xFFF, key & 0xFFF)
    at = REPORT_HEADER + n + n_cols
    rows = w[at:].reshape(-1, n)
    ints, floats = rows[:len(_INT_WORDS)], rows[len(_INT_WORDS):].view(np.float32)
    return RunReport(*(r.copy() for r in ints), w[REPORT_HEADER:REPORT_HEADER + n].copy(), *(r.copy() for r in floats), count, first,
                     int(w[4]), int(w[5]), int(w[6]), w[REPORT_HEADER + n:at].copy() if column_conflicts else None)


def device_run_report(paths_dev, tex_dev, lo, hi, goals, margin, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
    """run_report() of paths on the device, by mmd_fleet_run_report (two kernels, one buffer) and ONE device -> host copy: every integer,
    clear_min, max_step and end_error bit for bit, `length` within L * 2^-24 (a float32 sum in the device's fixed order).  Any contiguous
    float32 paths [N, L, 2] and any texture [nx, ny, 4] on one GPU; the arguments and their refusals are run_report's."""
    words = device_run_report_words(paths_dev, tex_dev, lo, hi, goals, margin, rr_margin, n_interp, goal_tol, column_conflicts)
    return report_from_words(words.cpu().numpy(), int(paths_dev.shape[0]), int(paths_dev.shape[1]), column_conflicts)


# ---- the fleet -----------------------------------------------------------------------------------------------------------------------------
class EpochTargets(NamedTuple):
    """What one epoch plans towards (WorldFleet.epoch_targets): numpy on the host, and the launch's own tensors on the device."""
    cells: np.ndarray           # int32 [N, 2]: the sub-goal cells in the world
    origins: np.ndarray         # int32 [N, 2]: the windows' origin cells
    offsets: np.ndarray         # float32 [N, 2]: the windows' offsets (environments.world_map_window_offsets)
    points: np.ndarray          # float32 [N, 2]: the sub-goal points, global: the cell's centre, or the robot's exact goal once `arrived`
    summary: np.ndarray         # int32 [N, 4]: (steps, remaining, status, arrived)
    samples: torch.Tensor = None    # seed_epochs: int32 [N, 64, 2] on the device, the walks' support cells (never copied back); else None
    words: torch.Tensor = None      # int32 [8 N] on the device, (cells, origins, summary) as launched (_split_words); with separation a view
    extra: np.ndarray = None        # separation: int32 [N, 2] = (walked, clear) of subgoals_apart; else None
    sweeps: int = None              # separation: the sweeps device_subgoals_apart ran; else None
    aside: np.ndarray = None        # step_aside: int32 [N, 2] = (role bits, l) of subgoals_aside; else None


class FleetResult(NamedTuple):
    """What WorldFleet.run returns."""
    paths: torch.Tensor         # float32 [N, E * 64, 2] on the device, global: epoch e's paths are columns [64 e, 64 e + 64)
    arrived: np.ndarray         # bool [N]: the robot stands on its exact goal point
    # per epoch {"conflict_counts", "summary", "offsets"}: the PlanResult's counts, the epoch's targets; with seed_epochs also
    # "clear_min", float32 [N]: the least texel value over each robot's seed points; with separation also "held_back" (int [N]: walked - k),
    # "sweeps" and "stalled" (every k is 0 and some robot is off its goal: every later epoch would repeat this one); with step_aside also
    # "aside" (int32 [N, 2]: role bits, l), "moved_aside", "released" (int: how many robots) and "cycling" (these start cells occurred before)
    epochs: list


class WorldFleet:
    """N robots from global starts to global goals [N, 2] anywhere on the world map `name` (environments.register_world_map), planned
    together epoch by epoch; one process (rank 0 of 1).  The constructor builds, once, the distance field of every distinct goal cell
    over the whole world grid on the resident world texture (device_distance_field, region None): 4 * nx * ny bytes per distinct goal,
    16.8 MB on a 2048-side world.  ValueError names the robot whose start or goal lies outside the world or on a cell that is not
    routable at `clearance`, or whose goal cannot be reached from its start.

    reach, max_steps: window_goal's, in cells; reach <= 199 on the model's 400-cell window.  Further keyword arguments go to every
    epoch's WorldRobotSampler (n_samples, constraint_table, ...).  `positions` (float32 [N, 2], global) are the robots' current points.

    seed_epochs=True: an epoch starts from its walk instead of from noise.  epoch_targets then runs mmd_grid_window_goal_samples in
    place of mmd_grid_window_goals (the same three outputs, and the walks' 64 support cells, which stay on the device); step builds every
    robot's seed trajectory in one mmd_window_seeds launch on the resident world texture -- from the robot's position to its sub-goal
    point, smooth_iters iterations, at the fleet's clearance, inside the robot's window -- and calls the sampler's
    plan_rounds_seeded(trajs_from_global(seeds), paths_local=the seeds' positions, local_rounds=True, n_noising_steps,
    n_denoising_steps): round 0's constraint table is built on the seed paths, not on straight lines through walls, and every round of
    the epoch is a local re-plan.  Such a round runs n_denoising_steps + n_diffusion_steps_without_noise UNet forwards (3 + 1 = 4 with
    the defaults: run_local_inference's q_sample is one launch without a forward, then conditional_sample's loop) where a round from
    noise runs T + 1 (26 at the released T = 25).  An arrived robot has steps = 0: all 64 samples are its goal cell, so its seed
    runs from its goal point to its goal point inside that one cell (the cell's centre in between, drawn towards the goal point by the
    smoothing) with velocities of at most half a cell over 2 dt; that is "held still" as far as a seed goes, and the robot is still
    sampled between its two pinned ends.  With seed_epochs=False (the default) nothing of this runs.

    separation=None (the default): every robot's sub-goal is its walk's end, whatever the others do.  An int >= 1
    (SUBGOAL_SEPARATION = 23 keeps the pinned ends RR_MARGIN apart) keeps every epoch's sub-goals that many cells apart (the module's
    docstring, SEPARATION): the constructor refuses, naming both robots, two start cells or two goal cells closer than that, and
    max_steps above 4095; epoch_targets runs
    device_subgoals_apart (mmd_grid_window_goals_apart: a restart call of 4 sweeps and, while robots still moved, 4 more) in place of
    mmd_grid_window_goals, with seed_epochs with the samples of the shortened walks, so that mmd_window_seeds, unchanged, builds the seeds
    on them; EpochTargets gains `extra` (walked, clear) and `sweeps`, every epoch's dict "held_back" (walked - k per robot), "sweeps" and
    "stalled"; run(max_epochs=None) loops until every robot has arrived or an epoch is stalled (no robot moves, every k is 0: the
    state would repeat for good), which terminates although epoch_bound no longer holds; an explicit max_epochs still caps it.

    step_aside=False (the default): a robot that the separation holds back waits, and a fleet whose robots all wait is stalled.  True
    (needs separation=; refused with seed_epochs=True): a standing robot steps aside for the robots it holds back, into a cell of its
    box of radius aside_reach (at most min(reach, 63)) at most aside_steps (at most 4095) steps away, and the robots it held walk in the
    same epoch (the module's docstring, STEPPING ASIDE: every epoch's pinned ends stay `separation` apart, and a side cell lies in the
    robot's window).  epoch_targets runs device_subgoals_aside's launches in place of device_subgoals_apart's
    (mmd_grid_window_goals_apart to its fixed point, then mmd_grid_window_goals_aside on its workspace: a restart call of 4 sweeps and,
    while the state still moved, 4 more); EpochTargets gains `aside` (role bits, l), every epoch's dict "aside", "moved_aside" and
    "released" (how many robots) and "cycling" (the tuple of the robots' start cells occurred earlier in the run: epoch_targets is a
    function of the cells alone, so the run would repeat for good; run() returns after that epoch).  "stalled" keeps its expression: a
    robot that moved aside has summary[:, 0] = l >= 1, so an epoch with a side step is not stalled; "held_back" keeps its expression too
    and means nothing for a robot that moved aside.  run(max_epochs=None) is refused: no bound on the epochs is proven, so the caller
    states the cap.  persistent=True works as ever, bit for bit: the launch's first 8 N words keep their layout.

    persistent=False (the default): every epoch builds a WorldRobotSampler, a guide and a named window set of its own and releases the
    set afterwards.  persistent=True keeps ONE sampler (own_windows=True), one guide and
    one window set [N, 1, 400, 400, 4] (slice r is robot r's) for the whole run and moves them between epochs on the device
    (_moved_sampler): every result -- paths, conflict counts, summaries, offsets, clear_min -- is the default's bit for bit, with
    seed_epochs and separation as well; only the time and the memory traffic differ.  close() releases the set, and run()
    closes when it returns; a neighbor_slots= smaller than some epoch needs is refused by the sampler's own message, in that epoch.

    The three options share one epoch_targets, one step and one run; each is a branch where its launch, its sampler or its stop rule
    differs.  EpochTargets.words is the sub-goal launch's device words [8 N] under every option (they were None without seed_epochs
    while only the seeded epoch read them; the persistent step reads them as well).

    report(result_or_paths) judges a run afterwards (RunReport; the module's docstring): obstacles at the waypoints and at sampled points
    inside the segments, robot against robot at every column of the whole run, arrival.  Opt-in: nothing above calls it.

    Out of scope here:
      - an arrived robot is sampled like any other, between two ends pinned to its goal point, not held still;
      - the fleet is not sharded over ranks;
      - repair= and replan=, which WorldRobotSampler refuses;
      - with separation= alone a stalled fleet is reported, not resolved; with step_aside=True no liveness is proven (a fleet may still
        stall or cycle), a cycling fleet is reported and not broken (the priorities are the robots' indices and never rotate), and
        seeded epochs are not built (a side step has no support cells); without separation two sub-goals may coincide.
    Whether a seeded epoch resolves conflicts as well as one from noise is not known."""

    def __init__(self, model, name, starts, goals, clearance=OBSTACLE_MARGIN, reach=180, max_steps=360, device="cuda", seed_epochs=False,
                 smooth_iters=64, n_noising_steps=3, n_denoising_steps=3, separation=None, persistent=False, step_aside=False,
                 aside_reach=48, aside_steps=96, **world_robot_sampler_kwargs):
        self.model, self.name, self.device = model, name, environments.resolved_device(device)
        self.persistent, self.step_aside = bool(persistent), bool(step_aside)
        if self.step_aside and separation is None:
            raise ValueError("WorldFleet: step_aside=True needs separation= (robots step aside for robots that the separation holds back)")
        if self.step_aside and seed_epochs:
            raise ValueError("WorldFleet: step_aside=True with seed_epochs=True is not built: a side step has no support cells yet")
        self._sampler = self._points_dev = self._points_host = self._goal_points_dev = self._line_a = self._report_goals_dev = None
        self.separation = None if separation is None else _checked_sep("WorldFleet: separation", separation)
        self.clearance = float(clearance)
        self.seed_epochs = bool(seed_epochs)
        self.smooth_iters, self.n_noising_steps, self.n_denoising_steps = int(smooth_iters), int(n_noising_steps), int(n_denoising_steps)
        if self.smooth_iters < 0 or self.n_noising_steps < 0 or self.n_denoising_steps < 1:
            raise ValueError(f"WorldFleet: smooth_iters = {smooth_iters} (>= 0), n_noising_steps = {n_noising_steps} (>= 0), "
                             f"n_denoising_steps = {n_denoising_steps} (>= 1)")
        self.sampler_kwargs = dict(world_robot_sampler_kwargs)
        for refused in ("rank", "world_size", "group", "env_id"):
            if refused in self.sampler_kwargs:
                raise ValueError(f"WorldFleet: {refused}= is not taken: a fleet runs in one process on the world map it was given")
        self.shape = tuple(environments.world_map_occupancy(name).shape)
        self.window = int(environments.grid_shape()[0])
        self.reach, self.max_steps, _ = _checked_walk_args("WorldFleet", self.shape, reach, max_steps, self.window)
        self.aside_reach, self.aside_steps = (_checked_aside("WorldFleet", self.reach, aside_reach, aside_steps) if self.step_aside
                                              else (aside_reach, aside_steps))
        self.limits = environments.world_map_limits(name)
        s_pts, self.goal_points = _points(starts), _points(goals)
        n = s_pts.shape[0]
        if n == 0 or self.goal_points.shape[0] != n:
            raise ValueError(f"WorldFleet: {n} starts and {self.goal_points.shape[0]} goals (equal and at least 1)")
        s_cells, g_cells = (self._cells(pts, what) for pts, what in ((s_pts, "start"), (self.goal_points, "goal")))
        if self.separation is not None:
            if self.max_steps > _lib.WINDOW_APART_MAX_STEPS:
                raise ValueError(f"WorldFleet: max_steps = {self.max_steps} with separation= (at most {_lib.WINDOW_APART_MAX_STEPS})")
            for what, cells in (("start", s_cells), ("goal", g_cells)):
                d = cells.astype(np.int64)[:, None, :] - cells.astype(np.int64)[None, :, :]
                close = np.argwhere(np.triu((d * d).sum(-1) < self.separation ** 2, 1))
                if close.size:
                    a, b = (int(v) for v in close[0])
                    raise ValueError(f"WorldFleet: the {what} cells of robots {a} and {b} on {name!r}, {cells[a].tolist()} and "
                                     f"{cells[b].tolist()}, are closer than separation = {self.separation} cells")
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
        self.last_clear_min = None

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
        """EpochTargets of the robots at the global points `positions` [N, 2]: one sub-goal launch -- mmd_grid_window_goals; with
        seed_epochs mmd_grid_window_goal_samples, the same words and the samples, which stay on the device; with separation
        device_subgoals_apart's launches (with seed_epochs: with the samples of the shortened walks), whose summary is
        (k, d0 - k, status, arrived) -- and one device -> host copy (with separation: one per call of the entry point).  A robot's cell
        is world_cells' texel of its point; its sub-goal point is the centre of the sub-goal cell by cell_centres' fp32 sequence, or,
        once the sub-goal cell is the goal's (`arrived`), the caller's exact goal point.  Refuses a robot whose status is not ROUTE_OK."""
        pts = _points(positions)
        if pts.shape[0] != self.n_robots:
            raise ValueError(f"WorldFleet.epoch_targets: {pts.shape[0]} positions for {self.n_robots} robots")
        c0 = self._cells(pts, "position")
        walk = (self.dist, c0, self._fields_dev, self._goals_dev, self.reach, self.max_steps)
        if self.separation is None:
            (words, samples), sweeps = _window_goals_words(*walk, self.window, self.seed_epochs), None
            host = words.cpu().numpy()
        elif self.step_aside:
            words, host, sweeps, _ = _subgoals_aside_words(*walk, self.separation, self.aside_reach, self.aside_steps, self.window, 4, "WorldFleet")
            samples = None
        else:
            words, host, samples, sweeps = _subgoals_apart_words(*walk, self.separation, self.window, 4, self.seed_epochs, "WorldFleet")
        cells, origins, summary, *extra = (a.copy() for a in _split_words(host, apart=self.separation is not None, aside=self.step_aside))
        bad = np.flatnonzero(summary[:, 2] != ROUTE_OK)
        if bad.size:
            r = int(bad[0])
            raise RuntimeError(f"WorldFleet: robot {r} on {self.name!r} at cell {c0[r].tolist()}: sub-goal status "
                               f"{_STATUS_NAMES.get(int(summary[r, 2]), int(summary[r, 2]))}")
        points = np.ascontiguousarray(cell_centres(cells, self.limits[0], self.limits[1], self.shape), dtype=np.float32)
        arrived = summary[:, 3] == 1
        points[arrived] = self.goal_points[arrived]
        return EpochTargets(cells, origins, environments.world_map_window_offsets(self.name, origins), points, summary, samples,
                            words[:8 * self.n_robots], extra[0] if extra else None, sweeps, extra[1] if self.step_aside else None)

    def _moved_sampler(self, targets):
        """persistent=True: (the fleet's one sampler, moved to the epoch's targets; the robots' points and their sub-goal points [N, 2]
        on the device; the straight lines between them [N, 64, 2]).  One mmd_fleet_epoch_frames launch on the launch's words, the
        robots' points and their goal points, all on the device, and the sampler moved to what it wrote
        (WorldRobotSampler._move_on_device: one mmd_sdf_grid_windows_moved launch, which cuts only the slices whose origin changed).
        The first epoch builds the sampler with own_windows=True first; its windows then do not move.  No sampler, guide or facade is
        built, no texture allocated, no window named, no hard condition, offset or line uploaded.  The robots' points of the next
        epoch are the device slice paths_local[:, -1]; the host copy feeds world_cells and its refusals, as ever."""
        if self._goal_points_dev is None:
            self._goal_points_dev = torch.from_numpy(self.goal_points).to(self.device)
            self._line_a = torch.from_numpy(np.linspace(0.0, 1.0, SEED_POINTS, dtype=np.float32)).to(self.device)
        if self._points_host is not self.positions:          # the first epoch, or positions set by the caller: the only upload of points
            self._points_dev = torch.from_numpy(np.ascontiguousarray(self.positions, dtype=np.float32).reshape(-1, 2)).to(self.device)
        if self._sampler is None:
            self._sampler = WorldRobotSampler(self.model, self.positions, targets.points, targets.offsets, env_id=self.name,
                                              device=self.device, own_windows=True, **self.sampler_kwargs)
        kw = {k: self.sampler_kwargs[k] for k in ("norm_mins", "norm_maxs") if k in self.sampler_kwargs}
        offsets_dev, points_dev, hard_first, hard_last, lines = device_epoch_frames(self.name, targets.words, self._points_dev,
                                                                                   self._goal_points_dev, line_a=self._line_a, **kw)
        self._sampler._move_on_device((self.positions, targets.points), targets.offsets, targets.origins, offsets_dev, hard_first, hard_last,
                                      _split_words(targets.words)[1])
        return self._sampler, self._points_dev, points_dev, lines

    def step(self, seed, max_rounds=8):
        """One epoch: the targets of the current positions; the epoch's sampler from the positions to the sub-goal points -- a fresh
        WorldRobotSampler on named windows, whose map set is released afterwards (map_textures.release_sdf_textures), or, with
        persistent=True, the fleet's one sampler moved in place (_moved_sampler; nothing is released), the same epoch bit for bit --;
        its plan -- plan(max_rounds, seed) on the fresh sampler, plan_rounds from the straight lines the frames launch wrote on the moved
        one, and with seed_epochs plan_rounds_seeded from the epoch's seeds on either (the class's docstring); the seeds' ends are the
        points as they come: host arrays, which device_window_seeds uploads, or the moved sampler's device tensors --; and the robots
        moved to the last points of the returned paths, as they are.  -> (PlanResult, EpochTargets); with seed_epochs `last_clear_min`
        (float32 [N]) holds the seeds' least texel values, from the copy that brings the new positions back."""
        targets = self.epoch_targets(self.positions)
        if self.persistent:
            sampler, starts, goals, lines = self._moved_sampler(targets)
        else:
            starts, goals = self.positions, targets.points
            sampler = WorldRobotSampler(self.model, starts, goals, targets.offsets, env_id=self.name, device=self.device, **self.sampler_kwargs)
        try:
            if self.seed_epochs:
                _, origins_dev, summary_dev = _split_words(targets.words)
                seeds, clear_min = device_window_seeds(map_textures.device_world_texture(self.name, self.device), self.limits[0], self.limits[1],
                                                       targets.samples, origins_dev, summary_dev, self.window, starts, goals, self.clearance,
                                                       self.smooth_iters)
                res = sampler.plan_rounds_seeded(sampler.trajs_from_global(seeds), paths_local=seeds[..., :2].contiguous(),
                                                 local_rounds=True, n_noising_steps=self.n_noising_steps,
                                                 n_denoising_steps=self.n_denoising_steps, max_rounds=max_rounds, seed=seed)
            elif self.persistent:
                res = sampler.plan_rounds(paths_local=lines, max_rounds=max_rounds, seed=seed)
            else:
                res = sampler.plan(max_rounds=max_rounds, seed=seed)
        finally:
            if not self.persistent:
                map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), self.device)
        ends = res.paths_local[:, -1, :]
        if self.seed_epochs:
            back = torch.cat([ends, clear_min[:, None]], dim=1).cpu().numpy()            # one copy: the ends and clear_min
            self.positions, self.last_clear_min = np.ascontiguousarray(back[:, :2], dtype=np.float32), back[:, 2].copy()
        else:
            self.positions = np.ascontiguousarray(ends.cpu().numpy(), dtype=np.float32)
        if self.persistent:
            self._points_dev, self._points_host = ends, self.positions
        return res, targets

    def report(self, result_or_paths, margin=ROBOT_RADIUS, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
        """RunReport (device_run_report: two kernels, one copy) of a FleetResult's paths, or of any global paths [N, L, 2] of this fleet's
        robots, on the resident world texture (map_textures.device_world_texture), over the fleet's limits and against its exact goal
        points.  Reads nothing of the sampler: it works after run() has closed it, and changes nothing in the fleet.  margin: the
        least value a point may read without being hit, by default the robot's radius (a value is the distance to the nearest occupied
        cell's edge); goal_tol=None: the world's cell pitch."""
        paths = result_or_paths.paths if isinstance(result_or_paths, FleetResult) else result_or_paths
        paths = torch.as_tensor(paths, dtype=torch.float32).to(self.device).contiguous()
        if paths.dim() != 3 or paths.shape[0] != self.n_robots:
            raise ValueError(f"WorldFleet.report: paths [{self.n_robots}, L, 2], got {tuple(paths.shape)}")
        if self._report_goals_dev is None:
            self._report_goals_dev = torch.from_numpy(self.goal_points).to(self.device)
        return device_run_report(paths, map_textures.device_world_texture(self.name, self.device), self.limits[0], self.limits[1],
                                 self._report_goals_dev, margin, rr_margin, n_interp, goal_tol, column_conflicts)

    def close(self):
        """persistent=True: release the sampler's window set (update_world_map no longer reaches it) and drop the sampler; the next
        step builds another.  Nothing otherwise.  run() closes when it returns, also on an exception."""
        sampler, self._sampler = self._sampler, None
        self._points_dev = self._points_host = None
        if sampler is not None:
            sampler.release_windows()

    def run(self, max_epochs=None, max_rounds=8, seed=0):
        """Epochs (epoch e with seed + e) until every robot has arrived, at most max_epochs of them (None: epoch_bound(), which suffices
        from the starts).  A robot that has arrived keeps taking part, from its goal point to its goal point, so that the others stay
        constrained by it.  With separation: until every robot has arrived or an epoch is stalled (the module's docstring: one of the two
        comes), at most max_epochs of them if that is given.  -> FleetResult"""
        apart = self.separation is not None
        if max_epochs is None:
            if self.step_aside:
                raise ValueError("WorldFleet.run: step_aside=True needs max_epochs (no bound on the epochs is proven: the caller states the cap)")
            max_epochs = None if apart else self.epoch_bound()
        elif int(max_epochs) < 1:
            raise ValueError(f"WorldFleet.run: max_epochs = {max_epochs} (at least 1)")
        paths, epochs, seen = [], [], set()
        try:
            while True:
                if self.step_aside:                          # the targets are a function of the robots' cells alone: a repeat repeats for good
                    at = world_cells(self.name, self.positions).tobytes()
                    cycling, _ = at in seen, seen.add(at)
                res, targets = self.step(seed + len(epochs), max_rounds)
                arrived = targets.summary[:, 3] == 1         # the epoch's sub-goal was the goal point: the robot now stands on it
                paths.append(res.paths_local)
                epochs.append({"conflict_counts": list(res.conflict_counts), "summary": targets.summary, "offsets": targets.offsets})
                stalled = bool(apart and (targets.summary[:, 0] == 0).all() and not arrived.all())  # no robot moves, one that arrives now included
                if apart:
                    epochs[-1].update(held_back=targets.extra[:, 0] - targets.summary[:, 0], sweeps=targets.sweeps, stalled=stalled)
                if self.step_aside:
                    epochs[-1].update(aside=targets.aside, moved_aside=int(((targets.aside[:, 0] & ASIDE_MOVED) != 0).sum()),
                                      released=int(((targets.aside[:, 0] & ASIDE_RELEASED) != 0).sum()), cycling=cycling)
                if self.seed_epochs:
                    epochs[-1]["clear_min"] = self.last_clear_min
                if arrived.all() or stalled or (self.step_aside and cycling) or (max_epochs is not None and len(epochs) >= int(max_epochs)):
                    return FleetResult(torch.cat(paths, dim=1), arrived, epochs)
        finally:
            self.close()
