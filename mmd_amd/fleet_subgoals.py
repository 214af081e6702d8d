"""The numpy function window_goal IS the definition of the sub-goal and the window; the kernel (csrc/window_goals.hip) computes the same
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
"""
import numpy as np

from . import _lib
from .world import OBSTACLE_MARGIN
from .world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, SEED_POINTS, UNREACHED, sample_offsets, seed_trajectory


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


def _taking_walks(dist, starts, fields, goals, reach, max_steps, window):
    """(window_goals' three arrays, the cell paths, the queries that take part): the walks of every sub-goal rule, under window_goals' name"""
    plain, paths = _walks("window_goals", dist, starts, fields, goals, reach, max_steps, window)
    return plain, paths, [q for q, p in enumerate(paths) if p is not None]


def _apart_in_order(paths, taking, sep):
    """(ks, clear) per taking-part query: subgoals_apart's choice, the robots taken in index order, each against _blockers of the choices so far"""
    ks, clear = {}, {}
    for r in taking:
        ks[r], clear[r] = _apart_choice(paths[r], _blockers(paths, taking, ks, r), sep)
    return ks, clear


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
    plain, paths, taking = _taking_walks(dist, starts, fields, goals, reach, max_steps, window)
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
    plain, paths, taking = _taking_walks(dist, starts, fields, goals, reach, max_steps, window)
    ks, clear = _apart_in_order(paths, taking, sep)
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
    plain, paths, taking = _taking_walks(dist, starts, fields, goals, reach, max_steps, window)
    aside_reach, aside_steps = _checked_aside("subgoals_aside", reach, aside_reach, aside_steps)
    dist, fields = np.asarray(dist), np.asarray(fields, np.int64).reshape(-1)
    ks, clear = _apart_in_order(paths, taking, sep)          # phase 1: subgoals_apart
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
