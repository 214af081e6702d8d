"""What the step-aside tests share (mmd_amd.world_fleet.subgoals_aside): the host run loop of the definition with its four ends, the
written-out cases, and the larger batches that the device tests add.  A case is (dist, starts, which, goals, args) with
args = (reach, max_steps, sep, aside_reach, aside_steps, window), subgoals_aside's arguments behind the goals."""
import numpy as np

import world_fleet_apart_model as A
import world_fleet_model as M
from mmd_amd import world_fleet as F
from mmd_amd.fleet_subgoals import _walk, _walks
from mmd_amd.world_routes import ROUTE_OK

SEP = A.SEP
ASIDE_REACH, ASIDE_STEPS = 5, 10
ARGS = (M.REACH, 100, SEP, ASIDE_REACH, ASIDE_STEPS, M.WINDOW)
HELD, YIELDS, MOVED, RELEASED = F.ASIDE_HELD, F.ASIDE_YIELDS, F.ASIDE_MOVED, F.ASIDE_RELEASED


def case(goals, starts, which=None, dist=None, routable=None, **kw):
    """a case on the open grid of 40 x 30 cells (or on `routable`, or on the fields `dist`), robot r bound for goals[r] unless `which` says
    otherwise; kw replaces entries of ARGS by name"""
    names = ("reach", "max_steps", "sep", "aside_reach", "aside_steps", "window")
    args = tuple(kw.get(name, value) for name, value in zip(names, ARGS))
    dist = M.fields(M.open_grid() if routable is None else routable, goals) if dist is None else dist
    which = np.arange(len(starts), dtype=np.int32) if which is None else np.asarray(which, np.int32)
    return dist, np.asarray(starts, np.int32), which, np.asarray(goals, np.int32), args


def aside(c):
    dist, starts, which, goals, args = c
    return F.subgoals_aside(dist, starts, which, goals, *args)


def conflict(a, b, sep=SEP):
    return (int(a[0]) - int(b[0])) ** 2 + (int(a[1]) - int(b[1])) ** 2 < sep * sep


def roles_by_hand(dist, starts, which, goals, args):
    """(held, clears) from subgoals_apart's words and the plain walks alone: the roles as the issue states them, not as the code computes
    them"""
    reach, max_steps, sep, _, _, window = args
    k, walked = F.subgoals_apart(dist, starts, which, goals, reach, max_steps, sep, window)[2:4]
    _, paths = _walks("window_goals", dist, starts, which, goals, reach, max_steps, window)
    n = len(starts)
    stands = [paths[q] is not None and k[q, 0] == 0 for q in range(n)]
    held = [stands[q] and walked[q, 0] >= 1 for q in range(n)]
    clears = [[r for r in range(n) if held[r] and r != j and stands[j] and conflict(starts[j], paths[r][1], sep) and (not held[j] or r < j)]
              for j in range(n)]
    return held, clears, paths


# ---- the written-out cases (tests/test_world_fleet_aside_host.py pins their words) -----------------------------------------------------------
def two_robots():
    """robot 0 stands on its goal (17, 15), in the way of robot 1 from (20, 13) to (1, 18)"""
    return case([(17, 15), (1, 18)], [(17, 15), (20, 13)])


TWO_ROBOT_CELLS = [[(17, 16), (15, 13)], [(17, 16), (10, 13)], [(17, 15), (5, 14)], [(17, 15), (1, 18)]]


def head_on(goal1=(0, 15), **kw):
    """two robots 3 cells apart in row 15 that walk towards one another: each is held by the other, robot 1 yields to robot 0"""
    return case([(30, 15), goal1], [(10, 15), (13, 15)], **kw)


def head_on_columns():
    """head_on turned by a quarter: the two side cells of robot 1 differ in ix alone"""
    return case([(20, 29), (20, 0)], [(20, 10), (20, 13)])


def boxed_in():
    """robot 0 stands on its goal in the way of robot 1; the cells of its box of radius 3 that robot 1's walk leaves free (class d) conflict
    with the six robots that stand on their goals above and below (class a)"""
    goals = [(17, 15), (1, 15), (14, 20), (17, 20), (20, 20), (14, 10), (17, 10), (20, 10)]
    return case(goals, [(17, 15), (20, 15)] + goals[2:], aside_reach=3)


def at_the_border(blocked):
    """head_on in row 1 with a box of radius 3 and 3 steps: of the two cells 3 steps off the row, (13, -2) is no cell of the grid; with
    `blocked` a robot stands on its goal (13, 6), in conflict with the other, (13, 4)"""
    extra = [(13, 6)] if blocked else []
    return case([(30, 1), (0, 1)] + extra, [(10, 1), (13, 1)] + extra, aside_reach=3, aside_steps=3)


def moved_not_released():
    """robot 1 is held and yields to robot 0; robot 2, which robot 1's first step conflicts with, is held too and yields to robot 1: both
    move aside, robot 1 is in clears(2), and a robot that moved aside is not released"""
    return case([(34, 28), (17, 11), (5, 22), (20, 29), (16, 4)], [(8, 16), (11, 16), (14, 15), (17, 12), (15, 9)])


def every_status():
    """two_robots among queries of every other status (test_world_fleet_apart_host.py's batch, moved to these fields)"""
    stuck, goal0, _ = M.unconverged_field()
    walled = M.fields(M.door_grid(door=(0, 0)), [(25, 5)])
    dist = np.concatenate([stuck, M.fields(M.open_grid(), [(17, 15), (1, 18)]), walled])
    goals = [goal0, (17, 15), (1, 18), (25, 5)]
    starts = [(17, 15), (-1, 3), (20, 13), (15, 15), (10, 12), (16, 15)]
    return case(goals, starts, which=[1, 1, 2, 3, 0, 7], dist=dist)


HOST_CASES = {
    "two robots": two_robots, "head on": head_on, "head on, goal above": lambda: head_on((0, 20)), "head on, columns": head_on_columns,
    "too few steps": lambda: head_on(aside_steps=2), "boxed in": boxed_in, "border, free": lambda: at_the_border(False),
    "border, blocked": lambda: at_the_border(True), "moved, not released": moved_not_released, "every status": every_status,
}


# ---- whole runs ---------------------------------------------------------------------------------------------------------------------------------
def run_aside(dist, starts, which, goals, args=ARGS, cap=300, step_aside=True):
    """(end, [(starts, out)]): whole epochs of the definition, each from the cells the one before chose; out is subgoals_aside's five arrays
    (step_aside=False: subgoals_apart's four).  end: "arrived"; "stalled" (no robot moves and one is off its goal); "cycling" (the
    epoch's start cells occurred before: the run would repeat for good; the epoch is listed); "cap" (`cap` epochs ran)"""
    reach, max_steps, sep, aside_reach, aside_steps, window = args
    epochs, at, seen = [], np.asarray(starts, np.int32), set()
    while True:
        if step_aside:
            out = F.subgoals_aside(dist, at, which, goals, reach, max_steps, sep, aside_reach, aside_steps, window)
        else:
            out = F.subgoals_apart(dist, at, which, goals, reach, max_steps, sep, window)
        assert (out[2][:, 2] == ROUTE_OK).all()
        epochs.append((at, out))
        cycling, _ = at.tobytes() in seen, seen.add(at.tobytes())
        if (out[2][:, 3] == 1).all():
            return "arrived", epochs
        if A.stalled(out[2]):
            return "stalled", epochs
        if cycling:
            return "cycling", epochs
        if len(epochs) >= cap:
            return "cap", epochs
        at = out[0].copy()


def real_scale(seed, n=32, side=400, sep=23):
    """(dist, starts, which, goals) of n robots on an open grid of side x side cells, starts and goals drawn pairwise sep apart"""
    routable = np.ones((side, side), bool)
    rng = np.random.Generator(np.random.PCG64(seed))
    goals = A.draw_apart(rng, routable, n, sep)
    starts = A.draw_apart(rng, routable, n, sep)
    return M.fields(routable, goals), np.asarray(starts, np.int32), np.arange(n, dtype=np.int32), np.asarray(goals, np.int32)


REAL_ARGS = (180, 360, 23, 48, 96, 400)
REAL_SEED, REAL_STRANDED = 1, 3  # of the seeds 0 .. 5 the one whose run stalls under the separation alone, with 3 robots off their goals


# ---- the device tests' larger batches -----------------------------------------------------------------------------------------------------------
def crowd(n, seed):
    """n robots on distinct cells of the 40 x 30 grid with the door, drawn with no regard to one another and bound for six goals: most
    stand, many are held, many yield -- more robots than a chunk of blockers has"""
    routable = M.door_grid()
    goals = [(2, 2), (37, 27), (2, 27), (37, 2), (25, 15), (12, 15)]
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.argwhere(routable)
    starts = free[rng.choice(len(free), n, replace=False)].astype(np.int32)
    return case(goals, starts, which=rng.integers(0, len(goals), n), routable=routable)


def big_crowd(n, seed, shape=(90, 60)):
    """crowd on a grid of 90 x 60 cells with a door, for more robots than the side kernel's chunk of 256 blockers has"""
    routable = M.door_grid(shape, wall=45, door=(20, 40))
    goals = [(2, 2), (87, 57), (2, 57), (87, 2), (60, 30), (30, 30)]
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.argwhere(routable)
    starts = free[rng.choice(len(free), n, replace=False)].astype(np.int32)
    return case(goals, starts, which=rng.integers(0, len(goals), n), routable=routable)


def long_walk(shape, reach, aside_reach, window, pitch=6, height=31):
    """Robot 0 walks a serpentine of corridors `height` cells long in the grid's lower rows (a wall closes them off from the rest, which is
    open), and on every third cell of its walk a robot stands on its goal (they share one hand-built field of zeros): robot 0 is held at
    its start by a walk of hundreds of cells that winds inside the side box of the robot that stands 3 cells ahead, which yields.
    -> (case, the length of robot 0's walk)"""
    routable = np.ones(shape, bool)
    routable[:, :height] = M.serpentine_grid((shape[0], height), pitch=pitch, gap=3)
    routable[:shape[0] - 3, height] = False
    start, goal = (3, 3), (shape[0] - 3, 3)
    real = M.fields(routable, [goal])
    path, status = _walk(real[0], start, goal, int(real[0][start]), reach, 4000)
    assert status == ROUTE_OK
    dist = np.concatenate([real, np.zeros((1,) + tuple(shape), np.int32)])
    starts = [start] + path[3::3]
    return case([goal, (0, 0)], starts, which=[0] + [1] * (len(starts) - 1), dist=dist, reach=reach, max_steps=len(path) - 1,
                aside_reach=aside_reach, aside_steps=4 * aside_reach, window=window), len(path) - 1
