"""What the sub-goal separation tests share (mmd_amd.world_fleet.subgoals_apart): seeded batches of 24 robots on the written-out grids of
world_fleet_model, whole runs of the definition iterated, and the written-out chain."""
import numpy as np

import world_fleet_model as M
from mmd_amd import world_fleet as F
from mmd_amd.world_routes import ROUTE_OK, UNREACHED

SEP, N_ROBOTS = 3, 24
GRIDS = {"open": M.open_grid, "door": M.door_grid, "serpentine": M.serpentine_grid}
# the seeds were chosen so that every batch's FIRST epoch shows the rule at work (test_world_fleet_apart_host.py asserts it): a robot held
# back to a k > 0, a robot at k = 0 that walked, a pair of plain sub-goals closer than SEP, and a choice that needs at least 2 sweeps
SEEDS = {"open": 2, "door": 1, "serpentine": 2}

CHAIN_STARTS = [(28 - 4 * i, 10) for i in range(7)] + [(31, 10)]
CHAIN_GOALS = [(39, 10), (39, 13), (39, 7), (39, 16), (39, 4), (39, 19), (39, 1), (31, 10)]
CHAIN_K = [[0, 4, 5, 5, 5, 5, 5, 0], [0, 1, 5, 5, 5, 5, 5, 0], [0, 1, 2, 5, 5, 5, 5, 0], [0, 1, 2, 3, 5, 5, 5, 0], [0, 1, 2, 3, 4, 5, 5, 0],
           [0, 1, 2, 3, 4, 5, 5, 0]]
CHAIN_CHANGED = [2, 1, 1, 1, 1, 0]
CHAIN_X = [28, 25, 22, 19, 16, 13, 9, 31]


def apart(cells, sep=SEP):
    """the least squared distance over all pairs of the cells [n, 2] (a large number for fewer than two)"""
    c = np.asarray(cells, np.int64)
    d = ((c[:, None] - c[None]) ** 2).sum(-1)
    d[np.diag_indices(len(c))] = np.iinfo(np.int64).max
    return int(d.min()) if len(c) > 1 else np.iinfo(np.int64).max


def draw_apart(rng, routable, n, sep, also=()):
    """n routable cells, pairwise at least sep apart (and from the cells `also`), by rejection"""
    free, chosen = np.argwhere(routable), [tuple(c) for c in also]
    while len(chosen) < len(also) + n:
        c = tuple(int(v) for v in free[rng.integers(0, len(free))])
        if all((c[0] - o[0]) ** 2 + (c[1] - o[1]) ** 2 >= sep * sep for o in chosen):
            chosen.append(c)
    return chosen[len(also):]


def batch(grid, seed=None):
    """(dist [24, nx, ny] read-only, starts, which = 0 .. 23, goals): 24 robots with starts pairwise >= SEP apart, goals pairwise >= SEP
    apart, every goal reached from its start"""
    routable = GRIDS[grid]()
    rng = np.random.Generator(np.random.PCG64(SEEDS[grid] if seed is None else seed))
    goals = draw_apart(rng, routable, N_ROBOTS, SEP)
    starts = draw_apart(rng, routable, N_ROBOTS, SEP)
    dist = M.fields(routable, goals)
    assert all(dist[r][starts[r]] != UNREACHED for r in range(N_ROBOTS))
    return dist, np.asarray(starts, np.int32), np.arange(N_ROBOTS, dtype=np.int32), np.asarray(goals, np.int32)


def chain():
    dist = M.fields(M.open_grid(), CHAIN_GOALS)
    return dist, np.asarray(CHAIN_STARTS, np.int32), np.arange(8, dtype=np.int32), np.asarray(CHAIN_GOALS, np.int32)


def stalled(summary):
    """WorldFleet's stall rule on an epoch's summary: no robot moves (a robot that walks onto its goal in this epoch does), and some robot
    is off its goal; the next epoch would repeat this one"""
    return bool((summary[:, 0] == 0).all() and not (summary[:, 3] == 1).all())


def run_apart(dist, starts, which, goals, reach=M.REACH, max_steps=100, sep=SEP, window=M.WINDOW, limit=200):
    """[(starts, plain = window_goals' outputs, out = subgoals_apart's outputs)] of whole epochs, each from the cells the one before chose,
    until every robot has arrived or no robot moves (every k is 0: a stalled epoch, the last one listed)"""
    epochs, at = [], np.asarray(starts, np.int32)
    while True:
        plain = F.window_goals(dist, at, which, goals, reach, max_steps, window)
        out = F.subgoals_apart(dist, at, which, goals, reach, max_steps, sep, window)
        assert (out[2][:, 2] == ROUTE_OK).all()
        epochs.append((at, plain, out))
        arrived = out[2][:, 3] == 1
        if arrived.all() or stalled(out[2]):
            return epochs
        assert len(epochs) < limit, "the run neither arrives nor stalls"
        at = out[0].copy()
