"""What the world-fleet tests share: small written-out grids and their fields, and the loop that iterates the definition
(mmd_amd.world_fleet.window_goal) from the cell each call reached until the robot stands on its goal."""
import numpy as np

from mmd_amd import world_fleet as F
from mmd_amd.world_routes import ROUTE_OK, UNREACHED, grid_distance_field

SMALL = (40, 30)                 # the host tests' grids, with reach 5 and window 12
REACH, WINDOW = 5, 12


def open_grid(shape=SMALL):
    return np.ones(shape, bool)


def door_grid(shape=SMALL, wall=20, door=(22, 24)):
    """A wall along the column ix = wall with one door, the cells iy in door[0] .. door[1] - 1"""
    routable = np.ones(shape, bool)
    routable[wall, :] = False
    routable[wall, door[0]:door[1]] = True
    return routable


def serpentine_grid(shape=SMALL, pitch=8, gap=3):
    """Walls along the columns ix = pitch, 2 pitch, ..., open for `gap` cells at the top and at the bottom in turn: one long corridor"""
    routable = np.ones(shape, bool)
    for k, ix in enumerate(range(pitch, shape[0] - 1, pitch)):
        routable[ix, :] = False
        if k % 2 == 0:
            routable[ix, shape[1] - gap:] = True
        else:
            routable[ix, :gap] = True
    return routable


def fields(routable, goals):
    """int32 [n_fields, nx, ny], read-only: the converged fields of the goal cells"""
    dist = grid_distance_field(routable, np.asarray(goals).reshape(-1, 2))
    dist.setflags(write=False)
    return dist


def iterate(dist, start, goal, reach, max_steps, window, limit=10000):
    """[(c0, cell, origin, steps, remaining)] of window_goal called from `start`, then from the cell each call reached, until remaining is
    0: every call must be ROUTE_OK"""
    calls, c0 = [], (int(start[0]), int(start[1]))
    while True:
        cell, origin, steps, remaining, status = F.window_goal(dist, c0, goal, reach, max_steps, window)
        assert status == ROUTE_OK, (c0, status)
        calls.append((c0, cell, origin, steps, remaining))
        if remaining == 0:
            return calls
        assert len(calls) < limit, "the walk does not arrive"
        c0 = cell


def unconverged_field(shape=SMALL):
    """(dist [1, nx, ny], goal, where the walk sticks): the open field of the goal (3, 3) with the two downhill neighbours of the cell
    (10, 10), which holds 14, raised to 20: a walk that stands on (10, 10) finds no neighbour that holds 13.  From (10, 12) the walk takes
    (10, 11) and (10, 10) and sticks after 2 steps."""
    goal = (3, 3)
    dist = grid_distance_field(open_grid(shape), [goal]).copy()
    assert dist[0, 10, 10] == 14 and UNREACHED > 20
    dist[0, 9, 10] = dist[0, 10, 9] = 20
    return dist, goal, (10, 10)
