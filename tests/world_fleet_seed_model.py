"""What the tests of a world fleet's epoch seeds share: the textures of world_fleet_model's grids, batches of walks with their samples by
the definition (mmd_amd.world_fleet.window_goals_samples), the cell path rebuilt one call of window_goal at a time, and batches of robots
for the seed kernel, good rows and odd ones."""
import functools

import numpy as np

import world_fleet_model as M
from mmd_amd import environments as E, world_fleet as F
from mmd_amd.world_routes import ROUTE_OK, ROUTE_STUCK, _texels, cell_centres

CELL = 0.005
LO = (2.0, 2.0)                  # the textures' lower corner: off the origin, as the fleet test's world
P = 64
DT = 5.0 / 64

GRIDS = {
    # name: (routable, goal cells, window, (reach, max_steps) of the long walks)
    "open": (lambda: M.open_grid(), [(20, 15), (0, 0), (39, 29), (7, 22)], M.WINDOW, (5, 100)),
    "door": (lambda: M.door_grid(), [(25, 5), (5, 25), (20, 22), (39, 0)], M.WINDOW, (5, 100)),
    "serpentine": (lambda: M.serpentine_grid((130, 70), pitch=16, gap=5), [(125, 3), (3, 3), (70, 35)], 64, (31, 1000)),
}


def hi_of(shape):
    return (LO[0] + shape[0] * CELL, LO[1] + shape[1] * CELL)


@functools.lru_cache(maxsize=None)
def grid(name):
    """(routable, fields, goals, window, (reach, max_steps), texture, hi) of a grid, built once; the arrays are read-only"""
    make, goals, window, setting = GRIDS[name]
    routable = make()
    tex = E.occupancy_sdf_texture(~routable, CELL)
    tex.setflags(write=False)
    routable.setflags(write=False)
    return routable, M.fields(routable, goals), goals, window, setting, tex, hi_of(routable.shape)


def path_by_single_steps(dist, start, goal, steps, window):
    """the walk's cells c_0 .. c_steps, one call of window_goal with max_steps = 1 per step (the step rule does not read the start, and
    a reach of 1 lets every single step pass)"""
    path = [(int(start[0]), int(start[1]))]
    for _ in range(steps):
        cell, _, took, _, status = F.window_goal(dist, path[-1], goal, 1, 1, window)
        assert status == ROUTE_OK and took == 1
        path.append(cell)
    return path


def robots(name, n, seed, shift=0.0012):
    """n robots on a grid, each an OK walk of the grid's long setting from a random routable cell in a random field: (samples [n, 64, 2],
    origins [n, 2], summary [n, 4], start points, goal points [n, 2] float32 off the cells' centres by `shift`)"""
    routable, dist, goals, window, (reach, max_steps), tex, hi = grid(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.argwhere(routable)
    starts, which = [], []
    while len(starts) < n:
        c, f = free[rng.integers(0, len(free))], int(rng.integers(0, len(goals)))
        if F.window_goal(dist[f], c, goals[f], reach, max_steps, window)[4] == ROUTE_OK:
            starts.append(c)
            which.append(f)
    cells, origins, summary, samples = F.window_goals_samples(dist, starts, which, goals, reach, max_steps, window)
    assert (summary[:, 2] == ROUTE_OK).all()
    s_pts = (cell_centres(np.asarray(starts), LO, hi, routable.shape) + np.float32(shift)).astype(np.float32)
    g_pts = (cell_centres(cells, LO, hi, routable.shape) - np.float32(shift)).astype(np.float32)
    return samples, origins, summary, s_pts, g_pts


def odd_rows(name):
    """Rows no fleet walk gives, for the same grid: (samples, origins, summary, start points, goal points, what each row is).
      0  a status that is not OK (stuck), over good samples: zero rows, clear_min 0
      1  samples outside the window (the origin moved away from them): no point moves
      2  an origin at the world's far edge, hand-built samples along the edge inside it
      3  a NaN start point: the midpoint next to it is NaN, whose texel has index 0 on that axis, outside the row's window
      4  an origin of the ends of int32 (the window test is taken in 64 bits): no point moves"""
    routable, dist, goals, window, _, tex, hi = grid(name)
    nx, ny = routable.shape
    corners = [(0, 0), (nx - window, 0), (0, ny - window), (nx - window, ny - window)]
    for seed in range(5, 200):                               # a walk that one of the world's corner windows misses altogether
        base = robots(name, 1, seed)
        low, high = base[0][0].min(0), base[0][0].max(0)    # the samples' box holds every midpoint: disjoint from the window on one axis
        away = [o for o in corners if ((high < np.asarray(o)) | (low >= np.asarray(o) + window)).any()]
        if away:
            break
    assert away, "no walk lies outside a corner window"
    samples = np.repeat(base[0], 5, axis=0)
    origins = np.repeat(base[1], 5, axis=0)
    summary = np.repeat(base[2], 5, axis=0)
    s_pts, g_pts = np.repeat(base[3], 5, axis=0), np.repeat(base[4], 5, axis=0)
    summary[0, 2] = ROUTE_STUCK
    origins[1] = away[0]
    origins[2] = (nx - window, ny - window)
    edge = np.stack([np.full(P, nx - 1), np.clip(ny - window + np.arange(P) * (window - 1) // (P - 1), 0, ny - 1)], 1)
    samples[2] = edge
    s_pts[2] = cell_centres(edge[0], LO, hi, (nx, ny)) + np.float32(0.001)
    g_pts[2] = cell_centres(edge[-1], LO, hi, (nx, ny)) - np.float32(0.001)
    s_pts[3, 0] = np.nan
    origins[3, 0] = max(origins[3, 0], 1)                    # (cell (0, iy) outside the window: the NaN midpoint is rejected whatever its texel holds)
    origins[4] = (np.iinfo(np.int32).max - 3, np.iinfo(np.int32).min)
    return samples, origins, summary, s_pts, g_pts, ("not OK", "outside the window", "the world's edge", "a NaN start", "an int32 origin")


def definition_seeds(name, samples, origins, summary, s_pts, g_pts, clearance, smooth_iters):
    """(seeds [n, 64, 4], clear_min [n]) by window_seed, zero for a status that is not OK"""
    _, _, _, window, _, tex, hi = grid(name)
    n = len(samples)
    seeds, clear_min = np.zeros((n, P, 4), np.float32), np.zeros(n, np.float32)
    for r in range(n):
        if summary[r, 2] == ROUTE_OK:
            seeds[r], clear_min[r] = F.window_seed(tex, LO, hi, samples[r], origins[r], window, s_pts[r], g_pts[r], clearance, smooth_iters, DT)
    return seeds, clear_min


def first_iteration_verdicts(name, samples, s_pts, g_pts, clearance):
    """(accepted, rejected): how many interior midpoints of the first iteration have a texel above the clearance, and how many do not"""
    routable, _, _, _, _, tex, hi = grid(name)
    acc = rej = 0
    for r in range(len(samples)):
        p = np.ascontiguousarray(cell_centres(samples[r], LO, hi, routable.shape), dtype=np.float32)
        p[0], p[-1] = s_pts[r], g_pts[r]
        c = np.float32(0.5) * (p[:-2] + p[2:])
        ix, iy = _texels(c, LO, hi, routable.shape)
        ok = tex[ix, iy, 0] > np.float32(clearance)
        acc, rej = acc + int(ok.sum()), rej + int((~ok).sum())
    return acc, rej
