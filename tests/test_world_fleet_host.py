"""CPU: world fleets (mmd_amd.world_fleet) -- the definition of a robot's next sub-goal and window (window_goal) on written-out grids of
40 x 30 cells with reach 5 and window 12: the staircase on open ground, a wall with a door, the two stops, every status; its two facts,
containment by brute force over every start cell and progress by iterating the definition along a serpentine; the inverse of the window
origins; the release of a map set; and the argument checks of mmd_grid_window_goals, which answer before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

import world_fleet_model as M
from mmd_amd import _lib, environments as E, map_textures, world_fleet as F
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, UNREACHED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACH, WINDOW = M.REACH, M.WINDOW
FAR = 14                         # a reach that no walk below meets, with WIDE: the whole path in one call
WIDE = 30


def walk_cells(dist, start, goal, reach, window):
    """the cells of the walk, one by one: the cell after k steps is window_goal's with max_steps = k"""
    cells = []
    while True:
        cell, _, steps, remaining, status = F.window_goal(dist, start, goal, reach, len(cells) + 1, window)
        assert status == ROUTE_OK
        if steps <= len(cells):
            return cells
        assert steps == len(cells) + 1 and remaining == int(dist[tuple(start)]) - steps
        cells.append(cell)


# ---- 1. the walk ------------------------------------------------------------------------------------------------------------------------------
def test_open_ground_gives_a_staircase():
    goal, start = (20, 15), (14, 10)
    dist = M.fields(M.open_grid(), [goal])[0]
    stairs = [(15, 10), (16, 10), (16, 11), (17, 11), (17, 12), (18, 12), (18, 13), (19, 13), (19, 14), (20, 14), (20, 15)]
    assert walk_cells(dist, start, goal, FAR, WIDE) == stairs
    # x goes first on a tie, and alone while the goal is farther along x
    assert walk_cells(dist, (10, 12), goal, FAR, WIDE)[:8] == [(11, 12), (12, 12), (13, 12), (14, 12), (15, 12), (16, 12), (17, 12), (18, 12)]
    # towards lower indices, and y first where the goal is farther along y
    assert walk_cells(dist, (22, 19), goal, FAR, WIDE) == [(22, 18), (22, 17), (21, 17), (21, 16), (20, 16), (20, 15)]
    # the reach stop on its own: the step to (20, 14) would be 6 cells from the start along x
    assert F.window_goal(dist, start, goal, REACH, 100, WINDOW) == ((19, 14), (8, 4), 9, 2, ROUTE_OK)
    # the max_steps stop on its own, inside the box
    assert F.window_goal(dist, start, goal, REACH, 3, WINDOW) == ((16, 11), (8, 4), 3, 8, ROUTE_OK)
    # one cell from the goal, and on it
    assert F.window_goal(dist, (20, 14), goal, REACH, 100, WINDOW) == ((20, 15), (14, 8), 1, 0, ROUTE_OK)
    assert F.window_goal(dist, (19, 15), goal, REACH, 1, WINDOW) == ((20, 15), (13, 9), 1, 0, ROUTE_OK)
    assert F.window_goal(dist, goal, goal, REACH, 100, WINDOW) == (goal, (14, 9), 0, 0, ROUTE_OK)
    # the window is clamped to the grid at both ends of both axes
    assert F.window_goal(dist, (2, 27), goal, REACH, 1, WINDOW)[1] == (0, 18)
    assert F.window_goal(dist, (38, 1), goal, REACH, 1, WINDOW)[1] == (28, 0)


def test_a_wall_with_a_door():
    goal, start = (25, 5), (15, 5)
    routable = M.door_grid()
    dist = M.fields(routable, [goal])[0]
    assert dist[start] == 44 and dist[20, 5] == UNREACHED
    want = ([(ix, 5) for ix in range(16, 20)] + [(19, iy) for iy in range(6, 23)] + [(20, 22), (21, 22)] +
            [(21, iy) for iy in range(21, 8, -1)] + [(22, 9), (22, 8), (23, 8), (23, 7), (24, 7), (24, 6), (25, 6), (25, 5)])
    assert len(want) == 44
    # the whole path needs a box of 17 cells, more than a window on this grid allows: walk it in calls of reach 5, each from the cell the
    # one before reached (the step rule does not read the start)
    calls = M.iterate(dist, start, goal, REACH, 100, WINDOW)
    cells = []
    for c0, cell, origin, steps, remaining in calls:
        cells += walk_cells(dist, c0, goal, REACH, WINDOW)
        assert cells[-1] == cell and len(cells) == 44 - remaining
    assert cells == want
    assert (20, 22) in cells and all(routable[c] for c in cells)
    # the first call stops under the wall: (19, 5) is 4 cells along x, then up to the box's edge
    assert calls[0][1:] == ((19, 10), (9, 0), 9, 35)


def test_every_status_and_the_batch_form():
    dist, goal, sticks_at = M.unconverged_field()
    assert F.window_goal(dist[0], (-1, 3), goal, REACH, 9, WINDOW) == ((0, 0), (0, 0), -1, -1, ROUTE_OUTSIDE)
    assert F.window_goal(dist[0], (3, 30), goal, REACH, 9, WINDOW) == ((0, 0), (0, 0), -1, -1, ROUTE_OUTSIDE)
    assert F.window_goal(dist[0], (40, 0), goal, REACH, 9, WINDOW) == ((0, 0), (0, 0), -1, -1, ROUTE_OUTSIDE)
    assert F.window_goal(dist[0], sticks_at, goal, REACH, 9, WINDOW) == (sticks_at, (4, 4), 0, 14, ROUTE_STUCK)
    assert F.window_goal(dist[0], (10, 12), goal, REACH, 9, WINDOW) == (sticks_at, (4, 6), 2, 14, ROUTE_STUCK)
    walled = M.fields(M.door_grid(door=(0, 0)), [(25, 5)])[0]
    assert F.window_goal(walled, (15, 5), (25, 5), REACH, 9, WINDOW) == ((0, 0), (0, 0), -1, -1, ROUTE_UNREACHED)
    assert F.window_goal(walled, (20, 5), (25, 5), REACH, 9, WINDOW) == ((0, 0), (0, 0), -1, -1, ROUTE_UNREACHED)       # on the wall
    both = np.concatenate([dist, M.fields(M.open_grid(), [(20, 15)])])
    goals = [goal, (20, 15)]
    starts = [(10, 12), (14, 10), (20, 15), (-1, 3), (14, 10), (14, 10), (20, 14)]
    which = [0, 1, 1, 1, 2, -1, 1]
    cells, origins, summary = F.window_goals(both, starts, which, goals, REACH, 100, WINDOW)
    assert cells.dtype == origins.dtype == summary.dtype == np.int32
    assert cells.tolist() == [[10, 10], [19, 14], [20, 15], [0, 0], [0, 0], [0, 0], [20, 15]]
    assert origins.tolist() == [[4, 6], [8, 4], [14, 9], [0, 0], [0, 0], [0, 0], [14, 8]]
    assert summary.tolist() == [[2, 14, ROUTE_STUCK, 0], [9, 2, ROUTE_OK, 0], [0, 0, ROUTE_OK, 1], [-1, -1, ROUTE_OUTSIDE, 0],
                                [-1, -1, ROUTE_OUTSIDE, 0], [-1, -1, ROUTE_OUTSIDE, 0], [1, 0, ROUTE_OK, 1]]
    for reach, max_steps, window in ((0, 9, 12), (6, 9, 12), (5, 0, 12), (5, 9, 31), (2, 9, 5)):
        with pytest.raises(ValueError, match="reach"):
            F.window_goal(both[1], (14, 10), (20, 15), reach, max_steps, window)
    assert F.window_goal(both[1], (14, 10), (20, 15), 1, 9, 5)[2] == 1                    # window 5: h = 2, reach 1 is allowed


# ---- 2. the two facts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [12, 13])
def test_containment_over_every_start_cell(window):
    nx, ny = M.SMALL
    dist = M.fields(M.open_grid(), [(20, 15)])[0]
    h = window // 2
    n = np.asarray(M.SMALL)
    for reach in (1, 3, h - 1):
        box = np.stack(np.meshgrid(np.arange(-reach, reach + 1), np.arange(-reach, reach + 1), indexing="ij"), -1).reshape(-1, 2)
        for x0 in range(nx):
            for y0 in range(ny):
                c0 = np.asarray((x0, y0))
                origin = np.asarray(F.window_goal(dist, (x0, y0), (20, 15), reach, 1, window)[1])
                assert (origin >= 0).all() and (origin + window <= n).all()
                assert (origin == np.clip(c0 - h, 0, n - window)).all()
                cells = c0 + box
                cells = cells[((cells >= 0) & (cells < n)).all(1)]
                assert ((cells >= origin) & (cells < origin + window)).all(), (x0, y0, reach)
                low_free, high_free = c0 - h >= 0, c0 - h <= n - window               # per axis: the window was not clamped to that edge
                assert ((cells - origin >= h - reach) | ~low_free).all(), (x0, y0, reach)
                assert ((origin + window - cells >= h - reach) | ~high_free).all(), (x0, y0, reach)
    # the clamped corners, spelled out
    assert F.window_goal(dist, (0, 0), (20, 15), 1, 1, window)[1] == (0, 0)
    assert F.window_goal(dist, (nx - 1, ny - 1), (20, 15), 1, 1, window)[1] == (nx - window, ny - window)
    assert F.window_goal(dist, (0, ny - 1), (20, 15), 1, 1, window)[1] == (0, ny - window)


@pytest.mark.parametrize("reach, max_steps", [(5, 100), (5, 3), (2, 7), (1, 1)])
def test_progress_and_the_epoch_bound_on_a_serpentine(reach, max_steps):
    routable = M.serpentine_grid()
    goal, start = (37, 2), (2, 2)
    dist = M.fields(routable, [goal])[0]
    d0 = int(dist[start])
    assert d0 == 135                                         # the corridor, not the straight line of 35 cells
    calls = M.iterate(dist, start, goal, reach, max_steps, WINDOW)
    d = d0
    for c0, cell, origin, steps, remaining in calls:
        assert int(dist[c0]) == d and steps >= min(d, max_steps, reach) and steps <= max_steps
        assert remaining == d - steps == int(dist[cell]) and routable[cell]
        assert max(abs(cell[0] - c0[0]), abs(cell[1] - c0[1])) <= reach
        assert all(origin[k] <= cell[k] < origin[k] + WINDOW and origin[k] <= c0[k] < origin[k] + WINDOW for k in range(2))
        d = remaining
    assert calls[-1][1] == goal
    assert len(calls) <= F.epoch_bound(d0, reach, max_steps) == -(-d0 // min(reach, max_steps))
    if max_steps <= reach:
        assert len(calls) == F.epoch_bound(d0, reach, max_steps)          # every call but the last takes exactly max_steps steps
    assert F.epoch_bound(0, 5, 3) == 0 and F.epoch_bound(1, 5, 3) == 1 and F.epoch_bound(6, 5, 3) == 2 and F.epoch_bound(7, 3, 5) == 3


# ---- 3. the offsets of window origins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [None, (1.0, 1.0), (-7.3, 2.9)])
def test_window_offsets_are_the_inverse_of_window_origins(origin):
    name = "FleetOffsets"
    E.register_world_map(name, np.zeros((2048, 2048), np.uint8), origin=origin)
    try:
        k = np.arange(2048 - 400 + 1, dtype=np.int32)
        origins = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(-1, 2)           # every origin of the world
        offsets = E.world_map_window_offsets(name, origins)
        assert offsets.dtype == np.float32 and offsets.shape == origins.shape
        back = E.world_map_window_origins(name, offsets)
        assert back.dtype == np.int32 and np.array_equal(back, origins)
        assert np.array_equal(offsets.view(np.uint32), E.snap_to_world_map(name, offsets).view(np.uint32))
        for bad in ([[-1, 0]], [[0, 1649]], [[0.0, 1.0]], np.zeros((0, 2), np.int32)):
            with pytest.raises(ValueError):
                E.world_map_window_offsets(name, bad)
    finally:
        E.unregister_world_map(name)


# ---- 4. the release of a map set -------------------------------------------------------------------------------------------------------------------
def test_release_forgets_exactly_one_map_set():
    a, b = (("W@0,0", "W@0,5"), "cpu"), (("W@0,0",), "cpu")
    kept = dict(map_textures._TEXTURES), dict(map_textures._WINDOW_CUTS)
    try:
        for key in (a, b):
            map_textures._TEXTURES[key] = object()
            map_textures._WINDOW_CUTS[key] = [("W", 0, None)]
        tensor = map_textures._TEXTURES[a]
        assert map_textures.release_sdf_textures(["W@0,0", "W@0,5"], "cpu") is True
        assert a not in map_textures._TEXTURES and a not in map_textures._WINDOW_CUTS and tensor is not None
        assert b in map_textures._TEXTURES and b in map_textures._WINDOW_CUTS
        assert map_textures.release_sdf_textures(["W@0,0", "W@0,5"], "cpu") is False          # not resident: nothing to forget
        assert map_textures.release_sdf_textures(("W@0,0",), "cpu") is True
        assert (dict(map_textures._TEXTURES), dict(map_textures._WINDOW_CUTS)) == kept
    finally:
        for key in (a, b):
            map_textures._TEXTURES.pop(key, None)
            map_textures._WINDOW_CUTS.pop(key, None)


# ---- 5. the C entry point answers before any launch ------------------------------------------------------------------------------------------------
def test_entry_point_argument_checks():
    lib = _lib.load()
    assert "mmd_grid_window_goals" in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES["mmd_grid_window_goals"][1]) == 15
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9                           # one additive symbol under v9
    assert " mmd_grid_window_goals(" in open(os.path.join(ROOT, "include", "mmd_amd.h")).read()
    for name in ("build.sh", "__graft_entry__.py"):
        assert "mmd_amd/csrc/window_goals.hip" in open(os.path.join(ROOT, name)).read()
    p = C.c_void_p(256)                                      # never dereferenced: every call below returns before a launch
    good = dict(nx=40, ny=30, n_fields=2, n=7, reach=5, max_steps=9, window=12)

    def call(dist=p, starts=p, field=p, goals=p, cells=p, origins=p, summary=p, **kw):
        a = dict(good, **kw)
        return lib.mmd_grid_window_goals(dist, a["nx"], a["ny"], a["n_fields"], starts, field, goals, a["n"], a["reach"], a["max_steps"],
                                         a["window"], cells, origins, summary, None)
    assert call(n=0) == 0 and call(n=0, dist=None, starts=None, field=None, goals=None, cells=None, origins=None, summary=None) == 0
    for kw, word in ((dict(nx=0), "grid"), (dict(ny=2049), "grid"), (dict(n_fields=-1), "n_fields"), (dict(n=-1), "n_queries"),
                     (dict(reach=0), "reach"), (dict(reach=6), "reach"), (dict(max_steps=0), "max_steps"), (dict(window=31), "window"),
                     (dict(window=0), "window"), (dict(window=3, reach=1), "reach"), (dict(n=0, reach=0), "reach"),
                     (dict(dist=None), "NULL dist"), (dict(goals=None), "NULL goals"), (dict(starts=None), "NULL starts"),
                     (dict(field=None), "NULL field"), (dict(cells=None), "NULL cells"), (dict(origins=None), "NULL origins"),
                     (dict(summary=None), "NULL summary")):
        assert call(**kw) == 2, kw
        assert word.encode() in lib.mmd_last_error(), (kw, lib.mmd_last_error())
