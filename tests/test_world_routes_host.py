"""CPU: world routes (mmd_amd/world_routes.py).  The numpy definitions -- routable_cells, grid_distance_field, descend -- on hand-made grids
with the integers written out and against scipy's shortest paths; the descent's tie rules and statuses on hand-made distance arrays
(tests/world_route_model.py); world_route on the host texture of a two-tile world; the three entry points' symbols and every error return,
answered before any device call (there is no GPU here)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mmd_amd import _lib, environments as E, world_routes as R
import world_route_model as M

U = R.UNREACHED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    worlds = set(E.registered_world_maps())
    yield
    for name in set(E.registered_world_maps()) - worlds:
        E.unregister_world_map(name)


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------
def test_routable_cells_is_a_strict_fp32_compare_inside_the_region():
    tex = np.zeros((3, 4, 4), np.float32)
    c = np.float32(0.16)
    tex[..., 0] = [[c, np.nextafter(c, np.float32(1)), np.nextafter(c, np.float32(0)), np.nan],
                   [1.0, -1.0, np.inf, -np.inf],
                   [1.0, 1.0, 1.0, 1.0]]
    assert R.routable_cells(tex, 0.16).tolist() == [[False, True, False, False], [True, False, True, False], [True] * 4]
    assert R.routable_cells(tex, 0.16, (1, 1, 3, 3)).tolist() == [[False] * 4, [False, False, True, False], [False, True, True, False]]
    assert not R.routable_cells(tex, 0.16, (1, 1, 1, 3)).any()                      # an empty region
    for region in ((0, 0, 4, 4), (2, 0, 1, 4), (-1, 0, 3, 4), (0, 0, 3)):
        with pytest.raises(ValueError):
            R.routable_cells(tex, 0.16, region)


def test_distance_field_on_hand_made_grids():
    # an open 5 x 7 grid: the Manhattan distance
    d = R.grid_distance_field(np.ones((5, 7), bool), [(1, 2), (4, 6)])
    assert d.dtype == np.int32 and d.shape == (2, 5, 7)
    assert d[0].tolist() == [[3, 2, 1, 2, 3, 4, 5],
                             [2, 1, 0, 1, 2, 3, 4],
                             [3, 2, 1, 2, 3, 4, 5],
                             [4, 3, 2, 3, 4, 5, 6],
                             [5, 4, 3, 4, 5, 6, 7]]
    assert d[1].tolist() == [[abs(i - 4) + abs(j - 6) for j in range(7)] for i in range(5)]
    # a wall with a gap: row 2 is blocked but for column 4
    free = np.ones((5, 6), bool)
    free[2, :] = False
    free[2, 4] = True
    d = R.grid_distance_field(free, [(0, 0)])[0]
    assert d.tolist() == [[0, 1, 2, 3, 4, 5],
                          [1, 2, 3, 4, 5, 6],
                          [U, U, U, U, 6, U],
                          [11, 10, 9, 8, 7, 8],
                          [12, 11, 10, 9, 8, 9]]
    # a blocked goal, a goal outside the grid, a walled-in goal
    free[0, 0] = False
    assert (R.grid_distance_field(free, [(0, 0), (5, 0), (0, -1), (-1, 2)]) == U).all()
    free = np.ones((3, 3), bool)
    free[0, 1] = free[1, 0] = False
    assert R.grid_distance_field(free, [(0, 0)])[0].tolist() == [[0, U, U], [U, U, U], [U, U, U]]
    assert R.grid_distance_field(np.ones((1, 1), bool), [(0, 0)]).tolist() == [[[0]]]


def test_distance_field_against_scipy():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import shortest_path
    free = M.random_free((37, 21), seed=3)
    nx, ny = free.shape
    idx = np.arange(nx * ny).reshape(nx, ny)
    pairs = [(idx[:-1, :][free[:-1, :] & free[1:, :]], idx[1:, :][free[:-1, :] & free[1:, :]]),
             (idx[:, :-1][free[:, :-1] & free[:, 1:]], idx[:, 1:][free[:, :-1] & free[:, 1:]])]
    a, b = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    graph = coo_matrix((np.ones(a.size), (a, b)), shape=(nx * ny, nx * ny)).tocsr()
    goals = [tuple(c) for c in np.argwhere(free)[[0, 57, 200, -1]].tolist()] + [tuple(np.argwhere(~free)[5].tolist())]
    ours = R.grid_distance_field(free, goals)
    for f, g in enumerate(goals[:4]):
        want = shortest_path(graph, directed=False, unweighted=True, indices=idx[g]).reshape(nx, ny)
        want = np.where(np.isfinite(want) & free, want, U).astype(np.int64)
        assert np.array_equal(ours[f], want), g
    assert (ours[:4] != U).sum() > 4 * 100 and (ours[4] == U).all()


@pytest.mark.parametrize("case", sorted(M.descent_cases()))
def test_descent_rules(case):
    args, want = M.descent_cases()[case]
    M.check_descent(R.descend(*args), want)


def test_descent_arguments_and_models():
    d = np.zeros((2, 2), np.int32)
    for tile, max_tiles in ((0, 4), (2, 0)):
        with pytest.raises(ValueError):
            R.descend(d, (0, 0), tile, (0, 0), max_tiles)
    # the models the GPU tests lean on: the serpentine's level count and the block-synchronous sweep counts
    free = M.serpentine_free()
    ref = R.grid_distance_field(free, [M.SERPENTINE_GOAL])[0]
    assert int(ref[ref != U].max()) + 1 == M.SERPENTINE_LEVELS and (ref != U).sum() == free.sum()
    sweeps, dist = M.block_sync_sweeps(free, M.SERPENTINE_GOAL)
    assert sweeps == 37 and np.array_equal(dist, ref)
    assert M.block_sync_sweeps(np.ones((37, 21), bool), (0, 0), block=8)[0] == 5 + 3
    for shape, want in (((130, 70), 5), ((64, 64), 2), ((65, 129), 5)):
        assert M.block_sync_sweeps(np.ones(shape, bool), (0, 0))[0] == want


# ---- a two-tile world on the host ------------------------------------------------------------------------------------------------------------
def test_world_route_on_the_host_texture(registry):
    occ = np.zeros((800, 400), np.uint8)
    occ[398:402, :] = 1
    occ[398:402, 140:260] = 0                       # a door of 120 cells: a clearance of 0.16 leaves the 56 more than 32.5 cells from both jambs
    E.register_world_map("TwoTiles", occ)
    assert R.world_lattice("TwoTiles") == ((0, 0, 800, 400), (2, 1))
    assert R.world_lattice("TwoTiles", (1, 0)) == ((1, 0, 401, 400), (1, 1))
    for origin in ((-1, 0), (0, 400), (401, 0)):
        with pytest.raises(ValueError):
            R.world_lattice("TwoTiles", origin)
    start, goal = M.cell_centre((100, 50), (800, 400)), M.cell_centre((700, 350), (800, 400))
    assert R.world_cells("TwoTiles", np.stack([start, goal])).tolist() == [[100, 50], [700, 350]]
    route = R.world_route("TwoTiles", start, goal)
    assert route.tiles.tolist() == [[0, 0], [1, 0]] and route.tiles.dtype == np.int32
    assert route.origins.tolist() == [[0, 0], [400, 0]] and route.origins.dtype == np.int32
    assert route.offsets.dtype == np.float32 and np.array_equal(route.offsets, E.snap_to_world_map("TwoTiles", route.offsets))
    assert (route.offsets[1] - route.offsets[0]).tolist() == [2.0, 0.0]                      # one tile pitch along x, exactly
    assert sorted(route.transforms) == [0, 1] and all(torch.equal(route.transforms[k], torch.from_numpy(route.offsets[k])) for k in (0, 1))
    assert route.env_ids == ["TwoTiles@0,0", "TwoTiles@400,0"]
    for k, name in enumerate(route.env_ids):
        kind, world, _, origin = E.resolve_map(name)
        assert (kind, world, tuple(origin)) == ("window", "TwoTiles", tuple(route.origins[k].tolist()))
    # the start lies in window 0 and the goal in window 1, in the frame MPDEnsemble gives them
    assert (np.abs(start - route.offsets[0]) <= 1).all() and (np.abs(goal - route.offsets[1]) <= 1).all()
    # steps: the definition on the same mask; through the door, so longer than the Manhattan distance
    rt = R.routable_cells(E.world_map_texture("TwoTiles"), R.OBSTACLE_MARGIN, (0, 0, 800, 400))
    assert route.steps == int(R.grid_distance_field(rt, [(700, 350)])[0][100, 50]) and route.steps >= 600 + 300
    assert not rt[398:402].all(1).any() and rt[400, 172:228].all() and not rt[400, 171] and not rt[400, 228]
    back, same = R.world_routes("TwoTiles", np.stack([goal, start]), np.stack([start, start]))
    assert back.tiles.tolist() == [[1, 0], [0, 0]] and back.steps == route.steps
    assert same.tiles.tolist() == [[0, 0]] and same.steps == 0 and same.env_ids == ["TwoTiles@0,0"]
    # refusals: the leftover strip of a shifted lattice, a point outside the world, a goal inside the wall, too many tiles
    with pytest.raises(ValueError, match="leftover strip"):
        R.world_route("TwoTiles", start, goal, lattice_origin=(1, 0))
    with pytest.raises(ValueError, match="outside the world"):
        R.world_route("TwoTiles", start, np.asarray([2.5, 0.0], np.float32))
    with pytest.raises(ValueError, match="outside the world"):
        R.world_route("TwoTiles", np.asarray([np.nan, 0.0], np.float32), goal)
    with pytest.raises(ValueError, match=r"goal cell \[399, 10\] cannot be reached from the start cell \[100, 50\]"):
        R.world_route("TwoTiles", start, M.cell_centre((399, 10), (800, 400)))
    with pytest.raises(ValueError, match="crosses 2 tiles, above max_tiles = 1"):
        R.world_route("TwoTiles", start, goal, max_tiles=1)


def test_route_planner_is_the_mpd_ensemble_call(monkeypatch):
    from mmd_amd import planners
    seen = {}
    monkeypatch.setattr(planners, "MPDEnsemble", lambda **kw: seen.update(kw) or "planner")
    route = R.WorldRoute(np.zeros((3, 2), np.int32), np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float32), {0: 0, 1: 1, 2: 2},
                         ["a", "b", "a"], 7)
    assert R.route_planner(route, "Model", "s", "g", planner_alg="mmd", seed=3) == "planner"
    assert seen == dict(model_ids=("Model",) * 3, transforms=route.transforms, env_ids=route.env_ids, start_state_pos="s", goal_state_pos="g",
                        planner_alg="mmd", seed=3)


# ---- the C boundary, without a GPU ----------------------------------------------------------------------------------------------------------------
NAMES = ("mmd_grid_distance_work_bytes", "mmd_grid_distance_field", "mmd_grid_descend")


def test_abi_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mmd_amd.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header
    assert "#define MMD_GRID_DIST_BLOCK 64" in header and "#define MMD_GRID_DIST_UNREACHED 0x7fffffff" in header
    assert (_lib.GRID_DIST_BLOCK, _lib.GRID_DIST_UNREACHED, R.UNREACHED) == (64, 0x7fffffff, 0x7fffffff)
    assert [len(_lib._SIGNATURES[n][1]) for n in NAMES] == [3, 14, 13]
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9
    assert C.sizeof(_lib.ConsBins) == 56 and C.sizeof(_lib.Conflict) == 48 and C.sizeof(_lib.UnetOptions) == 20
    for name in ("build.sh", "__graft_entry__.py"):
        assert "mmd_amd/csrc/grid_route.hip" in open(os.path.join(ROOT, name)).read()
    # the workspace: per field a sweep count and a word per 64 x 64 block; 0 for a size that is refused
    wb = lib.mmd_grid_distance_work_bytes
    assert wb(1, 1, 1) == 8 and wb(64, 64, 3) == 24 and wb(65, 129, 3) == 3 * 7 * 4 and wb(2048, 2048, 16) == 16 * 1025 * 4
    assert wb(130, 70, 0) == 0
    for args in ((0, 5, 1), (5, 0, 1), (2049, 5, 1), (5, 2049, 1), (5, 5, -1), (5, 5, 65536)):
        assert wb(*args) == 0


def _refused(fn, args, word):
    lib = _lib.load()
    rc = fn(*args)
    msg = lib.mmd_last_error().decode()
    assert rc != 0 and word in msg, (args, rc, msg)


def test_distance_field_error_returns():
    lib = _lib.load()
    p = C.c_void_p(4096)              # never read: every call below is refused, or has nothing to do
    region = (C.c_int32 * 4)(0, 0, 37, 45)
    ok = [p, 37, 45, 0.16, region, p, 2, 1, 3, p, p, 10 ** 6, p, None]
    fn = lib.mmd_grid_distance_field

    def with_(k, v):
        a = list(ok)
        a[k] = v
        return a
    for k, word in ((0, "NULL grid"), (5, "NULL goals"), (9, "NULL dist"), (10, "NULL workspace"), (12, "NULL changed"), (4, "NULL region")):
        _refused(fn, with_(k, None), word)
    for k, v, word in ((1, 0, "cells"), (1, 2049, "cells"), (2, 0, "cells"), (2, 2049, "cells"), (6, -1, "n_fields"), (6, 65536, "n_fields"),
                       (8, -1, "n_sweeps"), (3, float("nan"), "clearance"), (3, float("inf"), "clearance"), (3, float("-inf"), "clearance"),
                       (11, lib.mmd_grid_distance_work_bytes(37, 45, 2) - 1, "work_bytes"), (11, 0, "work_bytes")):
        _refused(fn, with_(k, v), word)
    for r in ((5, 0, 4, 45), (0, 9, 37, 8), (-1, 0, 37, 45), (0, -1, 37, 45), (0, 0, 38, 45), (0, 0, 37, 46)):
        _refused(fn, with_(4, (C.c_int32 * 4)(*r)), "region")
    # nothing to do: no field (whatever the pointers), or no sweep and no restart
    a = with_(6, 0)
    for k in (0, 5, 9, 10, 12):
        a[k] = None
    assert fn(*a) == 0
    a = with_(8, 0)
    a[7] = 0
    assert fn(*a) == 0
    # an empty region is a valid one: refused only for what else is wrong
    _refused(fn, with_(4, (C.c_int32 * 4)(7, 7, 7, 7))[:9] + [None] + ok[10:], "NULL dist")


def test_descend_error_returns():
    lib = _lib.load()
    p = C.c_void_p(4096)
    origin = (C.c_int32 * 2)(0, 0)
    ok = [p, 37, 45, 2, p, p, 5, 16, origin, 4, p, p, None]
    fn = lib.mmd_grid_descend

    def with_(k, v):
        a = list(ok)
        a[k] = v
        return a
    for k, word in ((0, "NULL dist"), (4, "NULL starts"), (5, "NULL field"), (10, "NULL tiles"), (11, "NULL summary"), (8, "NULL lattice_origin")):
        _refused(fn, with_(k, None), word)
    for k, v, word in ((1, 0, "cells"), (1, 2049, "cells"), (2, 0, "cells"), (2, 2049, "cells"), (3, -1, "n_fields"), (6, -1, "n_queries"),
                       (7, 0, "tile"), (7, -4, "tile"), (9, 0, "max_tiles"), (9, -1, "max_tiles"),
                       (8, (C.c_int32 * 2)(2 ** 30 + 1, 0), "lattice_origin"), (8, (C.c_int32 * 2)(0, -2 ** 30 - 1), "lattice_origin")):
        _refused(fn, with_(k, v), word)
    a = with_(6, 0)                     # no query: nothing to do, whatever the pointers
    for k in (0, 4, 5, 10, 11):
        a[k] = None
    assert fn(*a) == 0
