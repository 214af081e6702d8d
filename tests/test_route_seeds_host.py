"""CPU: the seed trajectories of world routes.  The numpy functions descend_samples and seed_trajectory (mmd_amd/world_routes.py) ARE the
definition: here their rules are pinned on written-out grids and hand-built textures, the kernel's two-walk form (route_seed_model.py) is
held to the definition, and the two entry points' error returns are checked at the C boundary, where nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mmd_amd import _lib, environments as E, world_routes as R
import route_seed_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def registry():
    worlds = set(E.registered_world_maps())
    yield
    for name in set(E.registered_world_maps()) - worlds:
        E.unregister_world_map(name)


# ---- the sample-index rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 2, 63, 64, 65, 4000))
def test_sample_offsets(m):
    off = R.sample_offsets(m)
    assert off.shape == (64,) and off[0] == 0 and off[63] == m - 1 and (np.diff(off) >= 0).all()
    assert off.tolist() == [(j * (m - 1) + 31) // 63 for j in range(64)]
    if m <= 64:
        assert set(off.tolist()) == set(range(m))                           # every path cell is hit
    else:
        assert len(set(off.tolist())) == 64 and np.diff(off).max() <= -(-(m - 1) // 63)


# ---- descend_samples on written-out grids ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.grids()))
def test_descend_samples_on_grids(name):
    free, goal, tile, origin, starts = M.grids()[name]
    dist = M.field_of(free, goal)
    for start in starts:
        found = R.descend_samples(dist, start, tile, origin, 128)
        tiles, steps, n_tiles, status, visit_cells, cells = found
        want = R.descend(dist, start, tile, origin, 128)
        assert np.array_equal(tiles, want[0]) and (steps, n_tiles, status) == want[1:] and status == R.ROUTE_OK
        assert visit_cells.dtype == np.int32 and cells.dtype == np.int32 and cells.shape == (n_tiles, 64, 2)
        assert visit_cells.shape == (n_tiles,) and (visit_cells >= 1).all() and int(visit_cells.sum()) == steps + 1
        assert cells[0, 0].tolist() == list(start) and cells[-1, 63].tolist() == list(goal)
        flat = cells.reshape(-1, 2)
        d = dist[flat[:, 0], flat[:, 1]]
        assert free[flat[:, 0], flat[:, 1]].all() and (np.diff(d) <= 0).all() and d[0] == steps and d[-1] == 0
        first = np.concatenate([[0], np.cumsum(visit_cells)[:-1]])
        for k in range(n_tiles):
            assert np.array_equal((cells[k] - np.asarray(origin)) // tile, np.tile(tiles[k], (64, 1)))          # in the visit's tile
            assert np.array_equal(steps - dist[cells[k, :, 0], cells[k, :, 1]], first[k] + R.sample_offsets(visit_cells[k]))   # path cells
        # the kernel's two-walk form leaves the same rows
        got = M.two_walk_samples(dist, start, tile, origin, 128)
        vc, padded = M.padded(found, 128)
        assert np.array_equal(got[0][:n_tiles], tiles) and got[1].tolist() == [steps, n_tiles, status, 0]
        assert np.array_equal(got[2], vc) and np.array_equal(got[3], padded)


def test_descend_samples_visits():
    g = M.grids()
    free, goal, tile, origin, starts = g["clipped_corner"]
    found = R.descend_samples(M.field_of(free, goal), starts[0], tile, origin)
    assert found[0].tolist() == [[0, 0], [1, 0], [1, 1]] and found[4].tolist() == [2, 1, 2]                     # a visit of one cell
    assert (found[5][1] == (2, 1)).all() and found[5][0, :32].tolist() == [[1, 0]] * 32 and found[5][0, 32:].tolist() == [[1, 1]] * 32
    free, goal, tile, origin, starts = g["corridor_long_visit"]
    dist = M.field_of(free, goal)
    found = R.descend_samples(dist, starts[0], tile, origin)
    assert found[4].tolist() == [100, 100] and found[5][0, :, 1].tolist() == R.sample_offsets(100).tolist()
    assert R.descend_samples(dist, starts[1], tile, origin)[4].tolist() == [65, 100]
    free, goal, tile, origin, starts = g["corridor"]
    dist = M.field_of(free, goal)
    on_goal = R.descend_samples(dist, (1, 199), tile, origin)
    assert on_goal[1:4] == (0, 1, 0) and on_goal[4].tolist() == [1] and (on_goal[5] == (1, 199)).all()
    assert R.descend_samples(dist, (1, 0), tile, origin)[4].tolist() == [32] * 6 + [8]
    # no samples with a status other than ROUTE_OK: max_tiles exceeded, unreachable, outside
    for start, max_tiles, status in (((1, 0), 6, R.ROUTE_TOO_MANY_TILES), ((0, 5), 16, R.ROUTE_UNREACHED), ((3, 5), 16, R.ROUTE_OUTSIDE),
                                     ((1, -1), 16, R.ROUTE_OUTSIDE)):
        found = R.descend_samples(dist, start, tile, origin, max_tiles)
        want = R.descend(dist, start, tile, origin, max_tiles)
        assert found[3] == status and np.array_equal(found[0], want[0]) and found[1:4] == want[1:]
        assert found[4].shape == (0,) and found[5].shape == (0, 64, 2)
        got = M.two_walk_samples(dist, start, tile, origin, max_tiles)
        assert got[1].tolist() == [want[1], want[2], status, 0] and not got[2].any() and not got[3].any()
    assert R.descend_samples(dist, (1, 0), tile, origin, 7)[3] == R.ROUTE_OK
    # a field that was not converged: stuck, no samples
    s = np.full((1, 4), R.UNREACHED, np.int32)
    s[0, 0], s[0, 1], s[0, 2] = 5, 4, 1
    found = R.descend_samples(s, (0, 0), 1)
    assert found[3] == R.ROUTE_STUCK and found[4].shape == (0,) and found[5].shape == (0, 64, 2)
    got = M.two_walk_samples(s, (0, 0), 1, (0, 0), 4)
    assert got[1].tolist() == [1, 2, 2, 0] and got[0][:2].tolist() == [[0, 0], [0, 1]] and not got[2].any() and not got[3].any()


# ---- the centre of a cell --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,shape", (((-5.12, -5.12), (5.12, 5.12), (2048, 2048)), ((-3.7, 1.3), (6.54, 11.54), (2048, 2048)),
                                         ((100.0, -0.001), (110.24, 4.999), (2048, 1000)), ((-1.0, -1.0), (1.0, 1.0), (400, 400))))
def test_the_texel_of_a_cell_centre_is_the_cell(lo, hi, shape):
    f = np.float32
    for cells in (np.stack([np.arange(shape[0]), np.arange(shape[0]) % shape[1]], 1), np.stack([np.arange(shape[1]) % shape[0], np.arange(shape[1])], 1)):
        centres = R.cell_centres(cells, lo, hi, shape)
        assert centres.dtype == np.float32 and centres.shape == cells.shape
        pitch = [np.abs(f(hi[k]) - f(lo[k])) / f(shape[k]) for k in range(2)]
        want = np.stack([f(lo[k]) + (cells[:, k].astype(f) + f(0.5)) * pitch[k] for k in range(2)], 1)         # the sequence, written out
        assert want.dtype == np.float32 and np.array_equal(centres.view(np.uint32), want.view(np.uint32))
        ix, iy, finite = E._texel_indices(centres, lo, hi, shape)
        assert finite.all() and np.array_equal(ix, cells[:, 0]) and np.array_equal(iy, cells[:, 1])
        jx, jy = R._texels(centres, lo, hi, shape)
        assert np.array_equal(jx, ix) and np.array_equal(jy, iy)
    # R._texels is _texel_indices on every finite point, and drops a NaN as fmaxf does
    rng = np.random.Generator(np.random.PCG64(3))
    pts = (rng.random((4096, 2)) * 30 - 10).astype(np.float32)
    ix, iy, _ = E._texel_indices(pts, lo, hi, shape)
    jx, jy = R._texels(pts, lo, hi, shape)
    assert np.array_equal(ix, jx) and np.array_equal(iy, jy)
    odd = np.asarray([[np.nan, np.inf], [-np.inf, np.nan]], np.float32)
    assert [a.tolist() for a in R._texels(odd, lo, hi, shape)] == [[0, 0], [shape[1] - 1, 0]]


# ---- seed_trajectory ------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def unit_centre(cell):
    return np.asarray([cell[0] + 0.5, cell[1] + 0.5], np.float32)


def test_seed_without_smoothing_and_a_straight_chain():
    free, goal, tile, origin, starts = M.grids()["door"]
    dist = M.field_of(free, goal)
    lo, hi = (-1.2, -1.0), (1.2, 1.0)                                        # a pitch of 0.025, not a power of two
    tex = M.texture_of(free)
    tiles, steps, n_tiles, status, _, cells = R.descend_samples(dist, starts[0], tile, origin)
    start, goal_pt = np.float32([-1.123, -0.871]), np.float32([1.06, -0.869])
    assert [a.tolist() for a in R._texels(np.stack([start, goal_pt]), lo, hi, tex.shape)] == [[3, 90], [5, 5]]
    seed, clear_min = R.seed_trajectory(tex, lo, hi, cells, tiles, tile, origin, start, goal_pt, 0.0, 0, 5.0 / 64)
    assert seed.dtype == np.float32 and seed.shape == (64 * n_tiles, 4) and clear_min == 1.0 and clear_min.dtype == np.float32
    want = R.cell_centres(cells.reshape(-1, 2), lo, hi, tex.shape)
    assert np.array_equal(bits(seed[1:-1, :2]), bits(want[1:-1]))
    assert np.array_equal(bits(seed[0, :2]), bits(start)) and np.array_equal(bits(seed[-1, :2]), bits(goal_pt))   # the caller's exact points
    two_dt = np.float32(2 * 5.0 / 64)
    assert np.array_equal(bits(seed[1:-1, 2:]), bits((seed[2:, :2] - seed[:-2, :2]) / two_dt))
    assert not seed[0, 2:].any() and not seed[-1, 2:].any()                  # velocities are zero at both ends
    # the endpoints stay fixed through the smoothing
    smooth, _ = R.seed_trajectory(tex, lo, hi, cells, tiles, tile, origin, start, goal_pt, 0.0, 7, 5.0 / 64)
    assert np.array_equal(bits(smooth[[0, -1]]), bits(seed[[0, -1]])) and not np.array_equal(smooth, seed)
    # a straight chain of evenly spaced points is a fixed point (unit pitch: every midpoint is exact)
    free = np.ones((128, 3), bool)
    cells = np.stack([np.stack([np.arange(64 * k, 64 * k + 64), np.ones(64, np.int64)], 1) for k in range(2)])
    args = (M.texture_of(free), (0, 0), (128, 3), cells, [(0, 0), (1, 0)], 64, (0, 0), unit_centre((0, 1)), unit_centre((127, 1)), 0.0)
    still, _ = R.seed_trajectory(*args, 0, 0.5)
    moved, _ = R.seed_trajectory(*args, 10, 0.5)
    assert np.array_equal(bits(still), bits(moved)) and (still[1:-1, 2] == 2.0).all() and not still[:, 3].any()
    # no visit: an empty seed
    empty, clear_min = R.seed_trajectory(tex, lo, hi, np.zeros((0, 64, 2), np.int32), np.zeros((0, 2), np.int32), 32, (0, 0), start, goal_pt)
    assert empty.shape == (0, 4) and clear_min == 0
    for bad in (dict(smooth_iters=-1), dict(dt=0.0), dict(dt=float("nan"))):
        with pytest.raises(ValueError):
            R.seed_trajectory(tex, lo, hi, cells, [(0, 0), (1, 0)], 64, (0, 0), start, goal_pt, **bad)


@pytest.mark.parametrize("name", ("door", "door_shifted", "serpentine", "L"))
def test_every_point_of_every_iteration_is_clear_and_in_its_tile(name):
    free, goal, tile, origin, starts = M.grids()[name]
    dist = M.field_of(free, goal)
    lo, hi = (-1.2, -1.0), (1.2, 1.0)
    tex = M.texture_of(free)
    tiles, steps, n_tiles, status, _, cells = R.descend_samples(dist, starts[0], tile, origin, 128)
    s, g = R.cell_centres(np.asarray(starts[0]), lo, hi, tex.shape), R.cell_centres(np.asarray(goal), lo, hi, tex.shape)
    lengths = []
    for iters in (0, 1, 2, 5, 40):
        seed, clear_min = R.seed_trajectory(tex, lo, hi, cells, tiles, tile, origin, s, g, 0.0, iters, 0.1)
        ix, iy = R._texels(seed[:, :2], lo, hi, tex.shape)
        assert (tex[ix, iy, 0] > 0).all() and clear_min == 1.0
        own = np.repeat(tiles, 64, axis=0)
        assert np.array_equal((ix - origin[0]) // tile, own[:, 0]) and np.array_equal((iy - origin[1]) // tile, own[:, 1])
        lengths.append(M.polyline_length(seed))
    assert lengths[-1] < lengths[0]                                         # smoothing shortens the staircase of cell centres


def test_the_clearance_is_a_strict_compare_and_a_nan_rejects():
    for value, accepted in M.corner_values():
        tex, cells = M.corner_case(value)
        seed, clear_min = R.seed_trajectory(tex, (0, 0), (8, 8), cells, [(0, 0)], 8, (0, 0), unit_centre((1, 1)), unit_centre((3, 3)), 0.16, 1, 0.5)
        assert seed[21, :2].tolist() == ([2.5, 2.5] if accepted else [3.5, 1.5]), value
        assert seed[20, :2].tolist() == [2.5, 1.5] and seed[22, :2].tolist() == [3.5, 2.5] and seed[19, :2].tolist() == [1.5, 1.5]
        assert bits(clear_min) == bits(value if accepted else np.float32(1))


def test_a_candidate_across_a_lattice_line_is_rejected():
    tex, cells = M.lattice_case()
    ends = unit_centre((3, 1)), unit_centre((7, 1))
    seed, _ = R.seed_trajectory(tex, (0, 0), (8, 8), cells, [(0, 0), (1, 0)], 4, (0, 0), *ends, 0.0, 1, 0.5)
    assert seed[63, :2].tolist() == [3.5, 1.5] and seed[64, :2].tolist() == [5.5, 1.5] and seed[65, :2].tolist() == [6.5, 1.5]
    one_tile, _ = R.seed_trajectory(tex, (0, 0), (8, 8), cells, [(0, 0), (0, 0)], 8, (0, 0), *ends, 0.0, 1, 0.5)
    assert one_tile[63, :2].tolist() == [4.5, 1.5]                          # the same candidate, with no line in the way
    shifted, _ = R.seed_trajectory(tex, (0, 0), (8, 8), cells, [(0, 0), (1, 0)], 4, (1, 0), *ends, 0.0, 1, 0.5)       # the line at ix = 5
    assert shifted[63, :2].tolist() == [4.5, 1.5] and shifted[64, :2].tolist() == [5.5, 1.5]


def test_clear_min_orders_by_the_bits():
    v = np.float32([0.0, -0.0, 1.0, np.inf])
    assert bits(v[np.argmin(R._bits_order(v))]) == bits(np.float32(-0.0))
    v = np.float32([3.0, np.nan, -2.0, -np.inf])
    assert v[np.argmin(R._bits_order(v))] == -np.inf and np.isnan(v[np.argmax(R._bits_order(v))])
    assert np.array_equal(R._bits_order(R._bits_order(v).view(np.float32)), bits(v))                            # its own inverse


# ---- the public interface on the host ------------------------------------------------------------------------------------------------------------
def test_world_route_seeded_on_the_host_texture(registry):
    occ = np.zeros((800, 400), np.uint8)
    occ[398:402, :] = 1
    occ[398:402, 140:260] = 0
    E.register_world_map("SeedTwoTiles", occ)
    start, goal = M.cell_centre((100, 50), (800, 400)) + np.float32(0.001), M.cell_centre((700, 350), (800, 400))
    route, seed = R.world_route_seeded("SeedTwoTiles", start, goal, smooth_iters=16)
    plain = R.world_route("SeedTwoTiles", start, goal)
    assert route.tiles.tolist() == [[0, 0], [1, 0]] and np.array_equal(route.tiles, plain.tiles) and route.steps == plain.steps
    assert route.env_ids == plain.env_ids and np.array_equal(route.offsets, plain.offsets)
    assert isinstance(seed, torch.Tensor) and seed.dtype == torch.float32 and seed.shape == (128, 4)
    assert torch.equal(seed[0, :2], torch.from_numpy(start)) and torch.equal(seed[-1, :2], torch.from_numpy(goal))
    # every support point keeps the margin and lies in its own window: in the window's frame it is inside the tile's limits
    tex = E.world_map_texture("SeedTwoTiles")
    lo, hi = E.world_map_limits("SeedTwoTiles")
    ix, iy = R._texels(seed[:, :2].numpy(), lo, hi, tex.shape)
    assert (tex[ix, iy, 0] > np.float32(R.OBSTACLE_MARGIN)).all() and (ix[:64] < 400).all() and (ix[64:] >= 400).all()
    for k in range(2):
        assert (np.abs(seed[64 * k:64 * k + 64, :2].numpy() - route.offsets[k]) <= 1).all()
    assert 172 <= iy[63] < 228 and 172 <= iy[64] < 228                      # through the door
    # the definition, called by hand
    dist = R.grid_distance_field(R.routable_cells(tex, R.OBSTACLE_MARGIN, (0, 0, 800, 400)), [(700, 350)])[0]
    found = R.descend_samples(dist, (100, 50), 400)
    want, _ = R.seed_trajectory(tex, lo, hi, found[5], found[0], 400, (0, 0), start, goal, R.OBSTACLE_MARGIN, 16, 5.0 / 64)
    assert np.array_equal(bits(seed.numpy()), bits(want))
    routes, seeds = R.world_routes_seeded("SeedTwoTiles", np.stack([goal, start]), np.stack([start, start]), smooth_iters=0)
    assert [r.tiles.tolist() for r in routes] == [[[1, 0], [0, 0]], [[0, 0]]] and [tuple(s.shape) for s in seeds] == [(128, 4), (64, 4)]
    on_the_spot = np.tile(R.cell_centres(np.asarray((100, 50)), lo, hi, tex.shape), (64, 1))
    on_the_spot[[0, 63]] = start
    assert np.array_equal(seeds[1][:, :2].numpy(), on_the_spot) and not seeds[1][[0, 63], 2:].any() and not seeds[1][2:62, 2:].any()
    # the same refusals as world_routes
    with pytest.raises(ValueError, match="crosses 2 tiles, above max_tiles = 1"):
        R.world_route_seeded("SeedTwoTiles", start, goal, max_tiles=1)
    with pytest.raises(ValueError, match=r"goal cell \[399, 10\] cannot be reached"):
        R.world_route_seeded("SeedTwoTiles", start, M.cell_centre((399, 10), (800, 400)))
    with pytest.raises(ValueError, match="outside the world"):
        R.world_route_seeded("SeedTwoTiles", start, np.asarray([2.5, 0.0], np.float32))
    for bad in (dict(max_tiles=17), dict(max_tiles=0), dict(smooth_iters=-1), dict(trajectory_duration=0.0)):
        with pytest.raises(ValueError, match="world_routes_seeded"):
            R.world_route_seeded("SeedTwoTiles", start, goal, **bad)


def test_route_experience():
    from mmd_amd.planners import PathBatchExperience
    seed = torch.arange(128 * 4, dtype=torch.float32).reshape(128, 4)
    exp = R.route_experience(seed, 5)
    assert isinstance(exp, PathBatchExperience) and exp.path_b.shape == (5, 128, 4) and all(torch.equal(exp.path_b[b], seed) for b in range(5))
    assert R.route_experience(seed.numpy(), 1).path_b.shape == (1, 128, 4)
    for bad, n in ((seed[:100], 5), (seed[:, :2], 5), (seed, 0), (seed[:0], 5)):
        with pytest.raises(ValueError):
            R.route_experience(bad, n)


# ---- the C boundary, without a GPU ----------------------------------------------------------------------------------------------------------------
NAMES = ("mmd_grid_descend_samples", "mmd_route_seeds")


def test_abi_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mmd_amd.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header
    assert "#define MMD_ROUTE_SEED_POINTS 64" in header and "#define MMD_ROUTE_SEED_MAX_TILES 16" in header
    assert (_lib.ROUTE_SEED_POINTS, _lib.ROUTE_SEED_MAX_TILES, R.SEED_POINTS) == (64, 16, 64)
    assert [len(_lib._SIGNATURES[n][1]) for n in NAMES] == [15, 20]
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9
    for name in ("build.sh", "__graft_entry__.py"):
        assert "mmd_amd/csrc/route_seeds.hip" in open(os.path.join(ROOT, name)).read()


def _refused(fn, args, word):
    lib = _lib.load()
    rc = fn(*args)
    msg = lib.mmd_last_error().decode()
    assert rc != 0 and word in msg, (args, rc, msg)


def _with(ok, k, v):
    a = list(ok)
    a[k] = v
    return a


def test_descend_samples_error_returns():
    lib = _lib.load()
    p = C.c_void_p(4096)              # never read: every call below is refused, or has nothing to do
    origin = (C.c_int32 * 2)(0, 0)
    ok = [p, 37, 45, 2, p, p, 5, 16, origin, 4, p, p, p, p, None]
    fn = lib.mmd_grid_descend_samples
    for k, word in ((0, "NULL dist"), (4, "NULL starts"), (5, "NULL field"), (10, "NULL tiles"), (11, "NULL summary"), (12, "NULL visit_cells"),
                    (13, "NULL cells"), (8, "NULL lattice_origin")):
        _refused(fn, _with(ok, k, None), word)
    for k, v, word in ((1, 0, "cells"), (1, 2049, "cells"), (2, 0, "cells"), (2, 2049, "cells"), (3, -1, "n_fields"), (6, -1, "n_queries"),
                       (7, 0, "tile"), (7, -4, "tile"), (9, 0, "max_tiles"), (9, -1, "max_tiles"), (9, 17, "max_tiles"),
                       (8, (C.c_int32 * 2)(2 ** 30 + 1, 0), "lattice_origin"), (8, (C.c_int32 * 2)(0, -2 ** 30 - 1), "lattice_origin")):
        _refused(fn, _with(ok, k, v), word)
    a = _with(ok, 6, 0)                 # no query: nothing to do, whatever the pointers
    for k in (0, 4, 5, 10, 11, 12, 13):
        a[k] = None
    assert fn(*a) == 0


def test_route_seeds_error_returns():
    lib = _lib.load()
    p = C.c_void_p(4096)
    origin = (C.c_int32 * 2)(0, 0)
    lo, hi = (C.c_float * 2)(-1, -1), (C.c_float * 2)(1, 1)
    ok = [p, 37, 45, lo, hi, 0.16, p, p, p, 3, 16, origin, 4, p, p, 8, 0.15, p, p, None]
    fn = lib.mmd_route_seeds
    for k, word in ((0, "NULL grid"), (3, "NULL limits"), (4, "NULL limits"), (6, "NULL cells"), (7, "NULL tiles"), (8, "NULL summary"),
                    (11, "NULL lattice_origin"), (13, "NULL start or goal"), (14, "NULL start or goal"), (17, "NULL seeds"), (18, "NULL clear_min")):
        _refused(fn, _with(ok, k, None), word)
    nan, inf = float("nan"), float("inf")
    for k, v, word in ((1, 0, "cells"), (1, 2049, "cells"), (2, 0, "cells"), (2, 2049, "cells"), (5, nan, "clearance"), (5, inf, "clearance"),
                       (5, -inf, "clearance"), (9, -1, "n_routes"), (10, 0, "tile"), (12, 0, "max_tiles"), (12, 17, "max_tiles"), (12, -3, "max_tiles"),
                       (15, -1, "smooth_iters"), (16, 0.0, "two_dt"), (16, -0.1, "two_dt"), (16, nan, "two_dt"), (16, inf, "two_dt"),
                       (11, (C.c_int32 * 2)(2 ** 30 + 1, 0), "lattice_origin"), (3, (C.c_float * 2)(nan, 0), "limits"),
                       (4, (C.c_float * 2)(-1, 5), "limits"), (4, (C.c_float * 2)(inf, 1), "limits")):
        _refused(fn, _with(ok, k, v), word)
    a = _with(ok, 9, 0)                 # no route: nothing to do, whatever the pointers
    for k in (0, 6, 7, 8, 13, 14, 17, 18):
        a[k] = None
    assert fn(*a) == 0
