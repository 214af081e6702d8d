"""Shared by test_world_routes_host.py and test_gpu_world_routes.py: the test world "doors" with its expected tile lists, the
serpentine, hand-made distance arrays for the descent's rules, and a block-synchronous model of the sweep count."""
import numpy as np

from mmd_amd import world_routes as R

U = R.UNREACHED
BLOCK = 64

# ---- the world "doors": 800 x 800 cells = 2 x 2 tiles.  A wall between the tile columns a = 0 and a = 1 with a door at the top (b = 1),
# and a wall between (0, 0) and (0, 1) with a door.  A clearance of 0.16 closes 32.5 cells on each side of a 120-cell door.
DOORS = "Doors"
DOORS_SHAPE = (800, 800)
DOORS_ROUTES = {          # goal cell -> [(start cell, tiles, or None where the goal cannot be reached)]
    (700, 100): [((100, 100), [(0, 0), (0, 1), (1, 1), (1, 0)]), ((100, 700), [(0, 1), (1, 1), (1, 0)]), ((700, 700), [(1, 1), (1, 0)]),
                 ((399, 0), None)],
    (100, 700): [((100, 100), [(0, 0), (0, 1)]), ((700, 100), [(1, 0), (1, 1), (0, 1)])],
}


def doors_bitmap(j_door_open=True):
    """uint8 [800, 800].  j_door_open=False closes the door between the tile columns: (1, *) is cut off from (0, *)."""
    occ = np.zeros(DOORS_SHAPE, np.uint8)
    occ[398:402, :] = 1
    if j_door_open:
        occ[398:402, 540:660] = 0
    occ[:398, 398:402] = 1
    occ[60:180, 398:402] = 0
    return occ


def cell_centre(cell, shape=DOORS_SHAPE, cell_size=0.005):
    """The global centre of a cell of a world of `shape` registered with the default origin (the world centred on the global origin)."""
    return np.asarray([(cell[k] + 0.5) * cell_size - shape[k] * cell_size / 2.0 for k in range(2)], np.float32)


# ---- textures for the raw kernels: channel 0 is 1 on a free cell and -1 on a blocked one; clearance 0 -------------------------------------
def texture_of(free):
    tex = np.zeros(free.shape + (4,), np.float32)
    tex[..., 0] = np.where(free, np.float32(1), np.float32(-1))
    return tex


def random_free(shape, seed, blocked=0.3):
    return np.random.Generator(np.random.PCG64(seed)).random(shape) >= blocked


def serpentine_free(shape=(130, 70)):
    """Walls on every 4th row (ix = 3, 7, ...) with one gap each, alternating between iy = 0 and iy = ny - 1: one long corridor."""
    free = np.ones(shape, bool)
    for n, ix in enumerate(range(3, shape[0], 4)):
        free[ix, :] = False
        free[ix, 0 if n % 2 == 0 else shape[1] - 1] = True
    return free


SERPENTINE_GOAL = (0, 69)
SERPENTINE_LEVELS = 2407


# ---- hand-made distance arrays for the descent: (dist, start, tile, lattice_origin, max_tiles) -> (tiles, steps, n_tiles, status) -----------
def descent_cases():
    cases = {}
    d = np.full((4, 4), U, np.int32)
    d[0, 0], d[1, 0], d[0, 1] = 2, 1, 1
    d[1, 1] = 0
    cases["direction_order"] = ((d, (0, 0), 4, (0, 0), 4), ([(0, 0)], 2, 1, 0))               # one tile; +x before +y (not observable in tiles)
    d = np.full((4, 4), U, np.int32)
    d[1, 0], d[2, 0], d[1, 1], d[2, 1] = 2, 1, 1, 0
    # tile = 2: (1, 0) is in tile (0, 0); +x (2, 0) is in tile (1, 0), +y (1, 1) is in tile (0, 0): the same-tile candidate wins, then
    # (1, 1) -> +x (2, 1) in tile (1, 0)
    cases["same_tile_preference"] = ((d, (1, 0), 2, (0, 0), 4), ([(0, 0), (1, 0)], 2, 2, 0))
    # the direction order decides between two candidates outside the tile: from (1, 1) with tile = 1 every neighbour is another tile;
    # +x (2, 1) and -x (0, 1) and +y (1, 2) hold d - 1 = 0: +x wins
    d = np.full((3, 3), U, np.int32)
    d[1, 1], d[2, 1], d[0, 1], d[1, 2] = 1, 0, 0, 0
    cases["first_candidate"] = ((d, (1, 1), 1, (0, 0), 4), ([(1, 1), (2, 1)], 1, 2, 0))
    d = np.full((3, 3), U, np.int32)
    d[1, 1], d[0, 1], d[1, 2], d[1, 0] = 1, 0, 0, 0
    cases["minus_x_before_y"] = ((d, (1, 1), 1, (0, 0), 4), ([(1, 1), (0, 1)], 1, 2, 0))
    d = np.full((3, 3), U, np.int32)
    d[1, 1], d[1, 2], d[1, 0] = 1, 0, 0
    cases["plus_y_before_minus_y"] = ((d, (1, 1), 1, (0, 0), 4), ([(1, 1), (1, 2)], 1, 2, 0))
    # a repeated tile: a U-shaped corridor of tile = 2 cells that leaves tile (0, 0), runs through (1, 0) and comes back
    d = np.full((4, 2), U, np.int32)
    d[1, 0], d[2, 0], d[2, 1], d[1, 1], d[0, 1] = 4, 3, 2, 1, 0
    cases["repeated_tile"] = ((d, (1, 0), 2, (0, 0), 4), ([(0, 0), (1, 0), (0, 0)], 4, 3, 0))
    # a shifted lattice origin: cells before the origin have negative tile indices (floor division)
    # with o = (1, 1): (1, 0), (2, 0) -> (0, -1); (2, 1), (1, 1) -> (0, 0); (0, 1) -> (-1, 0)
    cases["shifted_origin"] = ((d, (1, 0), 2, (1, 1), 3), ([(0, -1), (0, 0), (-1, 0)], 4, 3, 0))
    cases["shifted_origin_overflow"] = ((d, (1, 0), 2, (1, 1), 2), ([(0, -1), (0, 0)], 4, 3, 3))
    # status 1: the start holds UNREACHED
    cases["unreached"] = ((d, (0, 0), 2, (0, 0), 4), ([], -1, 0, 1))
    # status 2: the neighbours of the start hold d - 3 (not a converged field): stuck at once, the start's tile alone
    s = np.full((3, 3), U, np.int32)
    s[1, 1], s[2, 1], s[0, 1], s[1, 2], s[1, 0] = 5, 2, 2, 2, 2
    cases["stuck"] = ((s, (1, 1), 1, (0, 0), 4), ([(1, 1)], 0, 1, 2))
    # ... and stuck after one good step
    s2 = np.full((1, 4), U, np.int32)
    s2[0, 0], s2[0, 1], s2[0, 2] = 5, 4, 1
    cases["stuck_later"] = ((s2, (0, 0), 1, (0, 0), 4), ([(0, 0), (0, 1)], 1, 2, 2))
    # status 3: a straight corridor of 6 cells with tile = 1 and max_tiles = 3: 6 tiles needed, 3 returned
    c = np.arange(5, -1, -1, dtype=np.int32).reshape(1, 6)
    cases["too_many_tiles"] = ((c, (0, 0), 1, (0, 0), 3), ([(0, 0), (0, 1), (0, 2)], 5, 6, 3))
    cases["just_enough_tiles"] = ((c, (0, 0), 1, (0, 0), 6), ([(0, k) for k in range(6)], 5, 6, 0))
    # status 4: the start is no cell of the grid
    for k, start in enumerate(((-1, 0), (0, 6), (1, 0), (0, -1))):
        cases[f"outside_{k}"] = ((c, start, 1, (0, 0), 3), ([], -1, 0, 4))
    return cases


def check_descent(got, want):
    tiles, steps, n_tiles, status = got
    assert (np.asarray(tiles).reshape(-1, 2).tolist(), int(steps), int(n_tiles), int(status)) == \
        ([list(t) for t in want[0]], want[1], want[2], want[3])


# ---- the block-synchronous model of the sweeps: what a kernel whose blocks all read the halo of the sweep before would need --------------------
def block_sync_sweeps(free, goal, block=BLOCK):
    """(sweeps, dist): per sweep EVERY block relaxes to its own fixed point against the halo values of the sweep before; `sweeps` counts
    the sweeps run up to and including the first that lowers nothing, the one after which `changed` reads 0.  The kernel's blocks may read
    newer halo values within a sweep, which can only lower the count."""
    nx, ny = free.shape
    dist = np.full((nx + 2, ny + 2), U, np.int64)
    pad = np.zeros((nx + 2, ny + 2), bool)
    pad[1:-1, 1:-1] = free
    if free[goal]:
        dist[goal[0] + 1, goal[1] + 1] = 0
    sweeps = 0
    while True:
        sweeps += 1
        old = dist.copy()
        fell = False
        for i0 in range(0, nx, block):
            for j0 in range(0, ny, block):
                i1, j1 = min(i0 + block, nx), min(j0 + block, ny)
                loc = old[i0:i1 + 2, j0:j1 + 2].copy()
                mask = pad[i0:i1 + 2, j0:j1 + 2].copy()
                mask[0, :] = mask[-1, :] = mask[:, 0] = mask[:, -1] = False               # the halo is read, never relaxed
                while True:
                    m = np.full(loc.shape, U, np.int64)
                    m[1:, :] = np.minimum(m[1:, :], loc[:-1, :])
                    m[:-1, :] = np.minimum(m[:-1, :], loc[1:, :])
                    m[:, 1:] = np.minimum(m[:, 1:], loc[:, :-1])
                    m[:, :-1] = np.minimum(m[:, :-1], loc[:, 1:])
                    new = np.where(mask & (m + 1 < loc), m + 1, loc)
                    if np.array_equal(new, loc):
                        break
                    loc = new
                if not np.array_equal(loc[1:-1, 1:-1], old[i0 + 1:i1 + 1, j0 + 1:j1 + 1]):
                    fell = True
                dist[i0 + 1:i1 + 1, j0 + 1:j1 + 1] = loc[1:-1, 1:-1]
        if not fell:
            return sweeps, np.where(dist[1:-1, 1:-1] >= U, U, dist[1:-1, 1:-1]).astype(np.int32)
