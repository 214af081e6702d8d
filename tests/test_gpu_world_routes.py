"""-m gpu: world routes.  mmd_grid_distance_field and mmd_grid_descend compute the integers of the numpy definitions
(mmd_amd/world_routes.py) -- every comparison here is equality: at the smallest shapes that break a block scheme, on the serpentine whose
values pass through a block many times, within the sweep bound of an open grid, across continued calls, with the clearance at its fp32
edge; the world "doors" routes as tests/world_route_model.py lists, before and after update_world_map closes a door; route_planner is the
hand-built MPDEnsemble bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, environments as E, map_textures, synth, world_routes as R      # noqa: E402
import world_route_model as M                                                            # noqa: E402
from cases import H, D                                                                   # noqa: E402

U = R.UNREACHED
GUARD = 0x7fc00abc                     # a NaN's bits: the guard words behind dist, the workspace, changed, tiles and summary
N_GUARD = 64
SHAPES = ((1, 1), (64, 64), (65, 129), (130, 70))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    worlds = set(E.registered_world_maps())
    yield
    for name in set(E.registered_world_maps()) - worlds:
        E.unregister_world_map(name)


def guarded(n_words):
    """an int32 device buffer of n_words garbage words and N_GUARD guard words behind them"""
    t = torch.full((n_words + N_GUARD,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    t[n_words:] = GUARD
    return t


def guard_intact(t, n_words):
    return bool((t[n_words:] == GUARD).all()) and t.numel() == n_words + N_GUARD


class RawField:
    """mmd_grid_distance_field on a host texture [nx, ny, 4], called as the header says: guarded dist, workspace and changed buffers that live
    as long as the object, so that restart = 0 continues where the last call stopped."""

    def __init__(self, tex, goals, clearance=0.0, region=None):
        self.tex = torch.from_numpy(np.ascontiguousarray(tex, dtype=np.float32)).cuda()
        self.nx, self.ny = tex.shape[:2]
        self.goals = torch.tensor(np.asarray(goals).reshape(-1, 2), dtype=torch.int32, device="cuda")
        self.n = self.goals.shape[0]
        self.clearance = float(clearance)
        self.region = (C.c_int32 * 4)(*((0, 0, self.nx, self.ny) if region is None else region))
        self.work_bytes = int(_lib.load().mmd_grid_distance_work_bytes(self.nx, self.ny, self.n))
        assert self.work_bytes == 4 * self.n * (1 + (-(-self.nx // 64)) * (-(-self.ny // 64)))
        self.dist, self.work, self.changed = guarded(self.n * self.nx * self.ny), guarded(self.work_bytes // 4), guarded(self.n)
        self.sweeps = 0

    def call(self, restart, n_sweeps):
        """-> changed [n_fields] on the host"""
        _lib.launch("mmd_grid_distance_field", self.tex, C.c_void_p(self.tex.data_ptr()), self.nx, self.ny, self.clearance, self.region,
                    C.c_void_p(self.goals.data_ptr()), self.n, int(restart), int(n_sweeps), C.c_void_p(self.dist.data_ptr()),
                    C.c_void_p(self.work.data_ptr()), self.work_bytes, C.c_void_p(self.changed.data_ptr()))
        self.sweeps = n_sweeps if restart else self.sweeps + n_sweeps
        return self.changed[:self.n].cpu().numpy()

    def converge(self, per_call, bound):
        changed = self.call(1, per_call)
        while changed.any():
            assert self.sweeps < bound, f"not converged after {self.sweeps} sweeps: changed = {changed.tolist()}"
            changed = self.call(0, per_call)
        return self.field()

    def field(self):
        return self.dist[:self.n * self.nx * self.ny].cpu().numpy().reshape(self.n, self.nx, self.ny)

    def guards_intact(self):
        return guard_intact(self.dist, self.n * self.nx * self.ny) and guard_intact(self.work, self.work_bytes // 4) and \
            guard_intact(self.changed, self.n)


def goals_of(shape):
    """a block corner, a block edge (the first row of the second block, where there is one) and an interior cell"""
    nx, ny = shape
    return [(0, 0), (min(64, nx - 1), min(30, ny - 1)), (nx // 2, (2 * ny) // 3)]


def cut_region(shape):
    """a region that cuts through the blocks (the whole grid for 1 x 1)"""
    nx, ny = shape
    return (0, 0, 1, 1) if shape == (1, 1) else (3, 5, nx - 2, ny - 7)


def free_cells(shape, kind):
    if kind == "open":
        return np.ones(shape, bool)
    free = M.random_free(shape, seed=11 + shape[0])
    for g in goals_of(shape):
        free[g] = True
    return free


_REFERENCE = {}


def reference(shape, kind, region):
    """The definition's fields for (shape, kind, region), computed once and read-only"""
    key = (shape, kind, region)
    if key not in _REFERENCE:
        free = free_cells(shape, kind)
        ref = R.grid_distance_field(R.routable_cells(M.texture_of(free), 0.0, region), goals_of(shape))
        ref.setflags(write=False)
        _REFERENCE[key] = (free, ref)
    return _REFERENCE[key]


# ---- 1. the raw field is the definition, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", (False, True), ids=("whole", "cut"))
@pytest.mark.parametrize("kind", ("random", "open"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raw_field_equals_the_definition(shape, kind, cut):
    region = cut_region(shape) if cut else (0, 0) + shape
    free, ref = reference(shape, kind, region)
    raw = RawField(M.texture_of(free), goals_of(shape), 0.0, region)
    assert raw.n == 3
    bound = int(R.routable_cells(M.texture_of(free), 0.0, region).sum()) + 2
    got = raw.converge(4, bound)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    if kind == "open" and not cut and shape != (1, 1):
        assert (got != U).all() and got[0].max() == shape[0] + shape[1] - 2
    if cut and shape != (1, 1):
        assert (got[0] == U).all() and (got[2] != U).sum() > 1             # goal (0, 0) lies outside the region: nothing is seeded
    assert raw.guards_intact()
    first = got.copy()
    assert np.array_equal(raw.converge(4, bound), first)                       # a second run, on the used buffers: the same bits
    assert raw.guards_intact()
    # the wrapper: the same integers, within its own bound
    dist, sweeps = R.device_distance_field(raw.tex, goals_of(shape), 0.0, region, sweeps_per_call=3)
    assert np.array_equal(dist.cpu().numpy(), ref) and 3 <= sweeps <= bound + 2


def test_goals_that_seed_nothing():
    """A goal outside the grid, on a blocked cell or on a NaN texel gives a field that is UNREACHED everywhere and reports converged at once"""
    free = np.ones((65, 70), bool)
    free[10, 10] = False
    tex = M.texture_of(free)
    tex[20, 20, 0] = np.nan
    goals = [(-1, 0), (65, 0), (0, 70), (0, -5), (10, 10), (20, 20), (2 ** 31 - 1, -2 ** 31), (64, 69)]
    raw = RawField(tex, goals)
    assert raw.call(1, 0).tolist() == [0] * 7 + [1]                            # after a restart alone: the seeded goal's block is flagged
    changed = raw.call(1, 1)
    assert changed[:7].tolist() == [0] * 7
    got = raw.converge(2, 65 * 70)
    assert (got[:7] == U).all() and got[7, 64, 69] == 0 and got[7, 20, 20] == U and got[7, 10, 10] == U and (got[7] != U).sum() == 65 * 70 - 2
    assert np.array_equal(got, R.grid_distance_field(R.routable_cells(tex, 0.0), goals)) and raw.guards_intact()


# ---- 2. the serpentine: values pass through a block many times -------------------------------------------------------------------------------------
def test_serpentine_flags_and_fields_do_not_leak():
    free = M.serpentine_free()
    ref = R.grid_distance_field(free, [M.SERPENTINE_GOAL])[0]
    assert int(ref[ref != U].max()) + 1 == M.SERPENTINE_LEVELS
    # a call has one texture: the serpentine and an open field stand side by side in one (130, 141) grid with a blocked seam column between
    # them, so the serpentine keeps the (130, 70) block geometry (3 x 2 blocks; the seam lies in its second block column)
    both = np.zeros((130, 141), bool)
    both[:, :70] = free
    both[:, 71:] = True
    goals = [M.SERPENTINE_GOAL, (0, 71)]
    want = R.grid_distance_field(both, goals)
    assert np.array_equal(want[0][:, :70], ref) and (want[0][:, 70:] == U).all() and (want[1][:, :71] == U).all()
    raw = RawField(M.texture_of(both), goals)
    open_done = None
    changed = raw.call(1, 1)
    while changed.any():
        assert raw.sweeps < 37, f"the block-synchronous model needs 37 sweeps; changed = {changed.tolist()} after {raw.sweeps}"
        if changed[1] == 0 and open_done is None:
            open_done = raw.sweeps
            assert np.array_equal(raw.field()[1], want[1])
        if open_done is not None:
            assert changed[1] == 0                                             # a converged field stays quiet while the other one runs
        changed = raw.call(0, 1)
    # `changed == 0` is never reported before the field is the definition's
    assert np.array_equal(raw.field(), want) and raw.guards_intact()
    assert open_done is not None and open_done <= 3 + 2 and raw.sweeps > open_done
    # on its own (130, 70) grid: the first `changed == 0` comes within 37 sweeps and not before the field is the definition's
    alone = RawField(M.texture_of(free), [M.SERPENTINE_GOAL])
    changed = alone.call(1, 1)
    while changed.any():
        assert alone.sweeps < 37
        changed = alone.call(0, 1)
    assert np.array_equal(alone.field()[0], ref) and alone.guards_intact()


# ---- 3. the sweep bound of an open grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_open_grid_sweep_bound(shape):
    bx, by = -(-shape[0] // 64), -(-shape[1] // 64)
    raw = RawField(M.texture_of(np.ones(shape, bool)), [(0, 0)])
    changed = raw.call(1, 1)
    while changed.any():
        assert raw.sweeps < bx + by, f"changed = {changed.tolist()} after {raw.sweeps} sweeps, bound {bx + by}"
        changed = raw.call(0, 1)
    assert raw.sweeps <= bx + by
    ix, iy = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    assert np.array_equal(raw.field()[0], ix + iy) and raw.guards_intact()


# ---- 4. continuation -------------------------------------------------------------------------------------------------------------------------------------
def test_continued_calls_equal_one_long_call():
    free = M.serpentine_free()
    tex = M.texture_of(free)
    goals = [M.SERPENTINE_GOAL, (129, 0)]
    want = R.grid_distance_field(free, goals)
    long = RawField(tex, goals)
    long_changed = long.call(1, 40)
    split = RawField(tex, goals)
    split.call(1, 2)
    assert not np.array_equal(split.field(), want)                             # two sweeps are not enough: the continuation has work to do
    for k in (3, 1, 0, 30, 4):
        split_changed = split.call(0, k)
    assert split.sweeps == 40 and long_changed.tolist() == [0, 0] and split_changed.tolist() == [0, 0]
    assert np.array_equal(long.field(), want) and np.array_equal(split.field(), long.field())
    work = split.work.clone()
    assert split.call(0, 5).tolist() == [0, 0] and np.array_equal(split.field(), want)        # converged: further sweeps change nothing
    assert torch.equal(split.work[2:], work[2:]) and split.work[:2].tolist() == [45, 45]      # (but the sweep counts)
    assert long.guards_intact() and split.guards_intact()


# ---- 5. the clearance at its edge ----------------------------------------------------------------------------------------------------------------------
def test_clearance_is_a_strict_fp32_compare_on_a_built_texture():
    n = 21
    occ = np.zeros((n, n), np.uint8)
    occ[10, 10] = 1
    tex_dev = torch.empty(n, n, 4, dtype=torch.float32, device="cuda")
    E._occupancy_build(torch.from_numpy(occ).cuda(), tex_dev)
    tex = tex_dev.cpu().numpy()
    assert np.array_equal(tex.view(np.uint32), E.occupancy_sdf_texture(occ).view(np.uint32))
    ix, iy = np.meshgrid(np.arange(n) - 10, np.arange(n) - 10, indexing="ij")
    d2 = ix * ix + iy * iy
    at25 = np.unique(tex[..., 0][d2 == 25])
    assert at25.size == 1 and (d2 == 25).sum() == 12 and (d2 == 26).sum() == 8
    clearance = float(at25[0])                                                 # exactly the value of the cells at D2 = 25
    tex[2, 3, 0] = np.nan                                                      # (D2 = 113: routable but for the NaN)
    rt = R.routable_cells(tex, clearance)
    assert not rt[d2 <= 25].any() and rt[d2 == 26].all() and not rt[2, 3] and rt[(d2 > 25)].sum() == (d2 > 25).sum() - 1
    goals = [(15, 11), (15, 10), (0, 0)]                                        # D2 = 26, D2 = 25 (blocked), a corner
    want = R.grid_distance_field(rt, goals)
    raw = RawField(tex, goals, clearance)
    got = raw.converge(2, n * n)
    assert np.array_equal(got, want) and raw.guards_intact()
    assert (got[1] == U).all() and (got[0][d2 <= 25] == U).all() and (got[0][d2 == 26] != U).all() and got[0][2, 3] == U
    assert got[0][15, 9] == 2 + 2                                               # round the blocked (15, 10): not straight through it
    # one ulp up, the D2 = 26 ring stays; one ulp down, the D2 = 25 cells open
    down = RawField(tex, goals, float(np.nextafter(at25[0], np.float32(0)))).converge(2, n * n)
    assert (down[1] != U).sum() > 12 and down[0][15, 9] == 2 and (down[0][d2 == 25] != U).all() and (down[0][d2 < 25] == U).all()


# ---- 6. the raw descent is the definition -----------------------------------------------------------------------------------------------------------------
def raw_descend(dist, starts, fields, tile, origin, max_tiles):
    """mmd_grid_descend on host fields [n_fields, nx, ny] -> (tiles [n, max_tiles, 2] with untouched rows = GUARD, summary [n, 4]), guards checked"""
    dist = np.array(dist, dtype=np.int32)                     # (a writable copy: the shared references are read-only)
    n = len(starts)
    dist_dev = torch.from_numpy(dist).cuda()
    starts_dev = torch.tensor(np.asarray(starts).reshape(-1, 2), dtype=torch.int32, device="cuda")
    fields_dev = torch.tensor(np.asarray(fields).reshape(-1), dtype=torch.int32, device="cuda")
    tiles, summary = guarded(n * max_tiles * 2), guarded(n * 4)
    tiles[:n * max_tiles * 2] = GUARD
    _lib.launch("mmd_grid_descend", dist_dev, C.c_void_p(dist_dev.data_ptr()), dist.shape[1], dist.shape[2], dist.shape[0],
                C.c_void_p(starts_dev.data_ptr()), C.c_void_p(fields_dev.data_ptr()), n, tile, (C.c_int32 * 2)(*origin), max_tiles,
                C.c_void_p(tiles.data_ptr()), C.c_void_p(summary.data_ptr()))
    torch.cuda.synchronize()
    assert guard_intact(tiles, n * max_tiles * 2) and guard_intact(summary, n * 4)
    return tiles[:n * max_tiles * 2].cpu().numpy().reshape(n, max_tiles, 2), summary[:n * 4].cpu().numpy().reshape(n, 4)


def check_raw_descent(dist, starts, fields, tile, origin, max_tiles):
    tiles, summary = raw_descend(dist, starts, fields, tile, origin, max_tiles)
    statuses = set()
    for q, (start, f) in enumerate(zip(starts, fields)):
        if 0 <= f < dist.shape[0]:
            want_tiles, steps, n_tiles, status = R.descend(dist[f], start, tile, origin, max_tiles)
        else:
            want_tiles, steps, n_tiles, status = np.zeros((0, 2), np.int32), -1, 0, R.ROUTE_OUTSIDE
        assert summary[q].tolist() == [steps, n_tiles, status, 0], (q, start, f)
        k = len(want_tiles)
        assert k == min(n_tiles, max_tiles) and np.array_equal(tiles[q, :k], want_tiles), (q, start, f)
        assert (tiles[q, k:] == GUARD).all(), (q, start, f)                   # nothing is written behind a query's tiles
        statuses.add(status)
    return statuses


def test_raw_descent_on_the_fields():
    rng = np.random.Generator(np.random.PCG64(5))
    seen = set()
    for shape, kind in (((65, 129), "random"), ((130, 70), "open")):
        _, ref = reference(shape, kind, (0, 0) + shape)
        starts = np.stack([rng.integers(-2, shape[0] + 2, 200), rng.integers(-2, shape[1] + 2, 200)], axis=1).tolist()
        fields = rng.integers(-1, 4, 200).tolist()
        seen |= check_raw_descent(ref, starts, fields, 16, (5, 9), 8)
        seen |= check_raw_descent(ref, starts, fields, 16, (5, 9), 40)
    assert seen == {R.ROUTE_OK, R.ROUTE_UNREACHED, R.ROUTE_TOO_MANY_TILES, R.ROUTE_OUTSIDE}
    free = M.serpentine_free()
    ref = R.grid_distance_field(free, [M.SERPENTINE_GOAL])
    starts = [(129, 0), (128, 69), (64, 35), (3, 0), (0, 69), (3, 5)]
    assert check_raw_descent(ref, starts, [0] * 6, 16, (0, 0), 256) == {R.ROUTE_OK, R.ROUTE_UNREACHED}
    assert check_raw_descent(ref, starts, [0] * 6, 16, (3, 2), 256) == {R.ROUTE_OK, R.ROUTE_UNREACHED}          # a shifted lattice
    tiles, summary = raw_descend(ref, starts[:1], [0], 16, (0, 0), 256)
    assert summary[0, 0] == ref[0, 129, 0] and summary[0, 1] > 9 * 5                     # the corridor crosses every tile column again and again


@pytest.mark.parametrize("case", sorted(M.descent_cases()))
def test_raw_descent_rules(case):
    (dist, start, tile, origin, max_tiles), want = M.descent_cases()[case]
    tiles, summary = raw_descend(dist[None], [start], [0], tile, origin, max_tiles)
    k = min(int(summary[0, 1]), max_tiles)
    M.check_descent((tiles[0, :k], summary[0, 0], summary[0, 1], summary[0, 2]), want)
    assert summary[0, 3] == 0 and (tiles[0, k:] == GUARD).all()
    wt, ws = R.device_descend(torch.from_numpy(np.ascontiguousarray(dist[None])).cuda(), [start], [0], tile, origin, max_tiles)
    assert np.array_equal(ws.cpu().numpy(), summary) and np.array_equal(wt.cpu().numpy()[0, :k], tiles[0, :k]) and not wt[0, k:].any()


# ---- 7. the world "doors" on the device ----------------------------------------------------------------------------------------------------------------------
def test_world_doors_routes_and_update(registry):
    E.register_world_map(M.DOORS, M.doors_bitmap())
    queries = [(start, goal, tiles) for goal, rows in M.DOORS_ROUTES.items() for start, tiles in rows]
    good = [q for q in queries if q[2] is not None]
    assert len(good) == 5 and len(queries) == 6
    starts = np.stack([M.cell_centre(q[0]) for q in good])
    goals = np.stack([M.cell_centre(q[1]) for q in good])
    assert R.world_cells(M.DOORS, starts).tolist() == [list(q[0]) for q in good]
    routes = R.world_routes(M.DOORS, starts, goals, device="cuda")
    tex = map_textures.device_world_texture(M.DOORS, "cuda").cpu().numpy()
    rt = R.routable_cells(tex, R.OBSTACLE_MARGIN, R.world_lattice(M.DOORS)[0])
    ref = {goal: R.grid_distance_field(rt, [goal])[0] for goal in M.DOORS_ROUTES}
    for (start, goal, tiles), route in zip(good, routes):
        assert route.tiles.tolist() == [list(t) for t in tiles], (start, goal)
        assert route.steps == int(ref[goal][start]) and route.steps != U, (start, goal)
        assert route.origins.tolist() == [[400 * a, 400 * b] for a, b in tiles]
        assert route.env_ids == [f"{M.DOORS}@{400 * a},{400 * b}" for a, b in tiles]
        steps = np.abs(np.diff(route.offsets, axis=0))
        assert np.array_equal(np.sort(steps, axis=1), np.tile(np.float32([0.0, 2.0]), (len(tiles) - 1, 1)))      # neighbours share an edge
    # the sixth: a start inside the wall
    with pytest.raises(ValueError, match=r"goal cell \[700, 100\] cannot be reached from the start cell \[399, 0\]"):
        R.world_route(M.DOORS, M.cell_centre((399, 0)), M.cell_centre((700, 100)), device="cuda")
    # the whole field of one goal on the resident texture is the definition's
    wtex = map_textures.device_world_texture(M.DOORS, "cuda")
    dist, sweeps = R.device_distance_field(wtex, [(700, 100)], R.OBSTACLE_MARGIN, (0, 0, 800, 800))
    assert np.array_equal(dist[0].cpu().numpy(), ref[(700, 100)]) and sweeps >= 1
    # close the door between the tile columns: the resident texture is rebuilt in place and the next routing sees it
    E.update_world_map(M.DOORS, M.doors_bitmap(j_door_open=False))
    assert map_textures.device_world_texture(M.DOORS, "cuda").data_ptr() == wtex.data_ptr()
    for start in ((100, 100), (100, 700)):
        with pytest.raises(ValueError, match=r"goal cell \[700, 100\] cannot be reached"):
            R.world_route(M.DOORS, M.cell_centre(start), M.cell_centre((700, 100)), device="cuda")
    # (cell (700, 700) lies on the goal's side of that wall: no obstacle stands between the tiles (1, 1) and (1, 0), so it still routes)
    assert R.world_route(M.DOORS, M.cell_centre((700, 700)), M.cell_centre((700, 100)), device="cuda").tiles.tolist() == [[1, 1], [1, 0]]
    assert R.world_route(M.DOORS, M.cell_centre((100, 100)), M.cell_centre((100, 700)), device="cuda").tiles.tolist() == [[0, 0], [0, 1]]


# ---- 8. the planner ------------------------------------------------------------------------------------------------------------------------------------
def test_route_planner_is_the_hand_built_ensemble(registry):
    from mmd_amd.planners import MPDEnsemble
    E.register_world_map(M.DOORS, M.doors_bitmap())
    start, goal = torch.from_numpy(M.cell_centre((100, 700))), torch.from_numpy(M.cell_centre((700, 100)))
    route = R.world_route(M.DOORS, start, goal, device="cuda")
    assert route.tiles.tolist() == [[0, 1], [1, 1], [1, 0]]
    sd = synth.synth_unet_state_dict(0)
    kw = dict(planner_alg="mmd", device="cuda", seed=23, n_samples=8, model_state_dicts=[sd] * 3, model_args=dict(n_diffusion_steps=25),
              trained_models_dir="")
    p = R.route_planner(route, "EnvHighways2D-RobotPlanarDisk", start, goal, **kw)
    assert isinstance(p, MPDEnsemble) and [p.env_ids[k] for k in range(3)] == route.env_ids
    res = p(start, goal, seed=77)
    assert res.trajs_final.shape == (8, 3 * H, D) and torch.isfinite(res.trajs_final).all()
    by_hand = MPDEnsemble(model_ids=("EnvHighways2D-RobotPlanarDisk",) * 3,
                          transforms={0: torch.tensor([-1.0, 1.0]), 1: torch.tensor([1.0, 1.0]), 2: torch.tensor([1.0, -1.0])},
                          env_ids=[f"{M.DOORS}@0,400", f"{M.DOORS}@400,400", f"{M.DOORS}@400,0"], start_state_pos=start, goal_state_pos=goal,
                          **kw)
    assert torch.equal(by_hand(start, goal, seed=77).trajs_final, res.trajs_final)
