"""-m gpu: the seed trajectories of world routes.  mmd_grid_descend_samples and mmd_route_seeds compute the integers and the float32 bits of
the numpy definitions (mmd_amd/world_routes.py: descend_samples, seed_trajectory) -- every comparison here is equality, floats by their
int32 views: on raw grids with more than one block of queries, K = 1, 2 and max_tiles, visits of one cell and of more cells than samples,
odd and even iteration counts, the clearance and the lattice line at their edges, bad queries next to good ones, guard words behind every
buffer; then the world "SeedDoors" end to end, before and after update_world_map closes a door, and the planner call on the seed."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, environments as E, synth, world_routes as R      # noqa: E402
import route_seed_model as M                                               # noqa: E402

GUARD = 0x7fc00abc                     # a NaN's bits: the guard words behind every output buffer
N_GUARD = 64
P = 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


@pytest.fixture
def registry():
    worlds = set(E.registered_world_maps())
    yield
    for name in set(E.registered_world_maps()) - worlds:
        E.unregister_world_map(name)


def guarded(n_words, fill=0x5a5a5a5a):
    """an int32 device buffer of n_words words of `fill` and N_GUARD guard words behind them"""
    t = torch.full((n_words + N_GUARD,), fill, dtype=torch.int32, device="cuda")
    t[n_words:] = GUARD
    return t


def guard_intact(t, n_words):
    return bool((t[n_words:] == GUARD).all()) and t.numel() == n_words + N_GUARD


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class Raw:
    """The two entry points called as the header says, on guarded buffers that live as long as the object (a second call writes the same ones)."""

    def __init__(self, dist, starts, fields, tile, origin, max_tiles):
        self.dist = dev(np.array(dist, np.int32), np.int32)
        self.n, self.tile, self.origin, self.mt = len(starts), tile, (C.c_int32 * 2)(*origin), max_tiles
        self.starts, self.fields = dev(np.asarray(starts).reshape(-1, 2), np.int32), dev(np.asarray(fields).reshape(-1), np.int32)
        n, mt = self.n, max_tiles
        self.sizes = dict(tiles=n * mt * 2, summary=n * 4, visit_cells=n * mt, cells=n * mt * P * 2, seeds=n * mt * P * 4, clear_min=n)
        self.buf = {k: guarded(v) for k, v in self.sizes.items()}
        self.buf["tiles"][:self.sizes["tiles"]] = GUARD                      # (rows of tiles behind n_tiles are not written)

    def ptr(self, k):
        return C.c_void_p(self.buf[k].data_ptr())

    def host(self, k, shape):
        return self.buf[k][:self.sizes[k]].cpu().numpy().reshape(shape)

    def guards_intact(self):
        return all(guard_intact(self.buf[k], v) for k, v in self.sizes.items())

    def samples(self):
        """-> tiles [n, mt, 2], summary [n, 4], visit_cells [n, mt], cells [n, mt, 64, 2]"""
        d = self.dist
        _lib.launch("mmd_grid_descend_samples", d, C.c_void_p(d.data_ptr()), d.shape[1], d.shape[2], d.shape[0], C.c_void_p(self.starts.data_ptr()),
                    C.c_void_p(self.fields.data_ptr()), self.n, self.tile, self.origin, self.mt, self.ptr("tiles"), self.ptr("summary"),
                    self.ptr("visit_cells"), self.ptr("cells"))
        torch.cuda.synchronize()
        n, mt = self.n, self.mt
        return self.host("tiles", (n, mt, 2)), self.host("summary", (n, 4)), self.host("visit_cells", (n, mt)), self.host("cells", (n, mt, P, 2))

    def seeds(self, tex, lo, hi, clearance, start_points, goal_points, smooth_iters, dt, cells=None, tiles=None, summary=None):
        """-> seeds [n, mt * 64, 4], clear_min [n]; from the buffers samples() left, or from the given host arrays"""
        tex_dev = dev(tex, np.float32)
        given = [None if a is None else dev(a, np.int32) for a in (cells, tiles, summary)]
        p = [self.ptr(k) if g is None else C.c_void_p(g.data_ptr()) for k, g in zip(("cells", "tiles", "summary"), given)]
        s, g = dev(np.asarray(start_points).reshape(-1, 2), np.float32), dev(np.asarray(goal_points).reshape(-1, 2), np.float32)
        _lib.launch("mmd_route_seeds", tex_dev, C.c_void_p(tex_dev.data_ptr()), tex.shape[0], tex.shape[1], (C.c_float * 2)(*lo), (C.c_float * 2)(*hi),
                    float(clearance), p[0], p[1], p[2], self.n, self.tile, self.origin, self.mt, C.c_void_p(s.data_ptr()), C.c_void_p(g.data_ptr()),
                    int(smooth_iters), float(np.float32(2.0 * dt)), self.ptr("seeds"), self.ptr("clear_min"))
        torch.cuda.synchronize()
        return self.host("seeds", (self.n, self.mt * P, 4)).view(np.float32), self.host("clear_min", (self.n,)).view(np.float32)


def definition(dist, starts, fields, tile, origin, max_tiles):
    """[descend_samples(...)] per query; a field index outside the fields counts as a start outside the grid"""
    none = (np.zeros((0, 2), np.int32), -1, 0, R.ROUTE_OUTSIDE, np.zeros(0, np.int32), np.zeros((0, P, 2), np.int32))
    return [R.descend_samples(dist[f], s, tile, origin, max_tiles) if 0 <= f < len(dist) else none for s, f in zip(starts, fields)]


def check_samples(got, want, max_tiles):
    tiles, summary, visit_cells, cells = got
    for q, w in enumerate(want):
        assert summary[q].tolist() == [w[1], w[2], w[3], 0], q
        k = len(w[0])
        assert k == min(w[2], max_tiles) and np.array_equal(tiles[q, :k], w[0]) and (tiles[q, k:] == GUARD).all(), q
        vc, padded = M.padded(w, max_tiles)
        assert np.array_equal(visit_cells[q], vc) and np.array_equal(cells[q], padded), q


def check_seeds(got, want_samples, tex, lo, hi, tile, origin, start_points, goal_points, clearance, smooth_iters, dt, max_tiles):
    seeds, clear_min = got
    for q, w in enumerate(want_samples):
        seed, cmin = R.seed_trajectory(tex, lo, hi, w[5], w[0][:len(w[5])], tile, origin, start_points[q], goal_points[q], clearance, smooth_iters, dt)
        n = len(seed)
        assert n == (P * w[2] if w[3] == R.ROUTE_OK else 0), q
        assert np.array_equal(bits(seeds[q, :n]), bits(seed)), (q, smooth_iters)
        assert not bits(seeds[q, n:]).any() and bits(clear_min[q]) == bits(cmin), (q, smooth_iters)


LO, HI = (-1.2, -1.0), (1.2, 1.0)


def centres(cells, shape):
    return R.cell_centres(np.asarray(cells), LO, HI, shape)


# ---- 1. raw grids: samples and seeds are the definition's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("door", "door_shifted", "serpentine", "L"))
def test_samples_and_seeds_on_grids(name):
    free, goal, tile, origin, starts = M.grids()[name]                       # 96 x 80 and 130 x 70 cells, tile = 32
    dist = M.field_of(free, goal)[None]
    tex = M.texture_of(free)
    max_tiles = 16
    if name == "serpentine":
        starts = [M.start_with_tiles(dist[0], tile, origin, k) for k in (16, 1, 2, 17)] + list(starts)          # K = max_tiles, 1, 2; one too many
    starts = list(starts) + [goal, (-1, 0), (0, 3) if not free[0, 3] else (3, 0)]
    fields = [0] * len(starts)
    want = definition(dist, starts, fields, tile, origin, max_tiles)
    raw = Raw(dist, starts, fields, tile, origin, max_tiles)
    got = raw.samples()
    check_samples(got, want, max_tiles)
    assert raw.guards_intact()
    if name == "serpentine":
        assert [w[2] for w in want[:4]] == [16, 1, 2, 17] and [w[3] for w in want[:4]] == [0, 0, 0, R.ROUTE_TOO_MANY_TILES]
        assert max(int(w[4].max()) for w in want if len(w[4])) > 64         # a visit of more cells than samples
    s_pts, g_pts = centres(starts, tex.shape) + np.float32(0.003), np.tile(centres(goal, tex.shape), (len(starts), 1))
    for iters in (0, 1, 2, 33):
        check_seeds(raw.seeds(tex, LO, HI, 0.0, s_pts, g_pts, iters, 5.0 / 64), want, tex, LO, HI, tile, origin, s_pts, g_pts, 0.0, iters, 5.0 / 64,
                    max_tiles)
        assert raw.guards_intact()
    # a second call of both into the used buffers: the same bits
    first = [a.copy() for a in got] + [a.copy() for a in raw.seeds(tex, LO, HI, 0.0, s_pts, g_pts, 33, 5.0 / 64)]
    again = list(raw.samples()) + list(raw.seeds(tex, LO, HI, 0.0, s_pts, g_pts, 33, 5.0 / 64))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, again)) and raw.guards_intact()


def test_visits_of_one_cell_and_max_tiles_one():
    g = M.grids()
    free, goal, tile, origin, starts = g["clipped_corner"]
    dist = M.field_of(free, goal)[None]
    raw = Raw(dist, starts, [0], tile, origin, 3)
    want = definition(dist, starts, [0], tile, origin, 3)
    got = raw.samples()
    check_samples(got, want, 3)
    assert got[2][0].tolist() == [2, 1, 2] and (got[3][0, 1] == (2, 1)).all()
    tex = M.texture_of(free)
    pts = R.cell_centres(np.asarray([starts[0], goal]), (0, 0), (4, 4), (4, 4))
    for iters in (0, 1, 2, 33):
        check_seeds(raw.seeds(tex, (0, 0), (4, 4), 0.0, pts[:1], pts[1:], iters, 0.5), want, tex, (0, 0), (4, 4), tile, origin, pts[:1], pts[1:], 0.0,
                    iters, 0.5, 3)
    # max_tiles = 1: a route of one tile passes, one of two is status 3 with zero rows
    free, goal, tile, origin, _ = g["corridor_long_visit"]
    dist = M.field_of(free, goal)[None]
    starts = [(1, 120), (1, 35), (1, 199)]
    want = definition(dist, starts, [0] * 3, tile, origin, 1)
    raw = Raw(dist, starts, [0] * 3, tile, origin, 1)
    check_samples(raw.samples(), want, 1)
    assert [w[3] for w in want] == [0, 3, 0] and [w[4].tolist() for w in want] == [[80], [], [1]]
    tex = M.texture_of(free)
    s_pts, g_pts = R.cell_centres(np.asarray(starts), (0, 0), (3, 200), (3, 200)), R.cell_centres(np.asarray([goal] * 3), (0, 0), (3, 200), (3, 200))
    for iters in (0, 2, 33):
        check_seeds(raw.seeds(tex, (0, 0), (3, 200), 0.0, s_pts, g_pts, iters, 0.5), want, tex, (0, 0), (3, 200), tile, origin, s_pts, g_pts, 0.0, iters,
                    0.5, 1)
    assert raw.guards_intact()


# ---- 2. a batch: more queries than one workgroup of the descent, every status, several fields ----------------------------------------------------------
def test_a_batch_of_65_queries_with_every_status():
    free, goal, tile, origin, _ = M.grids()["door"]
    goals = [goal, (5, 5)]
    dist = R.grid_distance_field(free, goals)
    rng = np.random.Generator(np.random.PCG64(9))
    starts = np.stack([rng.integers(-1, 97, 65), rng.integers(-1, 81, 65)], axis=1).tolist()
    fields = rng.integers(0, 2, 65).tolist()
    starts[1], fields[1] = (48, 10), 0                                        # in the wall: status 1, between two good queries
    starts[2], fields[2] = (3, 5), 0
    starts[3], fields[3] = (3, 5), 2                                          # no such field: status 4
    starts[64], fields[64] = (20, 20), 1                                      # the second workgroup's only query
    max_tiles = 3                                                             # (3, 5) -> (90, 5) crosses more: status 3
    want = definition(dist, starts, fields, tile, origin, max_tiles)
    assert {w[3] for w in want} == {0, 1, 3, 4} and [want[k][3] for k in (1, 2, 3)] == [1, 3, 4] and want[64][3] == 0
    raw = Raw(dist, starts, fields, tile, origin, max_tiles)
    got = raw.samples()
    check_samples(got, want, max_tiles)
    # tiles and summary are mmd_grid_descend's on the same inputs, word for word (untouched words included)
    tiles, summary = guarded(65 * max_tiles * 2, GUARD), guarded(65 * 4)
    _lib.launch("mmd_grid_descend", raw.dist, C.c_void_p(raw.dist.data_ptr()), 96, 80, 2, C.c_void_p(raw.starts.data_ptr()),
                C.c_void_p(raw.fields.data_ptr()), 65, tile, raw.origin, max_tiles, C.c_void_p(tiles.data_ptr()), C.c_void_p(summary.data_ptr()))
    assert torch.equal(tiles, raw.buf["tiles"]) and torch.equal(summary, raw.buf["summary"])
    tex = M.texture_of(free)
    s_pts = centres(np.clip(starts, 0, (95, 79)), tex.shape)
    g_pts = centres([goals[min(f, 1)] for f in fields], tex.shape)
    for iters in (0, 1, 33):
        seeds, clear_min = raw.seeds(tex, LO, HI, 0.0, s_pts, g_pts, iters, 5.0 / 64)
        check_seeds((seeds, clear_min), want, tex, LO, HI, tile, origin, s_pts, g_pts, 0.0, iters, 5.0 / 64, max_tiles)
        for q in (1, 2, 3):                                                   # zero rows, and no leak into the neighbours' rows
            assert not bits(seeds[q]).any() and bits(clear_min[q]) == 0
    assert raw.guards_intact()
    # the wrappers: the same words
    wt, ws, wv, wc = R.device_descend_samples(raw.dist, starts, fields, tile, origin, max_tiles)
    assert np.array_equal(ws.cpu().numpy(), got[1]) and np.array_equal(wv.cpu().numpy(), got[2]) and np.array_equal(wc.cpu().numpy(), got[3])
    seeds_w, cmin_w = R.device_route_seeds(dev(tex, np.float32), LO, HI, wc, wt, ws, tile, origin, s_pts, g_pts, 0.0, 33, 5.0 / 64)
    assert np.array_equal(bits(seeds_w.cpu().numpy()), bits(seeds)) and np.array_equal(bits(cmin_w.cpu().numpy()), bits(clear_min))


# ---- 3. the two tests of a candidate, at their edges ----------------------------------------------------------------------------------------------------
def test_exact_clearance_nan_and_lattice_line_rejections():
    ok = np.asarray([[64, 1, 0, 0]], np.int32)
    ends = np.float32([[1.5, 1.5]]), np.float32([[3.5, 3.5]])
    raw = Raw(np.zeros((1, 1, 1)), [(0, 0)], [0], 8, (0, 0), 1)
    for value, accepted in M.corner_values():
        tex, cells = M.corner_case(value)
        for iters in (1, 2):
            seeds, clear_min = raw.seeds(tex, (0, 0), (8, 8), 0.16, *ends, iters, 0.5, cells=cells, tiles=[[[0, 0]]], summary=ok)
            want, cmin = R.seed_trajectory(tex, (0, 0), (8, 8), cells, [(0, 0)], 8, (0, 0), ends[0][0], ends[1][0], 0.16, iters, 0.5)
            assert np.array_equal(bits(seeds[0]), bits(want)) and bits(clear_min[0]) == bits(cmin)
            if iters == 1:
                assert seeds[0, 21, :2].tolist() == ([2.5, 2.5] if accepted else [3.5, 1.5]) and seeds[0, 20, :2].tolist() == [2.5, 1.5]
    assert raw.guards_intact()
    tex, cells = M.lattice_case()
    ok = np.asarray([[64, 2, 0, 0]], np.int32)
    ends = np.float32([[3.5, 1.5]]), np.float32([[7.5, 1.5]])
    for tile, origin, tiles, p63 in ((4, (0, 0), [(0, 0), (1, 0)], 3.5), (8, (0, 0), [(0, 0), (0, 0)], 4.5), (4, (1, 0), [(0, 0), (1, 0)], 4.5)):
        raw = Raw(np.zeros((1, 1, 1)), [(0, 0)], [0], tile, origin, 2)
        seeds, clear_min = raw.seeds(tex, (0, 0), (8, 8), 0.0, *ends, 1, 0.5, cells=cells, tiles=[tiles], summary=ok)
        want, cmin = R.seed_trajectory(tex, (0, 0), (8, 8), cells, tiles, tile, origin, ends[0][0], ends[1][0], 0.0, 1, 0.5)
        assert np.array_equal(bits(seeds[0]), bits(want)) and seeds[0, 63, :2].tolist() == [p63, 1.5] and seeds[0, 64, :2].tolist() == [5.5, 1.5]
        assert raw.guards_intact()
    # a summary the descent never writes: n_tiles of 0 or below gives zero rows, one above max_tiles counts as max_tiles
    raw = Raw(np.zeros((1, 1, 1)), [(0, 0)] * 3, [0] * 3, 8, (0, 0), 2)
    summary = np.asarray([[5, 0, 0, 0], [5, 7, 0, 0], [5, -3, 0, 0]], np.int32)
    seeds, clear_min = raw.seeds(tex, (0, 0), (8, 8), 0.0, np.tile(ends[0], (3, 1)), np.tile(ends[1], (3, 1)), 1, 0.5, cells=np.tile(cells, (3, 1, 1, 1)),
                                 tiles=[[(0, 0), (0, 0)]] * 3, summary=summary)
    want, cmin = R.seed_trajectory(tex, (0, 0), (8, 8), cells, [(0, 0), (0, 0)], 8, (0, 0), ends[0][0], ends[1][0], 0.0, 1, 0.5)
    assert not bits(seeds[[0, 2]]).any() and not bits(clear_min[[0, 2]]).any() and np.array_equal(bits(seeds[1]), bits(want)) and raw.guards_intact()


# ---- 4. the world "SeedDoors" end to end ------------------------------------------------------------------------------------------------------------------
def door_crossed(seed):
    """the iy cell at which a seed's support points pass from tile (0, 0) to tile (1, 0)"""
    ix, iy = R._texels(seed[:, :2].cpu().numpy(), *E.world_map_limits(M.WORLD), M.WORLD_SHAPE)
    crossing = np.flatnonzero(np.diff((ix >= 400).astype(int)))
    assert len(crossing) == 1
    return int(iy[crossing[0]])


def test_world_routes_seeded_and_the_planner_call(registry):
    E.register_world_map(M.WORLD, M.world_bitmap())
    cells = [((100, 350), (700, 300)), ((100, 50), (700, 300)), ((700, 350), (700, 300))]                      # one goal: one field
    starts = np.stack([M.cell_centre(s) for s, _ in cells]) + np.float32(0.001)
    goals = np.stack([M.cell_centre(g) for _, g in cells])
    routes, seeds = R.world_routes_seeded(M.WORLD, starts, goals, device="cuda", smooth_iters=33)
    plain = R.world_routes(M.WORLD, starts, goals, device="cuda")
    host_routes, host_seeds = R.world_routes_seeded(M.WORLD, starts, goals, smooth_iters=33)
    assert [r.tiles.tolist() for r in routes] == [[[0, 0], [1, 0]], [[0, 0], [1, 0]], [[1, 0]]]
    for r, p, h, s, hs in zip(routes, plain, host_routes, seeds, host_seeds):
        for other in (p, h):
            assert np.array_equal(r.tiles, other.tiles) and np.array_equal(r.origins, other.origins) and np.array_equal(r.offsets, other.offsets)
            assert r.env_ids == other.env_ids and r.steps == other.steps and all(torch.equal(r.transforms[k], other.transforms[k]) for k in r.transforms)
        assert s.is_cuda and s.dtype == torch.float32 and s.shape == (64 * len(r.tiles), 4)
        assert np.array_equal(bits(s.cpu().numpy()), bits(hs.numpy()))       # device and definition: the same bits
    route, seed = R.world_route_seeded(M.WORLD, starts[0], goals[0], device="cuda", smooth_iters=33)
    assert torch.equal(seed, seeds[0]) and np.array_equal(route.tiles, routes[0].tiles)
    assert M.UPPER_DOOR[0] <= door_crossed(seeds[0]) < M.UPPER_DOOR[1]       # iy 350 -> 300 through the upper door: the only shortest way

    # the planner on the seed: MPDEnsemble's local inference, bitwise the call with a hand-built experience
    from mmd_amd.planners import PathBatchExperience, PlannerOutput
    B = 4
    sd = synth.synth_unet_state_dict(0)
    start, goal = torch.from_numpy(starts[0]), torch.from_numpy(goals[0])
    planner = R.route_planner(routes[0], "EnvHighways2D-RobotPlanarDisk", start, goal, planner_alg="mmd", device="cuda", seed=23, n_samples=B,
                              model_state_dicts=[sd] * 2, model_args=dict(n_diffusion_steps=25), trained_models_dir="")
    assert planner.num_samples == B
    res = planner(start, goal, experience=R.route_experience(seeds[0], B), seed=77)
    assert isinstance(res, PlannerOutput) and res.trajs_final.shape == (B, 2 * 64, 4) and torch.isfinite(res.trajs_final).all()
    by_hand = planner(start, goal, experience=PathBatchExperience(seeds[0].unsqueeze(0).repeat(B, 1, 1)), seed=77)
    assert torch.equal(by_hand.trajs_final, res.trajs_final)

    # close the upper door: the resident texture is rebuilt, and the new seed goes through the lower one, with the margin kept
    E.update_world_map(M.WORLD, M.world_bitmap(upper_door_open=False))
    route, seed = R.world_route_seeded(M.WORLD, starts[0], goals[0], device="cuda", smooth_iters=33)
    assert route.tiles.tolist() == [[0, 0], [1, 0]] and route.steps > routes[0].steps
    assert M.LOWER_DOOR[0] <= door_crossed(seed) < M.LOWER_DOOR[1]
    from mmd_amd import map_textures
    tex = map_textures.device_world_texture(M.WORLD, "cuda").cpu().numpy()
    ix, iy = R._texels(seed[:, :2].cpu().numpy(), *E.world_map_limits(M.WORLD), M.WORLD_SHAPE)
    assert (tex[ix, iy, 0] > np.float32(R.OBSTACLE_MARGIN)).all()
