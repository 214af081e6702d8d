"""-m gpu: one sampler for a whole fleet run (WorldFleet(persistent=True)).  mmd_sdf_grid_windows_moved writes, for every window whose
origin is not the held one, the slice mmd_sdf_grid_windows writes, and leaves the others alone; mmd_fleet_epoch_frames writes the host
definitions' bits, where the operations are exact and where they round; a moved sampler plans what a fresh one plans; a persistent
fleet is the default fleet bit for bit, on one texture that update_world_map still reaches."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, environments as E, map_textures, synth, world_fleet as F      # noqa: E402
from mmd_amd.normalization import LimitsNormalizer                                       # noqa: E402
from mmd_amd.world import WorldRobotSampler, random_world_instance                       # noqa: E402
from mmd_amd.world_routes import ROUTE_OK                                                # noqa: E402

GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


def words(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype in (np.float32, np.uint32, np.int32), a.dtype
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_words(got, want, what):
    got, want = words(got), words(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        where = np.argwhere(bad)[:4]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {where.tolist()}: got "
                             f"{[hex(got[tuple(w)]) for w in where]} want {[hex(want[tuple(w)]) for w in where]}")


# ---- 1. the moved cut ------------------------------------------------------------------------------------------------------------------------
def hand_world(wnx, wny):
    """any 32-bit patterns, with NaN payloads, -0 and infinities at the corners and inside"""
    rng = np.random.Generator(np.random.PCG64(wnx * 100 + wny))
    world = rng.integers(0, 1 << 32, (wnx, wny, 4), dtype=np.uint64).astype(np.uint32)
    world[3, 4] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000]
    world[0, 0] = [0x80000000, 0xFF800001, 0x7FFFFFFF, 0x00000001]
    world[wnx - 1, wny - 1] = [0xFFFFFFFF, 0x80000000, 0x7F800000, 0xFF800000]
    return world


def dev_i32(a, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int64).astype(np.int32)))
    return (t if shape is None else t.reshape(shape)).cuda()


def moved_cut(world_d, wnx, wny, origins_d, held_d, n, nx, ny, buf):
    _lib.launch("mmd_sdf_grid_windows_moved", buf, C.c_void_p(world_d.data_ptr()), wnx, wny, C.c_void_p(origins_d.data_ptr()),
                C.c_void_p(held_d.data_ptr()) if held_d is not None else None, n, nx, ny, C.c_void_p(buf.data_ptr()))
    torch.cuda.synchronize()


# the issue's world of 19 x 23 texels takes the 8 x 8 windows and, 340 cells as well, 17 x 20 ones; a window of 20 x 17 fits the same
# world turned, 23 x 19 (a window is at most the world per axis)
@pytest.mark.parametrize("world_shape, window", [((19, 23), (8, 8)), ((23, 19), (20, 17)), ((19, 23), (17, 20))])
def test_moved_cut_writes_what_moved_and_only_that(world_shape, window):
    (wnx, wny), (nx, ny) = world_shape, window
    n, cells = 5, window[0] * window[1]
    assert cells in (64, 340)
    world_d = torch.from_numpy(hand_world(wnx, wny).view(np.int32)).cuda()
    held = [(2, 3), (1, 1), (0, 0), (4, 4), (0, 1)]
    origins = [(2, 3), (1, 2), (-3, -2), (wnx + 5, 2), (wnx - nx, wny - ny)]        # held; a cell away; negative; beyond; the far corner
    origins_d, held_d = dev_i32(origins), dev_i32(held)
    want = torch.full((n * cells * 4,), GUARD, dtype=torch.int32, device="cuda")
    _lib.launch("mmd_sdf_grid_windows", want, C.c_void_p(world_d.data_ptr()), wnx, wny, C.c_void_p(origins_d.data_ptr()), n, nx, ny,
                C.c_void_p(want.data_ptr()))
    want = words(want).reshape(n, cells * 4)
    pad = 256
    for held_now, written in ((held_d, [1, 2, 3, 4]), (None, [0, 1, 2, 3, 4])):
        buf = torch.full((n * cells * 4 + pad,), GUARD, dtype=torch.int32, device="cuda")
        for _ in range(2):                                    # the second call into the same buffer gives the same words
            moved_cut(world_d, wnx, wny, origins_d, held_now, n, nx, ny, buf)
            got = words(buf)
            assert (got[n * cells * 4:] == GUARD).all(), "wrote behind the windows"
            got = got[:n * cells * 4].reshape(n, cells * 4)
            for k in range(n):
                if k in written:
                    assert_same_words(got[k], want[k], f"slice {k} at {origins[k]}")
                else:
                    assert (got[k] == GUARD).all(), f"slice {k} was held at its origin and has been written"
        assert np.array_equal(words(origins_d), words(dev_i32(origins))) and np.array_equal(words(held_d), words(dev_i32(held)))


def test_moved_cut_error_returns_leave_the_output_alone():
    wnx, wny, nx, ny, n = 19, 23, 8, 8, 5
    world_d = torch.from_numpy(hand_world(wnx, wny).view(np.int32)).cuda()
    origins_d = dev_i32([(1, 1)] * n)
    buf = torch.full((n * nx * ny * 4,), GUARD, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    w, o, b = C.c_void_p(world_d.data_ptr()), C.c_void_p(origins_d.data_ptr()), C.c_void_p(buf.data_ptr())
    stream = _lib.current_stream_ptr()
    bad = [((w, wnx, wny, o, None, -1, nx, ny, b), "n_windows"), ((w, wnx, wny, o, None, 65536, nx, ny, b), "n_windows"),
           ((w, 0, wny, o, None, n, nx, ny, b), "world"), ((w, wnx, -1, o, None, n, nx, ny, b), "world"),
           ((w, wnx, wny, o, None, n, 0, ny, b), "windows"), ((w, wnx, wny, o, None, n, wnx + 1, ny, b), "windows"),
           ((w, wnx, wny, o, None, n, nx, wny + 1, b), "windows"), ((None, wnx, wny, o, None, n, nx, ny, b), "NULL world"),
           ((w, wnx, wny, None, None, n, nx, ny, b), "NULL origins"), ((w, wnx, wny, o, o, n, nx, ny, None), "NULL windows"),
           ((w, 46341, 46341, o, None, n, nx, ny, b), "32-bit")]
    for args, word in bad:
        rc = lib.mmd_sdf_grid_windows_moved(*args, stream)
        message = lib.mmd_last_error().decode()
        assert rc != 0 and word in message and "mmd_sdf_grid_windows_moved" in message, (word, rc, message)
    assert lib.mmd_sdf_grid_windows_moved(None, wnx, wny, None, None, 0, nx, ny, None, stream) == 0       # nothing to cut
    torch.cuda.synchronize()
    assert (words(buf) == GUARD).all(), "an error return wrote to the output"


# ---- the door world of test_gpu_world_fleet.py, under names of this module ----------------------------------------------------------------
WORLD, CENTRED = "PersistWorld", "PersistCentred"
SHAPE = (800, 400)
ORIGIN = (2.0, 2.0)
T, B, ROUNDS, SEED = 25, 4, 2, 31
REACH, MAX_STEPS = 120, 360
START_CELLS = np.asarray([(250, 100), (300, 300), (560, 200), (600, 60)])
GOAL_CELLS = np.asarray([(560, 280), (520, 120), (260, 200), (640, 90)])


def world_bitmap(door=(140, 260)):
    occ = np.zeros(SHAPE, np.uint8)
    occ[398:402, :] = 1
    occ[398:402, door[0]:door[1]] = 0
    return occ


def points_in(cells, shift, origin=ORIGIN):
    return (np.asarray(origin) + (np.asarray(cells) + 0.5) * E.SDF_CELL_SIZE + shift).astype(np.float32)


@pytest.fixture(scope="module")
def door_world():
    """(model, starts, goals) on the door world at origin (2, 2); the same bitmap is registered centred on the global origin as well"""
    import gpu_common
    E.register_world_map(WORLD, world_bitmap(), origin=ORIGIN)
    E.register_world_map(CENTRED, world_bitmap())
    yield gpu_common.hip_model(T), points_in(START_CELLS, 0.001), points_in(GOAL_CELLS, -0.0015)
    E.unregister_world_map(WORLD)
    E.unregister_world_map(CENTRED)


# ---- 2. the frames kernel ----------------------------------------------------------------------------------------------------------------
def host_frames(name, cells, origins, summary, points, goal_points):
    """the definitions: world_map_window_offsets, cell_centres / the goal point, the constructor's hard conditions, straight_line_paths"""
    lo, hi = E.world_map_limits(name)
    offsets = E.world_map_window_offsets(name, origins)
    subgoals = np.ascontiguousarray(F.cell_centres(cells, lo, hi, SHAPE), dtype=np.float32)
    arrived = summary[:, 3] == 1
    subgoals[arrived] = goal_points[arrived]
    nz = LimitsNormalizer(synth.NORM_MINS, synth.NORM_MAXS)
    hard = []
    for ends in (points - offsets, subgoals - offsets):                  # WorldRobotSampler.__init__, then MultiRobotSampler.__init__
        st = torch.as_tensor(ends, dtype=torch.float32)
        hard.append(nz.normalize(torch.cat((st, torch.zeros_like(st)), -1)).numpy())
    return offsets, subgoals, hard[0], hard[1], synth.straight_line_paths(points, subgoals, 64)


FRAME_CASES = {
    # cells, origins, summary, the cell of the current point, the cell of the goal point
    1: ([(370, 215)], [(50, 0)], [(120, 301, ROUTE_OK, 0)], [(250, 100)], [(560, 280)]),
    # robot 0 under way; robot 1 arrived (its sub-goal is its exact goal point); robot 2 with its window clamped at the world's far edge
    3: ([(370, 215), (520, 120), (700, 330)], [(50, 0), (320, 0), (400, 0)], [(120, 301, ROUTE_OK, 0), (7, 0, ROUTE_OK, 1), (120, 9, ROUTE_OK, 0)],
        [(250, 100), (513, 120), (640, 390)], [(560, 280), (520, 120), (700, 339)]),
}


@pytest.mark.parametrize("name", [WORLD, CENTRED])          # every operation exact; the operations round
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("strided", [False, True])
def test_frames_kernel_is_the_host_definitions(door_world, name, n, strided):
    cells, origins, summary, at, goal = (np.asarray(v, np.int32) for v in FRAME_CASES[n])
    origin = E.world_map_origin(name)
    points, goal_points = points_in(at, 0.001, origin), points_in(goal, -0.0015, origin)
    words_d = dev_i32(np.concatenate([cells.reshape(-1), origins.reshape(-1), summary.reshape(-1)]))
    if strided:                                              # the last points of paths [n, 64, 2], read where they lie
        paths = torch.full((n, 64, 2), float("nan"), device="cuda")
        paths[:, -1] = torch.from_numpy(points).cuda()
        points_d = paths[:, -1]
        assert points_d.stride(0) == 128
    else:
        points_d = torch.from_numpy(points).cuda()
    got = F.device_epoch_frames(name, words_d, points_d, torch.from_numpy(goal_points).cuda())
    want = host_frames(name, cells, origins, summary, points, goal_points)
    for what, g, w in zip(("offsets", "sub-goal points", "hard conditions of row 0", "hard conditions of row 63", "lines"), got, want):
        assert g.dtype == torch.float32 and w.dtype == np.float32
        assert_same_words(g, w, f"{name}, n = {n}: {what}")


def test_frames_kernel_takes_any_words(door_world):
    """nothing is indexed by the words: words of every size write finite or non-finite floats, and only into the outputs"""
    n = 3
    i32 = np.iinfo(np.int32)
    words_d = dev_i32([i32.min, i32.max, -1, 0, 7, i32.min] + [i32.max, i32.min, -400, 1 << 30, 0, -1] + [0, 0, 4, 1, -1, -1, 1, 0, 5, 5, 5, i32.min])
    pts = torch.from_numpy(points_in(START_CELLS[:n], 0.0)).cuda()
    out = F.device_epoch_frames(WORLD, words_d, pts, pts.clone())
    torch.cuda.synchronize()
    assert out[0].shape == (n, 2) and out[4].shape == (n, 64, 2)
    assert_same_words(out[1][0], pts[0].cpu().numpy(), "summary[.., 3] == 1 takes the goal point whatever the status")


# ---- 3. a moved sampler is a fresh sampler ---------------------------------------------------------------------------------------------------
def same_plan(a, b, what):
    assert_same_words(a.paths_local, b.paths_local, f"{what}: paths")
    assert_same_words(a.trajs, b.trajs, f"{what}: samples")
    assert list(a.conflict_counts) == list(b.conflict_counts) and a.n_rounds == b.n_rounds, what
    assert np.array_equal(a.robot_counts.cpu().numpy(), b.robot_counts.cpu().numpy()), what


@pytest.fixture(scope="module")
def two_epochs(door_world):
    """the targets of the fleet's first epoch, and those of the epoch that starts on its sub-goal points"""
    model, starts, goals = door_world
    fleet = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B)
    first = fleet.epoch_targets(starts)
    second = fleet.epoch_targets(first.points)
    assert (first.origins != second.origins).any()
    return (starts, first), (first.points, second)


@pytest.mark.parametrize("table", ["dense", "binned"])
def test_moved_sampler_plans_what_a_fresh_one_plans(door_world, two_epochs, table):
    model = door_world[0]
    (p0, t0), (p1, t1) = two_epochs
    sets = len(map_textures._WINDOW_SETS)
    moved = WorldRobotSampler(model, p0, t0.points, t0.offsets, env_id=WORLD, n_samples=B, constraint_table=table, own_windows=True)
    assert len(map_textures._WINDOW_SETS) == sets + 1 and moved._window_ids is None
    ptr = moved.guide._grids.data_ptr()
    assert moved.guide._grids.shape == (4, 1, 400, 400, 4) and moved.guide._robot_map.cpu().tolist() == [0, 1, 2, 3]
    moved.plan(max_rounds=1, seed=3)                              # a used sampler: tables, picks and caches of another epoch
    builds = map_textures.N_TEXTURE_BUILDS
    moved.move(p1, t1.points, t1.offsets)
    assert map_textures.N_TEXTURE_BUILDS - builds == int((t0.origins != t1.origins).any(1).sum())
    assert moved.guide._grids.data_ptr() == ptr
    fresh = WorldRobotSampler(model, p1, t1.points, t1.offsets, env_id=WORLD, n_samples=B, constraint_table=table)
    try:
        assert_same_words(moved.guide._grids[moved.guide._robot_map.long(), 0], fresh.guide._grids[fresh.guide._robot_map.long(), 0], "slices")
        for row in (0, 63):
            assert_same_words(moved.hard_conds[row], fresh.hard_conds[row], f"hard conditions of row {row}")
        assert_same_words(moved.offsets, fresh.offsets, "offsets")
        assert (moved.world_limits, moved.world_grid, moved.neighbor_slots) == (fresh.world_limits, fresh.world_grid, fresh.neighbor_slots)
        same_plan(moved.plan(max_rounds=ROUNDS, seed=SEED), fresh.plan(max_rounds=ROUNDS, seed=SEED), f"{table} table")
    finally:
        assert map_textures.release_sdf_textures(sorted(set(fresh._window_ids)), "cuda") is True
        moved.release_windows()
    assert len(map_textures._WINDOW_SETS) == sets


def test_moved_sampler_on_a_tile_map(door_world):
    """EnvEmpty2D: no textures are involved; any sampler moves"""
    model = door_world[0]
    a, b = random_world_instance(4, 6.0, 5), random_world_instance(4, 6.0, 6)
    moved = WorldRobotSampler(model, *a, n_samples=B)
    moved.plan(max_rounds=1, seed=3)
    moved.move(*b)
    same_plan(moved.plan(max_rounds=ROUNDS, seed=SEED), WorldRobotSampler(model, *b, n_samples=B).plan(max_rounds=ROUNDS, seed=SEED), "tile map")
    with pytest.raises(ValueError, match="outside the normaliser's limits"):
        moved.move(b[0] + 3.0, b[1], b[2])                       # the constructor's validation, and nothing changed
    assert_same_words(moved.offsets, b[2], "offsets after a refused move")


def test_move_needs_windows_of_the_samplers_own(door_world, two_epochs):
    model = door_world[0]
    (p0, t0), (p1, t1) = two_epochs
    named = WorldRobotSampler(model, p0, t0.points, t0.offsets, env_id=WORLD, n_samples=B)
    try:
        with pytest.raises(ValueError, match="own_windows=True"):
            named.move(p1, t1.points, t1.offsets)
    finally:
        map_textures.release_sdf_textures(sorted(set(named._window_ids)), "cuda")


# ---- 4. the persistent fleet is the default fleet ----------------------------------------------------------------------------------------------
def watched_run(fleet, **run_kwargs):
    """fleet.run with every step watched -> (result, [(texture pointer, N_TEXTURE_BUILDS it added, origins)] per epoch)"""
    seen, step = [], fleet.step

    def watched(seed, max_rounds=8):
        builds = map_textures.N_TEXTURE_BUILDS
        res, targets = step(seed, max_rounds)
        seen.append((fleet._sampler.guide._grids.data_ptr(), map_textures.N_TEXTURE_BUILDS - builds, targets.origins.copy()))
        return res, targets
    fleet.step = watched
    return fleet.run(**run_kwargs), seen


@pytest.mark.parametrize("options, run_kwargs", [({}, {}), ({"seed_epochs": True}, {}), ({"separation": F.SUBGOAL_SEPARATION}, {"max_epochs": 6})],
                         ids=["plain", "seeded", "apart"])
def test_persistent_fleet_is_the_default_fleet(door_world, options, run_kwargs):
    model, starts, goals = door_world
    kw = dict(reach=REACH, max_steps=MAX_STEPS, n_samples=B, **options)
    want = F.WorldFleet(model, WORLD, starts, goals, **kw).run(max_rounds=ROUNDS, seed=SEED, **run_kwargs)
    textures, sets = len(map_textures._TEXTURES), len(map_textures._WINDOW_SETS)
    fleet = F.WorldFleet(model, WORLD, starts, goals, persistent=True, **kw)
    got, seen = watched_run(fleet, max_rounds=ROUNDS, seed=SEED, **run_kwargs)
    assert len(map_textures._TEXTURES) == textures, "a persistent epoch built a named map set"
    assert fleet._sampler is None and len(map_textures._WINDOW_SETS) == sets, "run() did not close the fleet"
    assert fleet.close() is None and len(map_textures._WINDOW_SETS) == sets
    assert_same_words(got.paths, want.paths, "paths")
    assert got.arrived.tolist() == want.arrived.tolist() and len(got.epochs) == len(want.epochs) >= 2
    for e, (g, w) in enumerate(zip(got.epochs, want.epochs)):
        assert set(g) == set(w), e
        assert g["conflict_counts"] == w["conflict_counts"] and np.array_equal(g["summary"], w["summary"]), e
        assert_same_words(g["offsets"], w["offsets"], f"epoch {e}: offsets")
        if "clear_min" in w:
            assert_same_words(g["clear_min"], w["clear_min"], f"epoch {e}: clear_min")
        if "held_back" in w:
            assert np.array_equal(g["held_back"], w["held_back"]) and (g["sweeps"], g["stalled"]) == (w["sweeps"], w["stalled"]), e
    assert "clear_min" in want.epochs[0] if options.get("seed_epochs") else "clear_min" not in want.epochs[0]
    # one texture for the run; a slice is cut when its origin moves: all 4 in the first epoch, none for a robot that has arrived
    assert len({ptr for ptr, _, _ in seen}) == 1
    assert seen[0][1] == 4
    for e in range(1, len(seen)):
        assert seen[e][1] == int((seen[e][2] != seen[e - 1][2]).any(1).sum()), e
    if not options:
        # a robot whose sub-goal was its goal in epoch e - 2 starts epoch e - 1 on its goal cell and stays: epoch e finds its window held
        still = [int((want.epochs[e - 2]["summary"][:, 3] == 1).sum()) for e in range(2, len(seen))]
        assert any(still), "no robot arrives two epochs before the last"
        for e, n_still in zip(range(2, len(seen)), still):
            assert seen[e][1] <= 4 - n_still, f"epoch {e}: a robot that arrived early still counts"


def test_persistent_fleet_closes_on_an_exception(door_world):
    model, starts, goals = door_world
    sets = len(map_textures._WINDOW_SETS)
    fleet = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, persistent=True, neighbor_slots=9)
    with pytest.raises(ValueError, match="neighbor_slots"):    # the sampler's own refusal
        fleet.run(max_rounds=ROUNDS, seed=SEED)
    assert fleet._sampler is None and len(map_textures._WINDOW_SETS) == sets


# ---- 5. update_world_map reaches the fleet's one texture -----------------------------------------------------------------------------------
def test_update_world_map_recuts_the_slices_at_their_current_origins(door_world):
    model, starts, goals = door_world
    fleet = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, persistent=True)
    try:
        _, first = fleet.step(SEED, 1)
        _, second = fleet.step(SEED + 1, 1)
        assert (first.origins != second.origins).any()
        grids = fleet._sampler.guide._grids
        ptr, builds = grids.data_ptr(), map_textures.N_TEXTURE_BUILDS
        before = grids[:, 0].clone()
        E.update_world_map(WORLD, world_bitmap(door=(150, 250)))
        try:
            assert map_textures.N_TEXTURE_BUILDS - builds == 1 + 4            # the world's texture and the set's four slices
            crops = E.world_map_windows(WORLD, second.origins)                # of the new texture, at the CURRENT origins
            assert not np.array_equal(words(crops), words(before)), "the narrowed door shows in no window"
            assert_same_words(grids[:, 0], crops, "the slices after the update")
            assert fleet._sampler.guide._grids.data_ptr() == ptr
            _, third = fleet.step(SEED + 2, 1)                                # and the fleet goes on, on the same storage
            assert fleet._sampler.guide._grids.data_ptr() == ptr
            assert_same_words(grids[:, 0], E.world_map_windows(WORLD, third.origins), "the slices an epoch later")
        finally:
            E.update_world_map(WORLD, world_bitmap())
    finally:
        fleet.close()
