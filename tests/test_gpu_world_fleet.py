"""-m gpu: world fleets (mmd_amd.world_fleet).  mmd_grid_window_goals is the numpy definition window_goals word for word -- on open
ground, a wall with a door and a serpentine, several fields each at two (reach, max_steps) settings, on hand-built fields that hold every
status, with guard words round every output buffer -- and its error returns leave the outputs alone.  End to end, a fleet of 4 robots
crosses a world of 800 x 400 cells with a wall and one door: the checks rest on the pinned ends of every path, not on the weights."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import world_fleet_model as M                                    # noqa: E402
from mmd_amd import _lib, environments as E, map_textures, world_fleet as F      # noqa: E402
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, UNREACHED      # noqa: E402

GUARD = 0x5A5A5A5A
PAD = 16                         # guard words in front of, between and behind the outputs (a multiple of 4: the summary rows stay aligned)
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


def raw_window_goals(dist, starts, which, goals, reach, max_steps, window):
    """mmd_grid_window_goals on numpy inputs, twice into one buffer whose every word outside the three outputs is a guard ->
    (cells, origins, summary) numpy.  The guards must be untouched and the second call must give the first one's words."""
    dist_d = torch.from_numpy(np.array(dist, dtype=np.int32)).cuda()                     # (a copy: the shared fields are read-only)
    starts_d = torch.tensor(np.asarray(starts).reshape(-1, 2), dtype=torch.int32).cuda()
    which_d = torch.tensor(np.asarray(which).reshape(-1), dtype=torch.int32).cuda()
    goals_d = torch.tensor(np.asarray(goals).reshape(-1, 2), dtype=torch.int32).cuda()
    n = starts_d.shape[0]
    at = (PAD, 2 * PAD + 2 * n, 3 * PAD + 4 * n)                 # the first word of cells, origins, summary
    size = 4 * PAD + 8 * n
    runs = []
    buf = torch.full((size,), GUARD, dtype=torch.int32, device="cuda")
    for _ in range(2):
        _lib.launch("mmd_grid_window_goals", buf, C.c_void_p(dist_d.data_ptr()), dist.shape[1], dist.shape[2], dist.shape[0],
                    C.c_void_p(starts_d.data_ptr()), C.c_void_p(which_d.data_ptr()), C.c_void_p(goals_d.data_ptr()), n, reach, max_steps,
                    window, *(C.c_void_p(buf.data_ptr() + 4 * k) for k in at))
        torch.cuda.synchronize()
        words = buf.cpu().numpy()
        out = words[at[0]:at[0] + 2 * n], words[at[1]:at[1] + 2 * n], words[at[2]:at[2] + 4 * n]
        guards = np.concatenate([words[:at[0]], words[at[0] + 2 * n:at[1]], words[at[1] + 2 * n:at[2]], words[at[2] + 4 * n:]])
        assert guards.size == 4 * PAD and (guards == GUARD).all(), "wrote outside the outputs"
        runs.append((out[0].reshape(n, 2).copy(), out[1].reshape(n, 2).copy(), out[2].reshape(n, 4).copy()))
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "a second call into the same buffer differs"
    return runs[0]


def assert_same(got, want, what):
    for name, g, w in zip(("cells", "origins", "summary"), got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(1))
        assert bad.size == 0, f"{what}: {name} differ in {bad.size} of {len(w)} queries, first {int(bad[0])}: device {g[bad[0]].tolist()} " \
                              f"definition {w[bad[0]].tolist()}"


def queries(shape, n_fields, n, seed):
    """n starts over (and a little beyond) the grid with a field each: every cell of a coarse lattice, then random ones"""
    rng = np.random.Generator(np.random.PCG64(seed))
    step = int(np.ceil(np.sqrt(shape[0] * shape[1] / (n // 2))))
    lattice = np.stack(np.meshgrid(np.arange(0, shape[0], step), np.arange(0, shape[1], step), indexing="ij"), -1).reshape(-1, 2)
    more = np.stack([rng.integers(-1, shape[0] + 1, n - len(lattice)), rng.integers(-1, shape[1] + 1, n - len(lattice))], 1)
    starts = np.concatenate([lattice, more]).astype(np.int32)
    return starts, rng.integers(0, n_fields, len(starts)).astype(np.int32)


GRIDS = {
    # name: (routable, goal cells, window, the two (reach, max_steps) settings)
    "open": (lambda: M.open_grid(), [(20, 15), (0, 0), (39, 29), (7, 22)], M.WINDOW, ((5, 100), (3, 2))),
    "door": (lambda: M.door_grid(), [(25, 5), (5, 25), (20, 22), (39, 0)], M.WINDOW, ((5, 100), (2, 3))),
    "serpentine": (lambda: M.serpentine_grid((130, 70), pitch=16, gap=5), [(125, 3), (3, 3), (70, 35)], 64, ((31, 1000), (9, 6))),
}


# ---- 1. the kernel is the definition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_kernel_is_the_definition(grid):
    make, goals, window, settings = GRIDS[grid]
    routable = make()
    dist = M.fields(routable, goals)
    assert all(dist[f][tuple(g)] == 0 for f, g in enumerate(goals)) and (dist != UNREACHED).any(axis=(1, 2)).all()
    starts, which = queries(routable.shape, len(goals), 700, 11)
    dist_d = torch.from_numpy(dist.copy()).cuda()
    stops = set()
    for reach, max_steps in settings:
        want = F.window_goals(dist, starts, which, goals, reach, max_steps, window)
        ok = want[2][:, 2] == ROUTE_OK
        assert ok.sum() > 400 and (want[2][:, 2] == ROUTE_OUTSIDE).any() and (want[2][ok, 3] == 1).any()
        short = ok & (want[2][:, 1] > 0)                         # walks that stopped short of the goal: by max_steps, or else by reach
        stops |= {"max_steps"} if (want[2][short, 0] == max_steps).any() else set()
        stops |= {"reach"} if (want[2][short, 0] < max_steps).any() else set()
        what = f"{grid}, reach {reach}, max_steps {max_steps}"
        assert_same(raw_window_goals(dist, starts, which, goals, reach, max_steps, window), want, what)
        assert_same(F.device_window_goals(dist_d, starts, which, goals, reach, max_steps, window), want, what + " (device_window_goals)")
    assert stops == {"max_steps", "reach"}
    if grid == "door":
        assert (dist == UNREACHED).any() and (want[2][:, 2] == ROUTE_UNREACHED).any()      # starts on the wall


def test_every_status_in_one_batch():
    """Hand-built fields: an unconverged one (stuck at once and after 2 steps), a converged one, one that is UNREACHED everywhere, and one
    of words no search would leave (negative, 0 everywhere else) with a goal at the ends of int32."""
    stuck, goal0, sticks_at = M.unconverged_field()
    odd = np.zeros((1,) + M.SMALL, np.int32)
    odd[0, 5, 5], odd[0, 6, 6], odd[0, 7, 7] = -3, I32.min, I32.max - 1
    dist = np.concatenate([stuck, M.fields(M.open_grid(), [(20, 15)]), np.full((1,) + M.SMALL, UNREACHED, np.int32), odd])
    goals = [goal0, (20, 15), (1, 1), (I32.min, I32.max)]
    starts = [sticks_at, (10, 12), (14, 10), (20, 15), (20, 14), (-1, 3), (3, 30), (40, 0), (I32.min, I32.max), (14, 10), (14, 10), (14, 10),
              (9, 9), (5, 5), (6, 6), (7, 7), (8, 8)]
    which = [0, 0, 1, 1, 1, 1, 1, 1, 1, 4, -1, I32.max, 2, 3, 3, 3, 3]
    want = F.window_goals(dist, starts, which, goals, M.REACH, 100, M.WINDOW)
    assert want[2][:9].tolist() == [[0, 14, ROUTE_STUCK, 0], [2, 14, ROUTE_STUCK, 0], [9, 2, ROUTE_OK, 0], [0, 0, ROUTE_OK, 1], [1, 0, ROUTE_OK, 1]] + \
        [[-1, -1, ROUTE_OUTSIDE, 0]] * 4
    assert want[2][9:13].tolist() == [[-1, -1, ROUTE_OUTSIDE, 0]] * 3 + [[-1, -1, ROUTE_UNREACHED, 0]]
    assert want[2][13:].tolist() == [[0, -3, ROUTE_OK, 0], [0, I32.min, ROUTE_OK, 0], [0, I32.max - 1, ROUTE_STUCK, 0], [0, 0, ROUTE_OK, 1]]
    assert set(want[2][:, 2].tolist()) == {ROUTE_OK, ROUTE_UNREACHED, ROUTE_STUCK, ROUTE_OUTSIDE}
    assert_same(raw_window_goals(dist, starts, which, goals, M.REACH, 100, M.WINDOW), want, "the batch of every status")
    # no field at all: every query is outside, and nothing is read
    none = raw_window_goals(np.zeros((0,) + M.SMALL, np.int32), starts[:3], [0, 0, 0], np.zeros((0, 2), np.int32), M.REACH, 100, M.WINDOW)
    assert none[2].tolist() == [[-1, -1, ROUTE_OUTSIDE, 0]] * 3 and not none[0].any() and not none[1].any()


def test_error_returns_leave_the_outputs_alone():
    lib = _lib.load()
    dist = torch.zeros(2, 40, 30, dtype=torch.int32, device="cuda")
    ints = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((256,), GUARD, dtype=torch.int32, device="cuda")
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * k)                                  # noqa: E731
    good = dict(dist=p(dist), nx=40, ny=30, n_fields=2, starts=p(ints), field=p(ints, 32), goals=p(ints, 48), n=7, reach=5, max_steps=9,
                window=12, cells=p(out, 16), origins=p(out, 64), summary=p(out, 128))
    order = ("dist", "nx", "ny", "n_fields", "starts", "field", "goals", "n", "reach", "max_steps", "window", "cells", "origins", "summary")
    stream = C.c_void_p(_lib.raw_stream())
    call = lambda **kw: lib.mmd_grid_window_goals(*(dict(good, **kw)[k] for k in order), stream)      # noqa: E731
    for kw in (dict(nx=0), dict(nx=2049), dict(ny=0), dict(ny=2049), dict(n_fields=-1), dict(n=-1), dict(n=I32.max), dict(reach=0),
               dict(reach=6), dict(reach=-1), dict(max_steps=0), dict(max_steps=-5), dict(window=31), dict(window=0), dict(window=3, reach=1),
               dict(window=41, ny=50), dict(dist=None), dict(goals=None), dict(starts=None), dict(field=None), dict(cells=None),
               dict(origins=None), dict(summary=None)):
        assert call(**kw) == 2 and lib.mmd_last_error().startswith(b"mmd_grid_window_goals:"), (kw, lib.mmd_last_error())
    assert call(n=0) == 0 and call(n=0, dist=None, starts=None, summary=None) == 0
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call, or one of no queries, wrote"
    assert call() == 0                                        # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    words = out.cpu().numpy()
    assert (words[16:30].reshape(7, 2) == 0).all() and (words[64:78].reshape(7, 2) == [[0, 0]]).all()      # all at cell (0, 0), field 0 of zeros
    assert words[128:156].reshape(7, 4).tolist() == [[0, 0, ROUTE_OK, 1]] * 7
    rest = np.concatenate([words[:16], words[30:64], words[78:128], words[156:]])
    assert (rest == GUARD).all()


# ---- 2. a fleet crosses a world ----------------------------------------------------------------------------------------------------------------------
WORLD, SEALED = "FleetWorld", "FleetSealed"
SHAPE = (800, 400)
ORIGIN = (2.0, 2.0)
T, B, ROUNDS, SEED = 25, 4, 2, 31
REACH, MAX_STEPS = 120, 360
START_CELLS = np.asarray([(250, 100), (300, 300), (560, 200), (600, 60)])
GOAL_CELLS = np.asarray([(560, 280), (520, 120), (260, 200), (640, 90)])


def world_bitmap(door=True):
    """A wall of 4 cells across the world's middle, with one door of 120 cells (the clearance of 0.16 = 32 cells leaves 56 of them)"""
    occ = np.zeros(SHAPE, np.uint8)
    occ[398:402, :] = 1
    if door:
        occ[398:402, 140:260] = 0
    return occ


def points_in(cells, shift):
    """float32 global points inside the cells, `shift` off their centres"""
    return (np.asarray(ORIGIN) + (np.asarray(cells) + 0.5) * E.SDF_CELL_SIZE + shift).astype(np.float32)


@pytest.fixture(scope="module")
def crossing():
    """(fleet, the first run's result, the number of resident map sets before and after it), for the module.

    Why the ends can be held to the bit: the world's lower corner is at (2, 2), so every global coordinate and every window offset is at
    least 2 and therefore a multiple of 2^-22; a local coordinate, their difference, is such a multiple within [-1, 1], which float32
    holds exactly, and so are x + 1, its half, its double and x - 1 of the normaliser over [-1, 1] and back; adding the offset gives the
    global coordinate again, which is a float32.  Every operation between the caller's point and the path's end is exact.  (On the same
    world centred on the global origin the coordinates are finer than 2^-23 and those operations round: measured once, every end then
    lies within 6.0e-8 of its point, not on it.  That is the sampler's frame arithmetic, not the fleet's.)"""
    import gpu_common
    E.register_world_map(WORLD, world_bitmap(), origin=ORIGIN)
    E.register_world_map(SEALED, world_bitmap(door=False), origin=ORIGIN)
    starts, goals = points_in(START_CELLS, 0.001), points_in(GOAL_CELLS, -0.0015)
    fleet = F.WorldFleet(gpu_common.hip_model(T), WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B)
    before = len(map_textures._TEXTURES)
    result = fleet.run(max_rounds=ROUNDS, seed=SEED)
    after = len(map_textures._TEXTURES)
    yield fleet, result, starts, goals, (before, after)
    E.unregister_world_map(WORLD)
    E.unregister_world_map(SEALED)


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fleet_arrives_in_the_definitions_epochs(crossing):
    fleet, result, starts, goals, (before, after) = crossing
    assert fleet.field_goals.shape == (4, 2) and fleet.dist.shape == (4,) + SHAPE
    dist = fleet.dist.cpu().numpy()
    # the definition, iterated per robot on the robot's field: the epochs, and every epoch's targets
    calls = [M.iterate(dist[fleet.fields[r]], START_CELLS[r], GOAL_CELLS[r], REACH, MAX_STEPS, 400) for r in range(4)]
    n_epochs = max(len(c) for c in calls)
    assert n_epochs >= 3 and min(len(c) for c in calls) < n_epochs              # one robot arrives early and keeps taking part
    assert n_epochs <= fleet.epoch_bound() == max(F.epoch_bound(dist[fleet.fields[r]][tuple(START_CELLS[r])], REACH, MAX_STEPS) for r in range(4))
    assert len(result.epochs) == n_epochs
    assert result.paths.shape == (4, n_epochs * 64, 2) and result.paths.is_cuda and bool(torch.isfinite(result.paths).all())
    assert result.arrived.tolist() == [True] * 4
    paths = result.paths.cpu().numpy()
    assert same_bits(paths[:, 0], starts), "the first epoch begins at the starts"
    for e in range(1, n_epochs):
        assert same_bits(paths[:, 64 * e], paths[:, 64 * e - 1]), f"epoch {e} does not begin where epoch {e - 1} ended"
    assert same_bits(paths[:, -1], goals), "a robot's last point is not its goal"
    lo, hi = E.world_map_limits(WORLD)
    for e, epoch in enumerate(result.epochs):
        at = [c[e] if e < len(c) else None for c in calls]
        for r in range(4):
            if at[r] is None:                                 # arrived before: from the goal cell to the goal cell
                want = [0, 0, ROUTE_OK, 1]
                cell, origin = tuple(GOAL_CELLS[r]), tuple(np.clip(GOAL_CELLS[r] - 200, 0, np.asarray(SHAPE) - 400))
            else:
                c0, cell, origin, steps, remaining = at[r]
                want = [steps, remaining, ROUTE_OK, int(remaining == 0)]
            assert epoch["summary"][r].tolist() == want, (e, r)
            assert same_bits(epoch["offsets"][r], E.world_map_window_offsets(WORLD, np.asarray([origin], np.int32))[0]), (e, r)
            end = goals[r] if want[3] else F.cell_centres(np.asarray(cell), lo, hi, SHAPE)
            assert same_bits(paths[r, 64 * e + 63], np.asarray(end, np.float32)), (e, r)
        assert len(epoch["conflict_counts"]) in (2, 3)           # a report before each of at most 2 rounds, and the final one
    assert after == before, "an epoch's window map set stayed resident"
    assert not any(WORLD + "@" in m for key in map_textures._TEXTURES for m in key[0])


def test_fleet_run_repeats_and_equals_hand_built_epochs(crossing):
    import gpu_common
    from mmd_amd.world import WorldRobotSampler
    fleet, result, starts, goals, _ = crossing
    model = gpu_common.hip_model(T)
    again = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B).run(max_rounds=ROUNDS, seed=SEED)
    assert same_bits(again.paths, result.paths), "two runs with one seed differ"
    assert [e["conflict_counts"] for e in again.epochs] == [e["conflict_counts"] for e in result.epochs]
    other = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B)
    positions = starts
    for e, epoch in enumerate(result.epochs):
        targets = other.epoch_targets(positions)
        assert np.array_equal(targets.summary, epoch["summary"]) and same_bits(targets.offsets, epoch["offsets"])
        sampler = WorldRobotSampler(model, positions, targets.points, targets.offsets, env_id=WORLD, n_samples=B)
        res = sampler.plan(max_rounds=ROUNDS, seed=SEED + e)
        assert map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), "cuda") is True
        assert same_bits(res.paths_local, result.paths[:, 64 * e:64 * e + 64]), f"epoch {e} is not the hand-built sampler's plan"
        assert list(res.conflict_counts) == epoch["conflict_counts"]
        positions = res.paths_local[:, -1].cpu().numpy()


def test_fleet_refuses_what_it_cannot_plan(crossing):
    import gpu_common
    fleet, result, starts, goals, _ = crossing
    model = gpu_common.hip_model(T)
    outside, on_wall = starts.copy(), goals.copy()
    outside[2] = (1.5, 3.0)
    on_wall[1] = points_in([(400, 100)], 0.0)[0]
    with pytest.raises(ValueError, match="start of robot 2.*outside"):
        F.WorldFleet(model, WORLD, outside, goals)
    with pytest.raises(ValueError, match="goal of robot 1.*not routable"):
        F.WorldFleet(model, WORLD, starts, on_wall)
    with pytest.raises(ValueError, match="robot 0.*cannot be reached"):
        F.WorldFleet(model, SEALED, starts, goals)
    for kw in (dict(reach=200), dict(reach=0), dict(max_steps=0), dict(rank=1), dict(env_id="EnvEmpty2D")):
        with pytest.raises(ValueError):
            F.WorldFleet(model, WORLD, starts, goals, **kw)
    with pytest.raises(ValueError, match="max_epochs"):
        fleet.run(max_epochs=0)
