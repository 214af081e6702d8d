"""CPU: the seeds of a world fleet's epochs (mmd_amd.world_fleet) -- the definitions window_goal_samples and window_seed on
world_fleet_model's open, door and serpentine grids: the samples against window_goal and against the cell path rebuilt one step at a
time, the seed's ends, clearance and window; and the argument checks of mmd_grid_window_goal_samples and mmd_window_seeds, which answer
before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

import world_fleet_model as M
import world_fleet_seed_model as S
from mmd_amd import _lib, world_fleet as F
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, _texels, cell_centres, sample_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- 1. the samples of a walk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, stride", [("open", 3), ("door", 3), ("serpentine", 11)])
def test_samples_are_cells_of_the_walk(name, stride):
    routable, dist, goals, window, (reach, max_steps), _, _ = S.grid(name)
    starts = np.argwhere(np.ones_like(routable))[::stride]
    classes = set()
    for f, goal in enumerate(goals):
        for setting in ((reach, max_steps), (2, 3)):
            for start in list(starts[f::len(goals)]) + [np.asarray(goal)]:
                got = F.window_goal_samples(dist[f], start, goal, *setting, window)
                want = F.window_goal(dist[f], start, goal, *setting, window)
                assert got[:5] == want
                cell, _, steps, _, status = want
                samples = got[5]
                assert samples.dtype == np.int32 and samples.shape == (64, 2)
                if status != ROUTE_OK:
                    assert not samples.any()
                    continue
                classes.add("0" if steps == 0 else "<63" if steps < 63 else "63" if steps == 63 else ">63")
                assert tuple(samples[0]) == tuple(start) and tuple(samples[63]) == cell
                jump = np.abs(np.diff(samples, axis=0)).sum(1)
                assert jump.max() <= -(-steps // 63) and (steps > 63 or jump.max() <= 1)
                assert np.abs(samples - np.asarray(start)).max() <= setting[0]
                path = S.path_by_single_steps(dist[f], start, goal, steps, window)
                assert path[-1] == cell and np.array_equal(samples, np.asarray(path, np.int32)[sample_offsets(steps + 1)])
                assert np.array_equal(sample_offsets(steps + 1), (np.arange(64) * steps + 31) // 63)
                if steps <= 63:
                    assert {tuple(c) for c in samples.tolist()} == set(path)      # every cell of a short path is a sample
    assert classes >= ({"0", "<63", "63", ">63"} if name == "serpentine" else {"0", "<63"})


def test_statuses_and_the_batch_form():
    stuck, goal0, sticks_at = M.unconverged_field()
    dist = np.concatenate([stuck, M.fields(M.open_grid(), [(20, 15)])])
    goals = [goal0, (20, 15)]
    starts = [(10, 12), (14, 10), (20, 15), (-1, 3), (14, 10), (14, 10), (20, 14), sticks_at]
    which = [0, 1, 1, 1, 2, -1, 1, 0]
    cells, origins, summary, samples = F.window_goals_samples(dist, starts, which, goals, M.REACH, 100, M.WINDOW)
    for got, want in zip((cells, origins, summary), F.window_goals(dist, starts, which, goals, M.REACH, 100, M.WINDOW)):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert summary[:, 2].tolist() == [ROUTE_STUCK, ROUTE_OK, ROUTE_OK, ROUTE_OUTSIDE, ROUTE_OUTSIDE, ROUTE_OUTSIDE, ROUTE_OK, ROUTE_STUCK]
    assert samples.dtype == np.int32 and samples.shape == (8, 64, 2)
    ok = summary[:, 2] == ROUTE_OK
    assert not samples[~ok].any()                            # a stuck walk, which covered 2 steps, gives no samples either
    assert (samples[2] == (20, 15)).all()                    # on the goal: 64 times the one cell
    assert samples[6, :32].tolist() == [[20, 14]] * 32 and samples[6, 32:].tolist() == [[20, 15]] * 32       # one step: off(j) = (j + 31) // 63
    assert samples[1, 0].tolist() == [14, 10] and samples[1, 63].tolist() == [19, 14]
    walled = M.fields(M.door_grid(door=(0, 0)), [(25, 5)])[0]
    got = F.window_goal_samples(walled, (15, 5), (25, 5), M.REACH, 9, M.WINDOW)
    assert got[:5] == ((0, 0), (0, 0), -1, -1, ROUTE_UNREACHED) and not got[5].any()
    with pytest.raises(ValueError, match="reach"):
        F.window_goal_samples(dist[1], (14, 10), (20, 15), 6, 9, 12)


# ---- 2. the seed -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["door", "serpentine"])
def test_seed_keeps_ends_clearance_and_window(name):
    routable, _, _, window, _, tex, hi = S.grid(name)
    shape = routable.shape
    samples, origins, summary, s_pts, g_pts = S.robots(name, 12, 3)
    moved = 0
    for clearance in (0.0, 0.006):
        for r in range(len(samples)):
            centres = np.ascontiguousarray(cell_centres(samples[r], S.LO, hi, shape), dtype=np.float32)
            seed0, _ = F.window_seed(tex, S.LO, hi, samples[r], origins[r], window, s_pts[r], g_pts[r], clearance, 0, S.DT)
            assert np.array_equal(bits(seed0[1:-1, :2]), bits(centres[1:-1])), "no iteration: the cells' centres"
            seed, clear_min = F.window_seed(tex, S.LO, hi, samples[r], origins[r], window, s_pts[r], g_pts[r], clearance, 16, S.DT)
            assert seed.dtype == np.float32 and seed.shape == (64, 4)
            assert np.array_equal(bits(seed[0, :2]), bits(s_pts[r])) and np.array_equal(bits(seed[63, :2]), bits(g_pts[r]))
            assert not seed[[0, 63], 2:].any()
            ix, iy = _texels(seed[:, :2], S.LO, hi, shape)
            value = tex[ix, iy, 0]
            is_centre = (bits(seed[:, :2]) == bits(centres)).all(1)
            assert (is_centre[1:-1] | (value[1:-1] > np.float32(clearance))).all()
            assert ((ix >= origins[r, 0]) & (ix < origins[r, 0] + window) & (iy >= origins[r, 1]) & (iy < origins[r, 1] + window)).all()
            assert clear_min == value.min()
            two_dt = np.float32(2 * S.DT)
            assert np.array_equal(bits(seed[1:-1, 2:]), bits((seed[2:, :2] - seed[:-2, :2]) / two_dt))
            moved += int((~is_centre[1:-1]).sum())
        acc, rej = S.first_iteration_verdicts(name, samples, s_pts, g_pts, clearance)
        assert acc > 0 and (rej > 0) == (clearance > 0), (clearance, acc, rej)      # at 0.006 both branches run; at 0 every routable cell passes
    assert moved > 0


@pytest.mark.parametrize("name", ["door", "serpentine"])
def test_seed_is_the_route_seed_of_the_window_and_guards_hand_built_samples(name):
    from mmd_amd.world_routes import seed_trajectory
    routable, _, _, window, _, tex, hi = S.grid(name)
    samples, origins, summary, s_pts, g_pts, what = S.odd_rows(name)
    for r in (1, 2, 4):
        seed, clear_min = F.window_seed(tex, S.LO, hi, samples[r], origins[r], window, s_pts[r], g_pts[r], 0.0, 7, S.DT)
        want = seed_trajectory(tex, S.LO, hi, samples[r][None], [[0, 0]], window, origins[r], s_pts[r], g_pts[r], 0.0, 7, S.DT)
        assert np.array_equal(bits(seed), bits(want[0])) and bits(clear_min) == bits(want[1])
        centres = np.ascontiguousarray(cell_centres(samples[r], S.LO, hi, routable.shape), dtype=np.float32)
        stayed = np.array_equal(bits(seed[1:-1, :2]), bits(centres[1:-1]))
        assert stayed == (r != 2), what[r]                   # outside the window nothing moves; along the world's edge, inside it, points do


# ---- 3. the C entry points answer before any launch ---------------------------------------------------------------------------------------------------
def test_abi_and_sources():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9                           # two additive symbols under v9
    header = open(os.path.join(ROOT, "include", "mmd_amd.h")).read()
    for name, n_args in (("mmd_grid_window_goal_samples", 16), ("mmd_window_seeds", 18)):
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == n_args and f" {name}(" in header
    for name in ("build.sh", "__graft_entry__.py"):
        assert "mmd_amd/csrc/window_seeds.hip" in open(os.path.join(ROOT, name)).read()


def test_samples_entry_point_argument_checks():
    lib = _lib.load()
    p = C.c_void_p(256)                                      # never dereferenced: every call below returns before a launch
    good = dict(nx=40, ny=30, n_fields=2, n=7, reach=5, max_steps=9, window=12)

    def call(dist=p, starts=p, field=p, goals=p, cells=p, origins=p, summary=p, samples=p, **kw):
        a = dict(good, **kw)
        return lib.mmd_grid_window_goal_samples(dist, a["nx"], a["ny"], a["n_fields"], starts, field, goals, a["n"], a["reach"], a["max_steps"],
                                                a["window"], cells, origins, summary, samples, None)
    assert call(n=0) == 0
    assert call(n=0, dist=None, starts=None, field=None, goals=None, cells=None, origins=None, summary=None, samples=None) == 0
    for kw, word in ((dict(nx=0), "grid"), (dict(ny=2049), "grid"), (dict(n_fields=-1), "n_fields"), (dict(n=-1), "n_queries"),
                     (dict(n=2 ** 31 - 1), "n_queries"), (dict(reach=0), "reach"), (dict(reach=6), "reach"), (dict(max_steps=0), "max_steps"),
                     (dict(window=31), "window"), (dict(window=0), "window"), (dict(window=3, reach=1), "reach"), (dict(n=0, reach=0), "reach"),
                     (dict(dist=None), "NULL dist"), (dict(goals=None), "NULL goals"), (dict(starts=None), "NULL starts"),
                     (dict(field=None), "NULL field"), (dict(cells=None), "NULL cells"), (dict(origins=None), "NULL origins"),
                     (dict(summary=None), "NULL summary"), (dict(samples=None), "NULL samples")):
        assert call(**kw) == 2, kw
        err = lib.mmd_last_error()
        assert err.startswith(b"mmd_grid_window_goal_samples:") and word.encode() in err, (kw, err)


def test_seeds_entry_point_argument_checks():
    lib = _lib.load()
    p = C.c_void_p(256)
    two = lambda a, b: (C.c_float * 2)(a, b)                                             # noqa: E731
    good = dict(nx=40, ny=30, lo=two(2.0, 2.0), hi=two(2.2, 2.15), clearance=0.16, n=3, window=12, iters=4, two_dt=0.15)

    def call(grid=p, samples=p, origins=p, summary=p, starts=p, goals=p, seeds=p, clear_min=p, **kw):
        a = dict(good, **kw)
        return lib.mmd_window_seeds(grid, a["nx"], a["ny"], a["lo"], a["hi"], a["clearance"], samples, origins, summary, a["n"], a["window"],
                                    starts, goals, a["iters"], a["two_dt"], seeds, clear_min, None)
    assert call(n=0) == 0
    assert call(n=0, grid=None, samples=None, origins=None, summary=None, starts=None, goals=None, seeds=None, clear_min=None) == 0
    inf, nan = float("inf"), float("nan")
    for kw, word in ((dict(nx=0), "grid"), (dict(ny=2049), "grid"), (dict(lo=None), "NULL limits"), (dict(hi=None), "NULL limits"),
                     (dict(hi=two(2.0, 2.15)), "limits"), (dict(lo=two(nan, 2.0)), "limits"), (dict(hi=two(inf, 2.15)), "limits"),
                     (dict(clearance=nan), "clearance"), (dict(clearance=inf), "clearance"), (dict(two_dt=0.0), "two_dt"),
                     (dict(two_dt=-1.0), "two_dt"), (dict(two_dt=nan), "two_dt"), (dict(two_dt=inf), "two_dt"), (dict(iters=-1), "smooth_iters"),
                     (dict(n=-1), "n_robots"), (dict(window=0), "window"), (dict(n=0, window=0), "window"), (dict(grid=None), "NULL grid"),
                     (dict(samples=None), "NULL samples"), (dict(origins=None), "NULL origins"), (dict(summary=None), "NULL summary"),
                     (dict(starts=None), "NULL start"), (dict(goals=None), "NULL start or goal"), (dict(seeds=None), "NULL seeds"),
                     (dict(clear_min=None), "NULL clear_min")):
        assert call(**kw) == 2, kw
        err = lib.mmd_last_error()
        assert err.startswith(b"mmd_window_seeds:") and word.encode() in err, (kw, err)
