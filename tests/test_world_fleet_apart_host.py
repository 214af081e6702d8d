"""CPU: sub-goals kept apart (mmd_amd.world_fleet.subgoals_apart) -- the fact (starts pairwise sep apart give chosen cells pairwise sep
apart, every clear 1) by brute force over whole runs of 24 robots on the written-out grids of 40 x 30 cells, the sweeps against the
definition, the written-out chain, the queries that take no part, starts already in conflict, the argument checks of the two C entry
points, which answer before any launch, and the fleet's refusals and defaults."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import world_fleet_apart_model as A
import world_fleet_model as M
from mmd_amd import _lib, environments as E, world_fleet as F
from mmd_amd.multi_agent import RR_MARGIN
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACH, WINDOW, SEP = M.REACH, M.WINDOW, A.SEP
ARGS = (REACH, 100, SEP, WINDOW)                             # reach, max_steps, sep, window


def sweeps_to_fixed_point(dist, starts, which, goals, limit=40):
    for n in range(limit):
        out = F.subgoals_apart_sweeps(dist, starts, which, goals, REACH, 100, SEP, n, WINDOW)
        if out[4] == 0:
            return n, out
    raise AssertionError("no fixed point")


# ---- 1. the fact ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(A.GRIDS))
def test_chosen_cells_stay_apart_over_whole_runs(grid):
    dist, starts, which, goals = A.batch(grid)
    assert A.apart(starts) >= SEP * SEP and A.apart(goals) >= SEP * SEP
    epochs = A.run_apart(dist, starts, which, goals)
    assert len(epochs) >= 2
    held = zero = 0
    plain_min = []
    for e, (at, plain, (cells, origins, summary, extra)) in enumerate(epochs):
        assert A.apart(at) >= SEP * SEP, e                   # the ends of one epoch are the starts of the next
        assert A.apart(cells) >= SEP * SEP, f"epoch {e}: two chosen cells closer than {SEP}"
        assert (extra[:, 1] == 1).all(), e
        k, walked = summary[:, 0], extra[:, 0]
        assert np.array_equal(walked, plain[2][:, 0]) and ((0 <= k) & (k <= walked)).all() and np.array_equal(origins, plain[1])
        d0 = plain[2][:, 0] + plain[2][:, 1]
        assert np.array_equal(summary[:, 1], d0 - k) and np.array_equal(summary[:, 3], (d0 == k).astype(np.int32))
        assert all(dist[r][tuple(cells[r])] == summary[r, 1] for r in range(len(at)))
        held += int(((k > 0) & (k < walked)).sum())
        zero += int(((k == 0) & (walked > 0)).sum())
        plain_min.append(A.apart(plain[0]))
    # the rule at work, in the first epoch already (the seeds of world_fleet_apart_model were chosen for it)
    k, walked = epochs[0][2][2][:, 0], epochs[0][2][3][:, 0]
    assert ((k > 0) & (k < walked)).any() and ((k == 0) & (walked > 0)).any() and plain_min[0] < SEP * SEP
    assert held >= 7 and zero >= 1 and min(plain_min) <= 4
    # termination: in every epoch but the last some robot moves and its remaining falls; the last is all arrived, or stalled with every
    # k = 0, and one more epoch from its cells repeats it word for word
    for (_, _, a), (_, _, b) in zip(epochs, epochs[1:]):
        assert np.array_equal(b[2][:, 0] + b[2][:, 1], a[2][:, 1]) and (a[2][:, 0] > 0).any() and not A.stalled(a[2])
    at, _, last = epochs[-1]
    arrived = last[2][:, 3] == 1
    assert arrived.all() or (A.stalled(last[2]) and not last[2][:, 0].any() and np.array_equal(last[0], at))
    if not arrived.all():
        assert all(np.array_equal(a, b) for a, b in zip(F.subgoals_apart(dist, last[0], which, goals, *ARGS), last))
    print(f"{grid}: {len(epochs)} epochs, {int(arrived.sum())} of {len(at)} arrived, stalled {A.stalled(last[2])}, held back {held}, to k = 0 {zero}")


def test_a_robot_that_arrives_moves_and_the_epoch_is_not_stalled():
    """Robot 0 is held at k = 0 by the start of robot 1, which walks 4 cells onto its goal in the same epoch: every robot that is off its
    goal has k = 0, and yet the state does not repeat -- robot 1's start cell was the blocker, and it has moved."""
    goals = [(20, 15), (13, 19)]
    dist = M.fields(M.open_grid(), goals)
    starts, which = np.asarray([(10, 15), (13, 15)], np.int32), [0, 1]
    first = F.subgoals_apart(dist, starts, which, goals, *ARGS)
    assert first[2].tolist() == [[0, 10, ROUTE_OK, 0], [4, 0, ROUTE_OK, 1]] and first[3].tolist() == [[5, 1], [4, 1]]
    assert not A.stalled(first[2])
    epochs = A.run_apart(dist, starts, which, goals)
    assert [e[2][2][:, 0].tolist() for e in epochs] == [[0, 4], [5, 0], [5, 0]]
    assert (epochs[-1][2][2][:, 3] == 1).all() and not any(A.stalled(e[2][2]) for e in epochs)
    assert epochs[-1][2][0].tolist() == [[20, 15], [13, 19]]
    # the rule on written-out summaries: stalled iff every k is 0 and some robot is off its goal
    held = np.asarray([[0, 3, ROUTE_OK, 0], [0, 0, ROUTE_OK, 1]], np.int32)
    assert A.stalled(held) and not A.stalled(np.asarray([[0, 0, ROUTE_OK, 1]] * 2, np.int32))
    assert not A.stalled(np.asarray([[0, 3, ROUTE_OK, 0], [2, 0, ROUTE_OK, 1]], np.int32))


@pytest.mark.parametrize("grid", list(A.GRIDS))
def test_sweeps_reach_the_definition(grid):
    dist, starts, which, goals = A.batch(grid)
    want = F.subgoals_apart(dist, starts, which, goals, *ARGS)
    n, out = sweeps_to_fixed_point(dist, starts, which, goals)
    assert 3 <= n <= A.N_ROBOTS + 1                          # at least 2 sweeps that move a k, and the one that reads 0
    assert all(np.array_equal(a, b) for a, b in zip(out[:4], want))
    before = F.subgoals_apart_sweeps(dist, starts, which, goals, REACH, 100, SEP, n - 1, WINDOW)
    assert before[4] > 0 and np.array_equal(before[2], want[2])          # the sweep before moved a k onto the fixed point
    zero = F.subgoals_apart_sweeps(dist, starts, which, goals, REACH, 100, SEP, 0, WINDOW)
    plain = F.window_goals(dist, starts, which, goals, REACH, 100, WINDOW)
    assert all(np.array_equal(a, b) for a, b in zip(zero[:3], plain)) and zero[4] == A.N_ROBOTS and not zero[3][:, 1].any()
    samples = F.subgoals_apart_samples(dist, starts, which, goals, *ARGS)
    assert all(np.array_equal(a, b) for a, b in zip(samples[:4], want))
    assert np.array_equal(F.subgoals_apart_sweeps(dist, starts, which, goals, REACH, 100, SEP, n, WINDOW, with_samples=True)[5], samples[4])
    for r in range(A.N_ROBOTS):
        k = int(want[2][r, 0])
        assert samples[4][r, 0].tolist() == starts[r].tolist() and samples[4][r, 63].tolist() == want[0][r].tolist()
        walk = F.window_goal_samples(dist[r], starts[r], goals[r], REACH, k, WINDOW)[5] if k else np.tile(starts[r], (64, 1))
        assert np.array_equal(samples[4][r], walk)           # window_goal_samples' spacing on the walk cut at k


def test_the_chain_written_out():
    dist, starts, which, goals = A.chain()
    plain = F.window_goals(dist, starts, which, goals, REACH, 100, WINDOW)
    assert plain[2][:, 0].tolist() == [5, 5, 5, 5, 5, 5, 5, 0]
    ks, changed = [], []
    for n in range(1, 7):
        out = F.subgoals_apart_sweeps(dist, starts, which, goals, REACH, 100, SEP, n, WINDOW)
        ks.append(out[2][:, 0].tolist())
        changed.append(out[4])
        assert out[3][:, 0].tolist() == [5, 5, 5, 5, 5, 5, 5, 0]
    assert ks == A.CHAIN_K and changed == A.CHAIN_CHANGED
    cells, _, summary, extra = F.subgoals_apart(dist, starts, which, goals, *ARGS)
    assert cells[:, 0].tolist() == A.CHAIN_X and (cells[:, 1] == 10).all() and summary[:, 0].tolist() == A.CHAIN_K[-1]
    assert (extra[:, 1] == 1).all() and summary[7].tolist() == [0, 0, ROUTE_OK, 1]


# ---- 2. what the rule leaves alone ---------------------------------------------------------------------------------------------------------------
def test_far_apart_starts_give_window_goals():
    goals = [(20, 15), (0, 0), (39, 29), (7, 22)]
    dist = M.fields(M.open_grid(), goals)
    starts, which = [(2, 27), (30, 3), (5, 5), (36, 20), (20, 15)], [0, 1, 2, 3, 0]
    plain = F.window_goals(dist, starts, which, goals, REACH, 100, WINDOW)
    assert A.apart(plain[0]) >= 100
    out = F.subgoals_apart(dist, starts, which, goals, *ARGS)
    assert all(np.array_equal(a, b) for a, b in zip(out[:3], plain))
    assert np.array_equal(out[3][:, 0], plain[2][:, 0]) and (out[3][:, 1] == 1).all()
    swept = F.subgoals_apart_sweeps(dist, starts, which, goals, REACH, 100, SEP, 1, WINDOW)
    assert swept[4] == 0 and all(np.array_equal(a, b) for a, b in zip(swept[:4], out))


def test_queries_that_are_not_ok_take_no_part():
    stuck, goal0, sticks_at = M.unconverged_field()
    walled = M.fields(M.door_grid(door=(0, 0)), [(25, 5)])
    dist = np.concatenate([stuck, M.fields(M.open_grid(), [(20, 15), (22, 15)]), walled])
    goals = [goal0, (20, 15), (22, 15), (25, 5)]
    # robots 0 and 2 walk towards one another; between and behind them an outside start, a start on an unreached cell on robot 0's walk,
    # a stuck walk, and a field index outside on robot 0's walk
    starts = [(14, 15), (-1, 3), (28, 15), (15, 15), (10, 12), (16, 15)]
    which = [1, 1, 2, 3, 0, 7]
    plain = F.window_goals(dist, starts, which, goals, REACH, 100, WINDOW)
    assert plain[2][:, 2].tolist() == [ROUTE_OK, ROUTE_OUTSIDE, ROUTE_OK, ROUTE_UNREACHED, ROUTE_STUCK, ROUTE_OUTSIDE]
    out = F.subgoals_apart(dist, starts, which, goals, *ARGS)
    odd = [1, 3, 4, 5]
    for a, b in zip(out[:3], plain):
        assert np.array_equal(a[odd], b[odd])
    assert out[3][odd].tolist() == [[-1, 0], [-1, 0], [2, 0], [-1, 0]]
    assert plain[0][[0, 2]].tolist() == [[19, 15], [23, 15]] and out[0][[0, 2]].tolist() == [[19, 15], [23, 15]]      # 4 apart: both keep their walks
    keep = [0, 2]
    alone = F.subgoals_apart(dist, [starts[q] for q in keep], [which[q] for q in keep], goals, *ARGS)
    assert all(np.array_equal(a[keep], b) for a, b in zip(out, alone))
    # robot 2 two cells nearer and bound for robot 0's goal: now it is held back, and the odd queries change nothing about that
    starts[2], which[2] = (26, 15), 1
    out = F.subgoals_apart(dist, starts, which, goals, *ARGS)
    alone = F.subgoals_apart(dist, [starts[q] for q in keep], [which[q] for q in keep], goals, *ARGS)
    assert all(np.array_equal(a[keep], b) for a, b in zip(out, alone)) and out[2][2, 0] == 4 and out[3][2].tolist() == [5, 1]
    samples = F.subgoals_apart_samples(dist, starts, which, goals, *ARGS)[4]
    assert not samples[odd].any() and samples[2, 63].tolist() == [22, 15]


def test_starts_already_in_conflict():
    goals = [(20, 15), (22, 15)]
    dist = M.fields(M.open_grid(), goals)
    out = F.subgoals_apart(dist, [(10, 15), (11, 15), (10, 16)], [0, 1, 0], goals, *ARGS)
    assert (out[2][:, 2] == ROUTE_OK).all() and out[3][:, 0].tolist() == [5, 5, 5]
    assert 0 in out[3][:, 1].tolist() and (out[2][out[3][:, 1] == 0, 0] == 0).all()       # clear is 0 only with k = 0
    n, swept = sweeps_to_fixed_point(dist, [(10, 15), (11, 15), (10, 16)], [0, 1, 0], goals)
    assert n <= 4 and all(np.array_equal(a, b) for a, b in zip(swept[:4], out))
    for sep in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError, match="sep"):
            F.subgoals_apart(dist, [(10, 15)], [0], goals, REACH, 100, sep, WINDOW)
    with pytest.raises(ValueError, match="n_sweeps"):
        F.subgoals_apart_sweeps(dist, [(10, 15)], [0], goals, REACH, 100, SEP, -1, WINDOW)
    one = F.subgoals_apart(dist, [(10, 15), (11, 15)], [0, 1], goals, REACH, 100, 1, WINDOW)      # sep 1: only the same cell conflicts
    assert one[2][:, 0].tolist() == [5, 5] and (one[3][:, 1] == 1).all()


# ---- 3. the C entry points answer before any launch ------------------------------------------------------------------------------------------------
def test_entry_point_argument_checks():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mmd_amd.h")).read()
    for name, n_args in (("mmd_grid_window_apart_work_bytes", 2), ("mmd_grid_window_goals_apart", 23)):
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == n_args and f" {name}(" in header
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9                           # two additive symbols under v9
    for name in ("build.sh", "__graft_entry__.py"):
        assert "mmd_amd/csrc/window_apart.hip" in open(os.path.join(ROOT, name)).read()
    size = lib.mmd_grid_window_apart_work_bytes
    assert size(7, 9) >= 7 * (10 * 8 + 4 * 4) and size(1, 1) > 0 and size(0, 9) == 0 and size(24, 4095) >= 24 * 4096 * 8
    assert size(-1, 9) == 0 and size(7, 0) == 0 and size(7, 4096) == 0 and size(2 ** 31 - 1, 9) == 0
    assert size(2 ** 31 - 65, 4095) > 2 ** 45                # computed in size_t
    p = C.c_void_p(256)                                      # never dereferenced: every call below returns before a launch
    good = dict(nx=40, ny=30, n_fields=2, n=7, reach=5, max_steps=9, window=12, sep=3, restart=1, n_sweeps=4, work_bytes=size(7, 9))

    def call(dist=p, starts=p, field=p, goals=p, work=p, cells=p, origins=p, summary=p, extra=p, samples=p, changed=p, **kw):
        a = dict(good, **kw)
        return lib.mmd_grid_window_goals_apart(dist, a["nx"], a["ny"], a["n_fields"], starts, field, goals, a["n"], a["reach"], a["max_steps"],
                                               a["window"], a["sep"], a["restart"], a["n_sweeps"], work, a["work_bytes"], cells, origins,
                                               summary, extra, samples, changed, None)
    assert call(n=0) == 0 and call(n=0, dist=None, starts=None, field=None, goals=None, work=None, work_bytes=0, cells=None, origins=None,
                                   summary=None, extra=None, samples=None, changed=None) == 0
    for kw, word in ((dict(nx=0), "grid"), (dict(ny=2049), "grid"), (dict(n_fields=-1), "n_fields"), (dict(n=-1), "n_queries"),
                     (dict(reach=0), "reach"), (dict(reach=6), "reach"), (dict(max_steps=0), "max_steps"), (dict(window=31), "window"),
                     (dict(window=0), "window"), (dict(window=3, reach=1), "reach"), (dict(n=0, reach=0), "reach"),
                     (dict(max_steps=4096, work_bytes=2 ** 40), "max_steps"), (dict(sep=0), "sep"), (dict(sep=-3), "sep"), (dict(sep=1025), "sep"),
                     (dict(n=0, sep=0), "sep"), (dict(n_sweeps=-1), "n_sweeps"), (dict(n=0, n_sweeps=-1), "n_sweeps"),
                     (dict(dist=None), "NULL dist"), (dict(goals=None), "NULL goals"), (dict(starts=None), "NULL starts"),
                     (dict(field=None), "NULL field"), (dict(work=None), "workspace"), (dict(work=C.c_void_p(264)), "aligned"),
                     (dict(work_bytes=size(7, 9) - 1), "workspace"), (dict(work_bytes=0), "workspace"),
                     (dict(n=8), "workspace"), (dict(max_steps=10), "workspace"),
                     (dict(cells=None), "NULL cells"), (dict(origins=None), "NULL origins"), (dict(summary=None), "NULL summary"),
                     (dict(extra=None), "NULL extra"), (dict(changed=None), "NULL changed")):
        assert call(**kw) == 2, kw
        assert lib.mmd_last_error().startswith(b"mmd_grid_window_goals_apart:") and word.encode() in lib.mmd_last_error(), \
            (kw, lib.mmd_last_error())


def test_entry_point_and_wrapper_check_order_with_two_faults():
    """the order of the checks, which a caller with two faults sees: ranges (the shared ones, then sep and n_sweeps), the input pointers,
    the workspace, the output pointers; in the wrapper dist, the walk's arguments, sep, then the cap and the sweeps"""
    import torch
    lib, p = _lib.load(), C.c_void_p(256)
    size = lib.mmd_grid_window_apart_work_bytes(7, 9)

    def call(sep=3, n_sweeps=4, field=p, work=p, cells=p, extra=p):
        assert lib.mmd_grid_window_goals_apart(p, 40, 30, 2, p, field, p, 7, 5, 9, 12, sep, 1, n_sweeps, work, size, cells, p, p, extra, p, p,
                                               None) == 2
        return lib.mmd_last_error()
    for kw, word in ((dict(sep=0, cells=None), b"sep"), (dict(n_sweeps=-1, field=None), b"n_sweeps"), (dict(work=None, cells=None), b"workspace"),
                     (dict(field=None, work=None), b"NULL field"), (dict(cells=None, extra=None), b"NULL cells")):
        assert word in call(**kw), (kw, call(**kw))
    dist = torch.zeros(1, 40, 30, dtype=torch.int32)         # on the CPU: the first refusal, whatever else is wrong
    with pytest.raises(ValueError, match="dist must be a contiguous int32"):
        F.device_subgoals_apart(dist, [[1, 1]], [0], [[2, 2]], 5, 5000, 0, window=12, sweeps=0)


# ---- 4. the fleet's refusals and defaults ------------------------------------------------------------------------------------------------------------
def test_fleet_refusals_and_defaults():
    assert inspect.signature(F.WorldFleet.__init__).parameters["separation"].default is None
    # the least separation that keeps two end points RR_MARGIN apart, each anywhere in its cell: centres sep cells apart leave the points
    # at least sep - sqrt(2) cells apart (half a cell's diagonal off each centre)
    assert F.SUBGOAL_SEPARATION == 23 and abs(RR_MARGIN - 0.105) < 1e-12 and E.SDF_CELL_SIZE == 0.005
    assert (23 - 2 ** 0.5) * E.SDF_CELL_SIZE >= RR_MARGIN > (22 - 2 ** 0.5) * E.SDF_CELL_SIZE
    name = "ApartRefusals"
    E.register_world_map(name, np.zeros((800, 400), np.uint8), origin=(2.0, 2.0))
    try:
        at = lambda cells: (2.0 + (np.asarray(cells) + 0.5) * E.SDF_CELL_SIZE).astype(np.float32)                      # noqa: E731
        starts, goals = at([(100, 100), (300, 100), (500, 100)]), at([(100, 300), (300, 300), (500, 300)])
        near = at([(100, 100), (300, 100), (316, 116)])      # 16^2 + 16^2 = 512 < 23^2 = 529
        with pytest.raises(ValueError, match="start cells of robots 1 and 2.*closer than separation = 23"):
            F.WorldFleet(None, name, near, goals, device="cpu", separation=23)
        with pytest.raises(ValueError, match=r"goal cells of robots 1 and 2.*\[300, 100\] and \[316, 116\]"):
            F.WorldFleet(None, name, goals, near, device="cpu", separation=F.SUBGOAL_SEPARATION)
        for separation in (0, -1, 2.5, 1025):
            with pytest.raises(ValueError, match="separation"):
                F.WorldFleet(None, name, starts, goals, device="cpu", separation=separation)
        with pytest.raises(ValueError, match="max_steps"):
            F.WorldFleet(None, name, starts, goals, device="cpu", separation=23, max_steps=4096)
    finally:
        E.unregister_world_map(name)
