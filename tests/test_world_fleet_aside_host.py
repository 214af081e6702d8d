"""CPU: standing robots step aside (mmd_amd.world_fleet.subgoals_aside) -- safety and containment by brute force over whole runs of 24
robots on the written-out grids, the written-out cases word for word, the effect of the rule as conditions on recorded seeds, the
argument checks of the two C entry points, which answer before any launch, and the fleet's refusals and defaults."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import world_fleet_apart_model as A
import world_fleet_aside_model as S
import world_fleet_model as M
from mmd_amd import _lib, environments as E, world_fleet as F
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP = S.SEP
HELD, YIELDS, MOVED, RELEASED = S.HELD, S.YIELDS, S.MOVED, S.RELEASED


conflict, roles_by_hand = S.conflict, S.roles_by_hand


def check_epoch(dist, at, which, goals, args, out, what):
    """SAFETY, CONTAINMENT and the consistency of the five arrays of one epoch from starts pairwise sep apart"""
    reach, max_steps, sep, aside_reach, aside_steps, window = args
    cells, origins, summary, extra, aside = out
    bits, l = aside[:, 0], aside[:, 1]
    apart = F.subgoals_apart(dist, at, which, goals, reach, max_steps, sep, window)
    held, clears, paths = roles_by_hand(dist, at, which, goals, args)
    assert A.apart(at, sep) >= sep * sep, what
    assert A.apart(cells, sep) >= sep * sep, f"{what}: two final cells closer than {sep}"
    assert np.array_equal(origins, apart[1]) and np.array_equal(extra, apart[3]), what
    assert not ((bits & MOVED != 0) & (bits & RELEASED != 0)).any(), f"{what}: a robot that moved aside was released"
    assert ((bits & MOVED != 0) <= (bits & YIELDS != 0)).all() and ((bits & RELEASED != 0) <= (bits & HELD != 0)).all(), what
    assert np.array_equal(bits & HELD != 0, held) and np.array_equal(bits & YIELDS != 0, [bool(c) for c in clears]), what
    assert np.array_equal(l > 0, bits & MOVED != 0), what
    moved = np.flatnonzero(bits & MOVED)
    for q in range(len(at)):
        own = dist[which[q]]
        assert own[tuple(cells[q])] == summary[q, 1] and summary[q, 2] == ROUTE_OK and summary[q, 3] == int(summary[q, 1] == 0), (what, q)
        if bits[q] & MOVED:
            d = np.abs(cells[q].astype(int) - at[q])
            assert 1 <= l[q] <= aside_steps and l[q] == summary[q, 0] and d.max() <= aside_reach and d.sum() <= l[q], (what, q)
            assert ((cells[q] >= origins[q]) & (cells[q] < origins[q] + window)).all(), f"{what}: robot {q}'s side cell is outside its window"
            for r in clears[q]:                              # the walk it cleared no longer conflicts with its place
                assert not any(conflict(cells[q], c, sep) for c in paths[r]), (what, q, r)
        elif bits[q] & RELEASED:
            assert tuple(cells[q]) == paths[q][summary[q, 0]] and any(q in clears[j] for j in moved), (what, q)
        else:
            assert np.array_equal(cells[q], apart[0][q]) and np.array_equal(summary[q], apart[2][q]), (what, q)
    for r in range(len(at)):                                 # released is exactly: held, not moved, cleared by a robot that moved
        assert bool(bits[r] & RELEASED) == (held[r] and not bits[r] & MOVED and any(r in clears[j] for j in moved)), (what, r)


# ---- 1. the facts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(A.GRIDS))
def test_safety_and_containment_over_whole_runs(grid):
    counts = np.zeros(4, int)
    for seed in (None, 3, 4):
        dist, starts, which, goals = A.batch(grid, seed)
        end, epochs = S.run_aside(dist, starts, which, goals, cap=60)
        for e, (at, out) in enumerate(epochs):
            check_epoch(dist, at, which, goals, S.ARGS, out, f"{grid} seed {seed} epoch {e}")
            counts += [int((out[4][:, 0] & bit != 0).sum()) for bit in (HELD, YIELDS, MOVED, RELEASED)]
            if e:
                assert np.array_equal(at, epochs[e - 1][1][0])
        print(f"{grid} seed {seed}: {end} after {len(epochs)} epochs")
    print(f"{grid}: held, yields, moved, released = {counts.tolist()}")
    assert (counts >= 10).all()                              # the rule was at work


# ---- 2. the written-out cases ---------------------------------------------------------------------------------------------------------------------
def test_the_two_robot_case_written_out():
    dist, starts, which, goals, args = S.two_robots()
    assert F.subgoals_apart(dist, starts, which, goals, M.REACH, 100, SEP, M.WINDOW)[2][:, 0].tolist() == [0, 0]
    end, epochs = S.run_aside(dist, starts, which, goals, step_aside=False)
    assert end == "stalled" and len(epochs) == 1             # without the rule: stalled for ever
    end, epochs = S.run_aside(dist, starts, which, goals)
    assert end == "arrived" and [[tuple(c) for c in out[0].tolist()] for _, out in epochs] == S.TWO_ROBOT_CELLS
    first = epochs[0][1]
    assert first[2].tolist() == [[1, 1, ROUTE_OK, 0], [5, 19, ROUTE_OK, 0]] and first[3].tolist() == [[0, 1], [5, 1]]
    assert first[4].tolist() == [[YIELDS | MOVED, 1], [HELD | RELEASED, 0]]
    # epoch 1: robot 0 is held one cell off its goal by robot 1's start, which robot 1 leaves; it walks back in epoch 2
    assert [out[4].tolist() for _, out in epochs[1:]] == [[[HELD, 0], [0, 0]], [[0, 0], [0, 0]], [[0, 0], [0, 0]]]
    assert [out[2][:, 0].tolist() for _, out in epochs] == [[1, 5], [0, 5], [1, 6], [0, 8]]
    for e, (at, out) in enumerate(epochs):
        check_epoch(dist, at, which, goals, args, out, f"epoch {e}")


def test_a_held_robot_yields_to_a_lower_index_only():
    """head on: each holds the other; robot 1 yields to robot 0 and robot 0, held as well, does not yield to robot 1.  The side cell is 3
    steps off the row, where it is 3 cells from the cell of robot 0's walk under robot 1's start; robot 0, released, takes its whole walk."""
    cells, _, summary, extra, aside = S.aside(S.head_on())
    assert aside.tolist() == [[HELD | RELEASED, 0], [HELD | YIELDS | MOVED, 3]] and extra.tolist() == [[5, 1], [5, 1]]
    assert cells.tolist() == [[15, 15], [13, 12]] and summary.tolist() == [[5, 15, ROUTE_OK, 0], [3, 16, ROUTE_OK, 0]]
    dist, starts, which, goals, args = S.head_on()
    back = F.subgoals_aside(dist[::-1], starts[::-1], which, goals[::-1], *args)         # the same two robots with their indices exchanged
    assert back[4].tolist() == [[HELD | RELEASED, 0], [HELD | YIELDS | MOVED, 3]] and back[0].tolist() == [[8, 15], [10, 12]]


def test_ties_on_l_are_broken_by_the_own_field_then_ix_then_iy():
    # (13, 12) and (13, 18) are both 3 steps away and hold 16 in robot 1's field of the goal (0, 15): the lesser iy
    assert S.aside(S.head_on())[0][1].tolist() == [13, 12]
    # with the goal (0, 20) they hold 21 and 15: the own field decides, against iy
    out = S.aside(S.head_on((0, 20)))
    assert out[0][1].tolist() == [13, 18] and out[2][1].tolist() == [3, 15, ROUTE_OK, 0]
    # in columns the two cells are (17, 13) and (23, 13), both hold 16: the lesser ix
    out = S.aside(S.head_on_columns())
    assert out[0].tolist() == [[20, 15], [17, 13]] and out[4].tolist() == [[HELD | RELEASED, 0], [HELD | YIELDS | MOVED, 3]]


@pytest.mark.parametrize("name", ["too few steps", "boxed in", "border, blocked"])
def test_a_yielder_with_no_candidate_stays_and_releases_nobody(name):
    dist, starts, which, goals, args = S.HOST_CASES[name]()
    out = F.subgoals_aside(dist, starts, which, goals, *args)
    apart = F.subgoals_apart(dist, starts, which, goals, args[0], args[1], args[2], args[5])
    assert all(np.array_equal(a, b) for a, b in zip(out[:4], apart)) and np.array_equal(out[0][:2], starts[:2])
    assert not (out[4][:, 0] & (MOVED | RELEASED)).any() and not out[4][:, 1].any()
    yielder = 0 if name == "boxed in" else 1
    assert out[4][yielder, 0] & YIELDS and out[4][1 - yielder, 0] == HELD and not out[4][2:].any()
    # and the same robots with the obstruction taken away: it moves, and the robot it held walks
    free = {"too few steps": S.head_on, "border, blocked": lambda: S.at_the_border(False),
            "boxed in": lambda: S.case(goals[:2], starts[:2], aside_reach=3)}[name]()
    out = S.aside(free)
    assert out[4][yielder].tolist() == [(HELD if yielder else 0) | YIELDS | MOVED, 3] and out[4][1 - yielder].tolist() == [HELD | RELEASED, 0]
    if name == "border, blocked":
        assert out[0][1].tolist() == [13, 4]                  # (13, -2) is no cell
    check_epoch(*free, out, name)


def test_a_robot_that_moved_aside_is_not_released():
    dist, starts, which, goals, args = S.moved_not_released()
    held, clears, _ = roles_by_hand(dist, starts, which, goals, args)
    out = F.subgoals_aside(dist, starts, which, goals, *args)
    assert out[4].tolist() == [[HELD | RELEASED, 0], [HELD | YIELDS | MOVED, 3], [HELD | YIELDS | MOVED, 4], [0, 0], [0, 0]]
    assert 1 in clears[2] and held[1]                        # robot 2 moved and had robot 1 in its way: robot 1 moved itself, so it stays put
    assert out[0].tolist() == [[13, 16], [11, 13], [14, 19], [17, 17], [16, 4]]
    check_epoch(dist, starts, which, goals, args, out, "moved, not released")


def test_queries_that_take_no_part_keep_window_goals_words():
    dist, starts, which, goals, args = S.every_status()
    plain = F.window_goals(dist, starts, which, goals, M.REACH, 100, M.WINDOW)
    assert plain[2][:, 2].tolist() == [ROUTE_OK, ROUTE_OUTSIDE, ROUTE_OK, ROUTE_UNREACHED, ROUTE_STUCK, ROUTE_OUTSIDE]
    out = F.subgoals_aside(dist, starts, which, goals, *args)
    odd = [1, 3, 4, 5]
    for a, b in zip(out[:3], plain):
        assert np.array_equal(a[odd], b[odd])
    assert out[3][odd].tolist() == [[-1, 0], [-1, 0], [2, 0], [-1, 0]] and not out[4][odd].any()
    alone = S.aside(S.two_robots())                          # the odd queries stand on robot 1's walk and block nobody
    assert all(np.array_equal(a[[0, 2]], b) for a, b in zip(out, alone)) and out[4][[0, 2]].tolist() == [[YIELDS | MOVED, 1], [HELD | RELEASED, 0]]


def test_definition_refusals():
    dist, starts, which, goals, args = S.two_robots()
    for kw in (dict(aside_reach=0), dict(aside_reach=6), dict(aside_reach=2.5), dict(aside_steps=0), dict(aside_steps=4096), dict(sep=0)):
        a = dict(zip(("reach", "max_steps", "sep", "aside_reach", "aside_steps", "window"), args), **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            F.subgoals_aside(dist, starts, which, goals, **a)
    big = M.fields(np.ones((200, 200), bool), [(5, 5)])
    with pytest.raises(ValueError, match="aside_reach = 64"):                             # min(reach, 63)
        F.subgoals_aside(big, [(9, 9)], [0], [(5, 5)], 99, 100, 3, 64, 10, 200)
    assert F.subgoals_aside(big, [(9, 9)], [0], [(5, 5)], 99, 100, 3, 63, 4095, 200)[4].tolist() == [[0, 0]]


# ---- 3. the effect, as conditions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(13))
def test_open_batches_arrive_with_the_rule_and_stall_without_it(seed):
    batch = A.batch("open", seed)
    end, epochs = S.run_aside(*batch, step_aside=False)
    assert end == "stalled" and not (epochs[-1][1][2][:, 3] == 1).all()
    end, epochs = S.run_aside(*batch, cap=40)
    assert end == "arrived" and len(epochs) <= 40 and (epochs[-1][1][2][:, 1] == 0).all()


def test_the_real_scale_instance_arrives_with_the_rule():
    """32 robots on an open grid of 400 x 400 cells at the fleet's own scale (sep 23, reach 180, 360 steps): the seed is the first whose
    run stalls under the separation alone (S.REAL_SEED), with 3 robots stranded"""
    batch = S.real_scale(S.REAL_SEED)
    end, epochs = S.run_aside(*batch, S.REAL_ARGS, step_aside=False)
    assert end == "stalled" and int((epochs[-1][1][2][:, 3] == 0).sum()) == S.REAL_STRANDED
    end, epochs = S.run_aside(*batch, S.REAL_ARGS, cap=12)
    assert end == "arrived"
    for e, (at, out) in enumerate(epochs):
        assert A.apart(out[0], 23) >= 23 * 23, e
    assert sum(int((out[4][:, 0] & MOVED != 0).sum()) for _, out in epochs) >= 1


# ---- 4. the C entry points answer before any launch ------------------------------------------------------------------------------------------------
def test_entry_point_argument_checks():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mmd_amd.h")).read()
    for name, n_args in (("mmd_grid_window_aside_work_bytes", 1), ("mmd_grid_window_goals_aside", 25)):
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == n_args and f" {name}(" in header
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9                           # two additive symbols under v9
    assert (_lib.WINDOW_ASIDE_MAX_REACH, _lib.WINDOW_ASIDE_MAX_STEPS) == (63, 4095)
    assert "#define MMD_WINDOW_ASIDE_MAX_REACH 63" in header and "#define MMD_WINDOW_ASIDE_MAX_STEPS 4095" in header
    for name in ("build.sh", "__graft_entry__.py"):
        assert "mmd_amd/csrc/window_aside.hip" in open(os.path.join(ROOT, name)).read()
    size = lib.mmd_grid_window_aside_work_bytes
    assert size(7) >= 7 * 36 and size(1) > 0 and size(0) == 0 and size(-1) == 0 and size(2 ** 31 - 1) == 0
    assert size(2 ** 31 - 65) > 2 ** 35                      # computed in size_t
    p = C.c_void_p(256)                                      # never dereferenced: every call below returns before a launch
    apart_size = lib.mmd_grid_window_apart_work_bytes
    good = dict(nx=40, ny=30, n_fields=2, n=7, reach=5, max_steps=9, window=12, sep=3, aside_reach=5, aside_steps=10, restart=1, n_sweeps=4,
                apart_bytes=apart_size(7, 9), work_bytes=size(7))

    def call(dist=p, field=p, apart=p, work=p, cells=p, origins=p, summary=p, extra=p, aside=p, changed=p, **kw):
        a = dict(good, **kw)
        return lib.mmd_grid_window_goals_aside(dist, a["nx"], a["ny"], a["n_fields"], field, a["n"], a["reach"], a["max_steps"], a["window"],
                                               a["sep"], a["aside_reach"], a["aside_steps"], a["restart"], a["n_sweeps"], apart,
                                               a["apart_bytes"], work, a["work_bytes"], cells, origins, summary, extra, aside, changed, None)
    assert call(n=0) == 0 and call(n=0, dist=None, field=None, apart=None, work=None, apart_bytes=0, work_bytes=0, cells=None, origins=None,
                                   summary=None, extra=None, aside=None, changed=None) == 0
    for kw, word in ((dict(nx=0), "grid"), (dict(ny=2049), "grid"), (dict(n_fields=-1), "n_fields"), (dict(n=-1), "n_queries"),
                     (dict(reach=0), "reach"), (dict(reach=6), "reach"), (dict(max_steps=0), "max_steps"), (dict(window=31), "window"),
                     (dict(max_steps=4096, apart_bytes=2 ** 40), "max_steps"), (dict(sep=0), "sep"), (dict(sep=1025), "sep"),
                     (dict(aside_reach=0), "aside_reach"), (dict(aside_reach=6), "aside_reach"), (dict(aside_reach=-1), "aside_reach"),
                     (dict(nx=200, ny=200, window=200, reach=99, aside_reach=64), "aside_reach"),
                     (dict(aside_steps=0), "aside_steps"), (dict(aside_steps=4096), "aside_steps"), (dict(n=0, aside_steps=0), "aside_steps"),
                     (dict(n_sweeps=-1), "n_sweeps"), (dict(n=0, n_sweeps=-1), "n_sweeps"),
                     (dict(dist=None), "NULL dist"), (dict(field=None), "NULL field"), (dict(apart=None), "apart workspace"),
                     (dict(apart=C.c_void_p(264)), "aligned"), (dict(apart_bytes=apart_size(7, 9) - 1), "apart workspace"),
                     (dict(work=None), "NULL workspace"), (dict(work=C.c_void_p(264)), "aligned"), (dict(work_bytes=size(7) - 1), "workspace"),
                     (dict(n=8), "workspace"), (dict(max_steps=10), "apart workspace"),
                     (dict(cells=None), "NULL cells"), (dict(origins=None), "NULL origins"), (dict(summary=None), "NULL summary"),
                     (dict(extra=None), "NULL extra"), (dict(aside=None), "NULL aside"), (dict(changed=None), "NULL changed")):
        assert call(**kw) == 2, kw
        assert lib.mmd_last_error().startswith(b"mmd_grid_window_goals_aside:") and word.encode() in lib.mmd_last_error(), \
            (kw, lib.mmd_last_error())
    # the order a caller with two faults sees: ranges, the inputs, the apart workspace, the workspace, the outputs
    for kw, word in ((dict(aside_reach=0, cells=None), b"aside_reach"), (dict(field=None, work=None), b"NULL field"),
                     (dict(apart=None, work=None), b"apart workspace"), (dict(work=None, aside=None), b"NULL workspace"),
                     (dict(cells=None, aside=None), b"NULL cells")):
        assert call(**kw) == 2 and word in lib.mmd_last_error(), (kw, lib.mmd_last_error())
    import torch
    with pytest.raises(ValueError, match="dist must be a contiguous int32"):              # on the CPU: the wrapper's first refusal
        F.device_subgoals_aside(torch.zeros(1, 40, 30, dtype=torch.int32), [[1, 1]], [0], [[2, 2]], 5, 5000, 0, 0, 0, window=12, sweeps=0)


# ---- 5. the fleet's refusals and defaults ----------------------------------------------------------------------------------------------------------
def test_fleet_refusals_and_defaults():
    params = inspect.signature(F.WorldFleet.__init__).parameters
    assert (params["step_aside"].default, params["aside_reach"].default, params["aside_steps"].default) == (False, 48, 96)
    assert F.EpochTargets._fields[-1] == "aside" and F.EpochTargets._field_defaults["aside"] is None
    assert F.FleetResult._fields == ("paths", "arrived", "epochs")
    assert (F.ASIDE_HELD, F.ASIDE_YIELDS, F.ASIDE_MOVED, F.ASIDE_RELEASED) == (1, 2, 4, 8)
    name = "AsideRefusals"
    E.register_world_map(name, np.zeros((800, 400), np.uint8), origin=(2.0, 2.0))
    try:
        at = lambda cells: (2.0 + (np.asarray(cells) + 0.5) * E.SDF_CELL_SIZE).astype(np.float32)                      # noqa: E731
        starts, goals = at([(100, 100), (300, 100), (500, 100)]), at([(100, 300), (300, 300), (500, 300)])
        with pytest.raises(ValueError, match="step_aside=True needs separation"):
            F.WorldFleet(None, name, starts, goals, device="cpu", step_aside=True)
        with pytest.raises(ValueError, match="seed_epochs"):
            F.WorldFleet(None, name, starts, goals, device="cpu", separation=23, step_aside=True, seed_epochs=True)
        for kw in (dict(aside_reach=64), dict(aside_reach=0), dict(reach=40), dict(aside_steps=0), dict(aside_steps=4096)):
            with pytest.raises(ValueError, match="aside_reach = .* aside_steps = "):
                F.WorldFleet(None, name, starts, goals, device="cpu", separation=23, step_aside=True, **kw)
    finally:
        E.unregister_world_map(name)
