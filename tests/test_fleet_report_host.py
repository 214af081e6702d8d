"""The fleet run report's definition (world_fleet.run_report) on hand-built cases, no GPU: the hop over a wall one cell thick that only the
interior points of a segment see; the strict `<` of both margins at the edge; bad points, a point far outside, a single robot; arrival;
the sums that tie the conflict words together; the vectorised definition against the same report written out point by point; and the
surface of mmd_fleet_run_report as far as it shows without a launch."""
import numpy as np
import pytest

import fleet_report_cases as K
import fp32_forms
from mmd_amd import world_fleet as F

f32 = np.float32


def report(paths, goals, margin=0.0, rr_margin=F.RR_MARGIN, n_interp=3, goal_tol=None, **kw):
    return F.run_report(paths, K.texture(), K.LO, K.HI, goals, margin, rr_margin, n_interp, goal_tol, **kw)


def test_the_norm_is_the_margin_tests_host_model():
    """world_fleet.torch_norm2 is fp32_forms.torch_norm2 (which test_mapf_host holds to exact arithmetic) on pairs at the margin, on
    ordinary differences, and where the sum overflows or is not a number"""
    pa, pb = fp32_forms.margin_pairs(3, 20000)
    d = pa - pb
    np.testing.assert_array_equal(K.bits(F.torch_norm2(d[:, 0], d[:, 1])), K.bits(fp32_forms.torch_norm2(d[:, 0], d[:, 1])))
    r = np.random.default_rng(4).normal(0, 1, (20000, 2)).astype(f32) * f32(10.0) ** np.random.default_rng(5).integers(-20, 18, (20000, 1)).astype(f32)
    np.testing.assert_array_equal(K.bits(F.torch_norm2(r[:, 0], r[:, 1])), K.bits(fp32_forms.torch_norm2(r[:, 0], r[:, 1])))
    odd = F.torch_norm2(f32([3e30, np.inf, np.nan, 0, -np.inf]), f32([1, 2, 0, 0, np.inf]))
    assert odd[0] == np.inf and odd[1] == np.inf and np.isnan(odd[2]) and odd[3] == 0 and odd[4] == np.inf


def test_the_hop_is_seen_by_interior_points_only():
    paths, goals = K.hop_case()
    assert (K.texture()[K.WALL_X, :, 0] < 0).all() and K.texture()[K.WALL_X - 1, 10, 0] > 0 and K.texture()[K.WALL_X + 1, 10, 0] > 0
    assert K.cells_of(paths[0]).tolist() == [[16, 10], [19, 10], [22, 10], [25, 10]]
    a, b = paths[0, 1], paths[0, 2]
    q = [a + (b - a) * (f32(j) / f32(3)) for j in (1, 2)]
    assert K.cells_of(q).tolist() == [[K.WALL_X, 10], [K.WALL_X + 1, 10]], "the interior points must land in the wall and behind it"
    r = report(paths, goals, margin=0.0, n_interp=2)
    assert r.points_hit.tolist() == [0] and r.interp_hit.tolist() == [1] and r.first_hit.tolist() == [1] and r.robots_hit == 1
    assert r.clear_min[0] == K.texture()[K.WALL_X, 10, 0] < 0
    clean = report(paths, goals, margin=0.0, n_interp=0)
    assert clean.points_hit.tolist() == [0] and clean.interp_hit.tolist() == [0] and clean.first_hit.tolist() == [-1] and clean.robots_hit == 0
    assert clean.clear_min[0] > 0
    three = f32(3 * K.CELL)
    assert r.max_step[0] == three and r.length[0] == f32(9 * K.CELL) and r.end_error[0] == 0 and r.arrival.tolist() == [3]


def test_margin_is_strict_at_a_value_of_the_texture():
    paths, goals, value, n_at = K.margin_edge_case()
    at = report(paths, goals, margin=value, n_interp=0)
    assert at.points_hit.tolist() == [0] and at.first_hit.tolist() == [-1] and at.clear_min[0] == value
    above = report(paths, goals, margin=np.nextafter(value, f32(np.inf)), n_interp=0)
    assert above.points_hit.tolist() == [n_at] and above.first_hit.tolist() == [0] and above.robots_hit == 1
    # the interior points lie in the same column of cells: they hold the same value and fall with the waypoints
    assert report(paths, goals, margin=value, n_interp=3).interp_hit.tolist() == [0]
    assert report(paths, goals, margin=np.nextafter(value, f32(np.inf)), n_interp=3).interp_hit.tolist() == [3 * (n_at - 1)]


def test_rr_margin_is_strict_at_a_distance_in_torch_norms_form():
    paths, goals, d = K.rr_edge_case()
    at = report(paths, goals, margin=-1.0, rr_margin=d, column_conflicts=True)
    assert at.conflict_count == 0 and at.first_conflict == (-1, -1, -1) and at.conflicts.tolist() == [0, 0] and at.robots_in_conflict == 0
    above = report(paths, goals, margin=-1.0, rr_margin=np.nextafter(d, f32(np.inf)), column_conflicts=True)
    assert above.conflict_count == 1 and above.first_conflict == (0, 0, 1) and above.conflicts.tolist() == [1, 1]
    assert above.robots_in_conflict == 2 and above.column_conflicts.tolist() == [1, 0]


def test_bad_points_a_far_point_and_a_single_robot():
    c = [K.centre(24 + 2 * t, 20) for t in range(10)]
    paths = np.asarray([c], f32)
    paths[0, 2, 1] = np.nan
    paths[0, 5, 0] = np.inf
    paths[0, 7] = (3e6, -3e6)
    r = report(paths, paths[:, -1].copy(), margin=0.0, n_interp=3, column_conflicts=True)
    assert r.bad_points.tolist() == [2] and r.outside.tolist() == [1] and r.points_hit.tolist() == [0] and r.interp_hit.tolist() == [0]
    # the far point reads the clamped corner texel (47, 0), which is free; the segments at a bad point or at the far point: 0-1 and 8-9 remain
    # among the short ones, 6-7 and 7-8 are long and finite
    assert K.cells_of(paths[0, 7]).tolist() == [[47, 0]]
    lengths = F.segment_lengths(paths)[0]
    assert (lengths[[1, 2, 4, 5]] == 0).all() and (lengths[[0, 3, 8]] == f32(2 * K.CELL)).all() and (lengths[[6, 7]] > 1e6).all()
    assert r.max_step[0] == lengths.max() and np.isfinite(r.length[0])
    assert r.conflict_count == 0 and r.first_conflict == (-1, -1, -1) and r.conflicts.tolist() == [0] and r.column_conflicts.tolist() == [0] * 10
    assert r.arrival.tolist() == [9] and r.end_error[0] == 0
    # a bad last point: no arrival, and the end error is the NaN the device writes
    paths[0, -1, 0] = -np.inf
    r = report(paths, np.asarray([c[-1]], f32))
    assert r.arrival.tolist() == [10] and K.bits(r.end_error).tolist() == [0x7fc00000] and r.robots_arrived == 0
    # two robots on one bad point do not collide there
    both = np.stack([paths[0], paths[0]])
    r = report(both, both[:, 0].copy(), rr_margin=0.1)
    assert r.conflicts.tolist() == [7, 7] and r.conflict_count == 7 and r.first_conflict == (0, 0, 1)


def test_arrival_is_the_start_of_the_last_stay_on_the_goal():
    goal = np.asarray(K.centre(10, 10), f32)
    away = np.asarray(K.centre(14, 10), f32)
    tol = f32(K.CELL)
    near = goal + np.asarray([tol, 0], f32)                     # exactly goal_tol away (a dyadic sum): still on the goal, `<=`
    assert fp32_forms.pos_norm(near, goal) == tol
    comes_back = [away, away, away, goal, goal, away, away, goal, near, goal]
    never = [away] * 10
    leaves = [goal] * 9 + [away]
    always = [goal] * 10
    beyond = [goal] * 9 + [np.asarray([np.nextafter(near[0], f32(np.inf)), near[1]], f32)]    # one float32 further out: off the goal
    assert fp32_forms.pos_norm(beyond[-1], goal) > tol
    paths = np.asarray([comes_back, never, leaves, always, beyond], f32)
    r = report(paths, np.tile(goal, (5, 1)), margin=-1.0, rr_margin=0.0)
    assert r.arrival.tolist() == [7, 10, 10, 0, 10] and r.robots_arrived == 2
    assert F.run_report(paths, K.texture(), K.LO, K.HI, np.tile(goal, (5, 1)), -1.0, 0.0, 0, 0.0).arrival.tolist() == [9, 10, 10, 0, 10]
    with pytest.raises(ValueError, match="goal_tol"):
        report(paths, np.tile(goal, (5, 1)), goal_tol=-1.0)
    with pytest.raises(ValueError, match="n_interp"):
        report(paths, np.tile(goal, (5, 1)), n_interp=64)
    with pytest.raises(ValueError, match="L = 1"):
        report(paths[:, :1], np.tile(goal, (5, 1)))


@pytest.mark.parametrize("n, length, n_interp", [(5, 9, 2), (3, 70, 0), (9, 20, 5)])
def test_the_definition_is_its_own_text_point_by_point(n, length, n_interp):
    paths, goals = K.random_case(n, length, 100 + n)
    tol = f32(K.CELL)
    got = report(paths, goals, margin=0.03, rr_margin=0.105, n_interp=n_interp, goal_tol=tol, column_conflicts=True)
    want = K.loop_report(paths, K.texture(), K.LO, K.HI, goals, 0.03, 0.105, n_interp, tol)
    for k in K.INT_FIELDS + ("column_conflicts",):
        np.testing.assert_array_equal(getattr(got, k), want[k], err_msg=k)
    for k in K.EXACT_FLOAT_FIELDS:
        np.testing.assert_array_equal(K.bits(getattr(got, k)), K.bits(want[k]), err_msg=k)
    for k in K.RUN_FIELDS:
        assert getattr(got, k) == want[k], k
    np.testing.assert_array_equal(K.bits(F.segment_lengths(paths)), K.bits(want["lengths"]))
    np.testing.assert_array_equal(got.length, want["lengths"].astype(np.float64).sum(1).astype(f32))


def test_the_conflict_words_add_up_and_the_cases_hold_every_kind():
    paths, goals = K.random_case(21, 130, 7)
    r = report(paths, goals, margin=0.03, n_interp=3, column_conflicts=True)
    assert r.conflict_count > 0 and int(r.conflicts.sum()) == 2 * r.conflict_count and int(r.column_conflicts.sum()) == r.conflict_count
    t, i, j = r.first_conflict
    assert 0 <= i < j < 21 and t == int(np.flatnonzero(r.column_conflicts)[0])
    assert r.points_hit.sum() > 0 and r.interp_hit.sum() > 0 and r.bad_points.sum() > 0 and r.outside.sum() > 0
    assert 0 < r.robots_arrived < 21 and 0 < r.robots_in_conflict <= 21 and (r.first_hit >= -1).all()
    assert r.column_conflicts.dtype == np.int32 and report(paths, goals).column_conflicts is None


# ---- the surface, as far as it shows without a GPU -----------------------------------------------------------------------------------------
def test_entry_point_is_built_declared_and_answers_before_any_launch():
    import ctypes as C
    import os
    import __graft_entry__ as G
    from mmd_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "mmd_amd/csrc/fleet_report.hip" in G.SOURCES and "mmd_amd/csrc/fleet_report.hip" in open(os.path.join(root, "build.sh")).read()
    header = open(os.path.join(root, "include", "mmd_amd.h")).read()
    assert "int mmd_fleet_run_report(" in header and _lib.ABI_VERSION == 9 and "mmd_fleet_run_report" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    p = C.c_void_p(256)                                         # never dereferenced: every call below returns before a launch
    lo, hi = (C.c_float * 2)(-1.5, -1.25), (C.c_float * 2)(1.5, 1.25)
    good = [p, 3, 70, p, 48, 40, lo, hi, p, 0.05, 0.105, 3, 0.0625, 0, p]
    nan, inf = float("nan"), float("inf")
    for at, value, word in ((1, -1, "n_robots"), (1, 4097, "n_robots"), (2, 1, "length"), (2, 65536, "length"), (4, 0, "grid of"),
                            (5, 1 << 20, "grid of"), (6, None, "NULL limits"), (7, None, "NULL limits"), (7, lo, "limits ("),
                            (6, (C.c_float * 2)(nan, 0), "limits ("), (9, nan, "margin = "), (9, inf, "margin = "), (10, nan, "rr_margin"),
                            (10, -inf, "rr_margin"), (11, -1, "n_interp"), (11, 64, "n_interp"), (12, -0.5, "goal_tol"), (12, nan, "goal_tol"),
                            (12, inf, "goal_tol"), (13, 2, "column_conflicts"), (13, -1, "column_conflicts"), (0, None, "paths"),
                            (0, C.c_void_p(260), "paths"), (3, None, "grid"), (3, C.c_void_p(264), "grid"), (8, None, "goals"),
                            (8, C.c_void_p(260), "goals"), (14, None, "report"), (14, C.c_void_p(260), "report")):
        args = list(good)
        args[at] = value
        rc = lib.mmd_fleet_run_report(*args, None)
        message = lib.mmd_last_error().decode()
        assert rc != 0 and word in message and message.startswith("mmd_fleet_run_report:"), (at, word, message)
        assert word != "margin = " or "rr_margin" not in message
    args = list(good)
    args[1] = 0
    assert lib.mmd_fleet_run_report(*args, None) == 0           # no robots: nothing launched
    assert lib.mmd_fleet_run_report(None, 0, 70, None, 48, 40, lo, hi, None, 0.05, 0.105, 3, 0.0625, 1, None, None) == 0
    # the Python surface: the report is opt-in, FleetResult keeps its three fields
    import inspect
    assert F.FleetResult._fields == ("paths", "arrived", "epochs")
    sig = inspect.signature(F.WorldFleet.report).parameters
    assert sig["margin"].default == F.ROBOT_RADIUS and sig["rr_margin"].default == F.RR_MARGIN and sig["n_interp"].default == 3
    assert sig["goal_tol"].default is None
    assert list(inspect.signature(F.device_run_report).parameters)[:9] == ["paths_dev", "tex_dev", "lo", "hi", "goals", "margin", "rr_margin",
                                                                           "n_interp", "goal_tol"]
    import torch
    from mmd_amd import ops  # noqa: F401
    assert hasattr(torch.ops.mmd_amd, "fleet_run_report")
