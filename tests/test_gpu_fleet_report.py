"""-m gpu: the fleet run report (mmd_fleet_run_report, world_fleet.device_run_report, WorldFleet.report).  The kernels are the numpy
definition run_report: every integer word, clear_min, max_step and end_error bit for bit on seeded runs whose sizes straddle every chunk
of 64 columns and every tile of 32 robots, with points on walls, outside the world and not finite; `length` within the bound of a float32
sum.  The hop over a thin wall and the strict `<` of both margins, on the device; refused calls and N = 0 leave the buffer alone; the
torch op gives the ctypes path's words; and a real fleet run reports what the definition says of its copied-back paths."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fleet_report_cases as K                                   # noqa: E402
from mmd_amd import _lib, map_textures, world_fleet as F         # noqa: E402
from test_gpu_world_fleet import crossing                        # noqa: E402,F401  (the module's fleet run, as a fixture here)

f32 = np.float32
GUARD = 0x5A5A5A5A
PAD = 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


@pytest.fixture(scope="module")
def tex_dev():
    return torch.from_numpy(K.texture()).cuda()


def n_words(n, length, columns):
    return 8 + 11 * n + (length if columns else 0)


def raw_args(paths_d, tex_d, goals_d, margin, rr_margin, n_interp, goal_tol, columns, out_ptr):
    n, length = paths_d.shape[:2]
    return [C.c_void_p(paths_d.data_ptr()), n, length, C.c_void_p(tex_d.data_ptr()), tex_d.shape[0], tex_d.shape[1], (C.c_float * 2)(*K.LO),
            (C.c_float * 2)(*K.HI), C.c_void_p(goals_d.data_ptr()), float(margin), float(rr_margin), int(n_interp), float(goal_tol), int(columns),
            C.c_void_p(out_ptr)]


def raw_report(paths, tex_d, goals, margin, rr_margin, n_interp, goal_tol, columns=True):
    """mmd_fleet_run_report through ctypes, twice into one buffer with guard words in front of and behind the report -> RunReport.  The
    guards must be untouched and the second call must leave the first one's words."""
    paths_d, goals_d = torch.from_numpy(paths).cuda(), torch.from_numpy(goals).cuda()
    n, length = paths.shape[:2]
    size = n_words(n, length, columns)
    buf = torch.full((2 * PAD + size,), GUARD, dtype=torch.int32, device="cuda")
    runs = []
    for _ in range(2):
        _lib.launch("mmd_fleet_run_report", buf, *raw_args(paths_d, tex_d, goals_d, margin, rr_margin, n_interp, goal_tol, columns,
                                                           buf.data_ptr() + 4 * PAD))
        torch.cuda.synchronize()
        words = buf.cpu().numpy()
        assert (words[:PAD] == GUARD).all() and (words[PAD + size:] == GUARD).all(), "wrote outside the report"
        runs.append(words[PAD:PAD + size].copy())
    assert np.array_equal(runs[0], runs[1]), "a second call into the same buffer differs"
    return F.report_from_words(runs[0], n, length, columns)


def assert_length_within_the_sum_bound(got, paths, what):
    """`length` against the float64 sum of the definition's own float32 segment lengths: a float32 sum of L - 1 non-negative terms in any
    order is within (L - 1) u / (1 - (L - 1) u) < L * 2^-24 of it, relatively"""
    length = paths.shape[1]
    exact = F.segment_lengths(paths).astype(np.float64).sum(1)
    err = np.abs(got.length.astype(np.float64) - exact)
    print(f"{what}: length, worst relative error {float((err / np.maximum(exact, 1e-300)).max()):.3e}, bound {length * 2.0 ** -24:.3e}")
    assert (err <= length * 2.0 ** -24 * exact).all(), (what, float((err / np.maximum(exact, 1e-300)).max()))


SIZES = [(1, 2, 3), (2, 63, 1), (3, 64, 0), (64, 65, 3), (65, 65, 8), (130, 129, 1), (64, 128, 0), (3, 200, 8), (65, 200, 3), (130, 2, 1)]


@pytest.mark.parametrize("n, length, n_interp", SIZES)
def test_kernels_are_the_definition(tex_dev, n, length, n_interp):
    paths, goals = K.random_case(n, length, 1000 * n + length)
    margin, rr_margin, tol = 0.03, F.RR_MARGIN, f32(K.CELL)
    want = F.run_report(paths, K.texture(), K.LO, K.HI, goals, margin, rr_margin, n_interp, tol, column_conflicts=True)
    what = f"N {n}, L {length}, n_interp {n_interp}"
    if n >= 64 and length >= 63:                                  # the cases hold every kind of point and of outcome
        assert want.points_hit.sum() > 0 and want.bad_points.sum() > 0 and want.outside.sum() > 0 and want.conflict_count > 0
        assert 0 < want.robots_arrived < n and (want.interp_hit.sum() > 0 or n_interp == 0)
    got = raw_report(paths, tex_dev, goals, margin, rr_margin, n_interp, tol)
    K.assert_reports_equal(got, want, length, what)
    assert_length_within_the_sum_bound(got, paths, what)
    assert int(got.conflicts.sum()) == 2 * got.conflict_count and int(got.column_conflicts.sum()) == got.conflict_count
    surface = F.device_run_report(torch.from_numpy(paths).cuda(), tex_dev, K.LO, K.HI, goals, margin, rr_margin, n_interp, tol)
    K.assert_reports_equal(surface, want, length, what + " (device_run_report)")
    assert surface.column_conflicts is None and np.array_equal(K.bits(surface.length), K.bits(got.length))
    if n >= 64:                                                   # few conflicts: the first one is not in column 0, nor in the first tile
        sparse = on_device(tex_dev, paths, goals, margin, rr_margin=0.004, n_interp=0, goal_tol=tol)
        assert sparse.conflict_count < want.conflict_count


def on_device(tex_dev, paths, goals, margin, rr_margin=F.RR_MARGIN, n_interp=3, goal_tol=None, columns=True):
    """(device_run_report, run_report) of one case, after holding the first to the second"""
    got = F.device_run_report(torch.from_numpy(paths).cuda(), tex_dev, K.LO, K.HI, goals, margin, rr_margin, n_interp, goal_tol, columns)
    want = F.run_report(paths, K.texture(), K.LO, K.HI, goals, margin, rr_margin, n_interp, goal_tol, columns)
    K.assert_reports_equal(got, want, paths.shape[1])
    return got


def test_the_hop_and_both_strict_margins_on_the_device(tex_dev):
    paths, goals = K.hop_case()
    r = on_device(tex_dev, paths, goals, 0.0, n_interp=2)
    assert r.points_hit.tolist() == [0] and r.interp_hit.tolist() == [1] and r.first_hit.tolist() == [1] and r.robots_hit == 1
    clean = on_device(tex_dev, paths, goals, 0.0, n_interp=0)
    assert clean.points_hit.tolist() == [0] and clean.interp_hit.tolist() == [0] and clean.first_hit.tolist() == [-1] and clean.robots_hit == 0
    paths, goals, value, n_at = K.margin_edge_case()
    assert on_device(tex_dev, paths, goals, value, n_interp=3).robots_hit == 0
    above = on_device(tex_dev, paths, goals, np.nextafter(value, f32(np.inf)), n_interp=3)
    assert above.points_hit.tolist() == [n_at] and above.interp_hit.tolist() == [3 * (n_at - 1)] and above.first_hit.tolist() == [0]
    paths, goals, d = K.rr_edge_case()
    at = on_device(tex_dev, paths, goals, -1.0, rr_margin=d)
    assert at.conflict_count == 0 and at.first_conflict == (-1, -1, -1) and at.robots_in_conflict == 0
    above = on_device(tex_dev, paths, goals, -1.0, rr_margin=np.nextafter(d, f32(np.inf)))
    assert above.conflict_count == 1 and above.first_conflict == (0, 0, 1) and above.conflicts.tolist() == [1, 1]
    assert above.column_conflicts.tolist() == [1, 0] and above.robots_in_conflict == 2


def test_refused_calls_and_no_robots_leave_the_buffer_alone(tex_dev):
    paths, goals = K.random_case(5, 70, 3)
    paths_d, goals_d = torch.from_numpy(paths).cuda(), torch.from_numpy(goals).cuda()
    size = n_words(5, 70, True)
    buf = torch.full((size + PAD,), GUARD, dtype=torch.int32, device="cuda")
    lib, stream = _lib.load(), _lib.current_stream_ptr()
    good = raw_args(paths_d, tex_dev, goals_d, 0.03, 0.105, 3, K.CELL, 1, buf.data_ptr())
    for at, value, word in ((1, 4097, "n_robots"), (2, 1, "length"), (4, 0, "grid of"), (9, float("nan"), "margin"), (10, float("inf"), "rr_margin"),
                            (11, 64, "n_interp"), (12, -1.0, "goal_tol"), (13, 2, "column_conflicts"), (0, None, "paths"), (3, None, "grid"),
                            (8, C.c_void_p(goals_d.data_ptr() + 4), "goals"), (14, C.c_void_p(buf.data_ptr() + 4), "report"), (1, 0, None)):
        args = list(good)
        args[at] = value
        rc = lib.mmd_fleet_run_report(*args, stream)
        if word is None:
            assert rc == 0                                        # no robots: accepted, nothing launched
        else:
            assert rc != 0 and word in lib.mmd_last_error().decode() and "mmd_fleet_run_report" in lib.mmd_last_error().decode(), (at, word)
        torch.cuda.synchronize()
        assert bool((buf == GUARD).all()), (at, word)
    assert lib.mmd_fleet_run_report(*good, stream) == 0
    torch.cuda.synchronize()
    words = buf.cpu().numpy()
    assert (words[size:] == GUARD).all()
    want = F.run_report(paths, K.texture(), K.LO, K.HI, goals, 0.03, 0.105, 3, K.CELL, column_conflicts=True)
    K.assert_reports_equal(F.report_from_words(words[:size], 5, 70, True), want, 70)
    assert words[7] == 0                                          # the header's spare word is written too


def test_the_torch_op_gives_the_ctypes_paths_words(tex_dev):
    from mmd_amd import ops  # noqa: F401
    paths, goals = K.random_case(65, 129, 5)
    paths_d, goals_d = torch.from_numpy(paths).cuda(), torch.from_numpy(goals).cuda()
    for columns in (False, True):
        direct = F.device_run_report_words(paths_d, tex_dev, K.LO, K.HI, goals_d, 0.03, F.RR_MARGIN, 3, K.CELL, columns)
        op = torch.ops.mmd_amd.fleet_run_report(paths_d, tex_dev, goals_d, K.LO[0], K.LO[1], K.HI[0], K.HI[1], 0.03, F.RR_MARGIN, 3, K.CELL, columns)
        assert op.dtype == torch.int32 and op.shape == (n_words(65, 129, columns),) and torch.equal(op, direct)
    with pytest.raises(RuntimeError, match="n_interp"):
        torch.ops.mmd_amd.fleet_run_report(paths_d, tex_dev, goals_d, K.LO[0], K.LO[1], K.HI[0], K.HI[1], 0.03, F.RR_MARGIN, 64, K.CELL, False)


def test_a_real_run_reports_what_the_definition_says_of_its_paths(crossing):  # noqa: F811
    from mmd_amd import environments as E
    fleet, result, starts, goals, _ = crossing
    assert fleet._sampler is None                                 # run() has closed: the report needs nothing of the sampler
    n, length = result.paths.shape[:2]
    got = fleet.report(result, column_conflicts=True)
    tex = map_textures.device_world_texture(fleet.name, fleet.device).cpu().numpy()
    lo, hi = E.world_map_limits(fleet.name)
    want = F.run_report(result.paths.cpu().numpy(), tex, lo, hi, goals, F.ROBOT_RADIUS, F.RR_MARGIN, 3, None, column_conflicts=True)
    K.assert_reports_equal(got, want, length, "the crossing")
    assert_length_within_the_sum_bound(got, result.paths.cpu().numpy(), "the crossing")
    assert (got.arrival < length).all() and (got.arrival < length).tolist() == result.arrived.tolist()
    assert K.bits(got.end_error).tolist() == [0] * n, "that world's arithmetic is exact: every last point is its goal"
    assert got.robots_arrived == n and got.bad_points.tolist() == [0] * n and got.outside.tolist() == [0] * n
    again = fleet.report(result.paths.cpu().numpy(), column_conflicts=True)           # any paths of the fleet's robots, from the host as well
    K.assert_reports_equal(again, got, length, "the crossing, from host paths")
