"""-m gpu: the best-path pick and the conflict report on a cell table of the best paths (mmd_bin_paths, mmd_count_collisions_binned,
mmd_path_conflicts_binned) and MultiRobotSampler.plan.  The yardsticks are the all-pairs kernels that predate them (mmd_count_collisions,
mmd_find_conflicts, mmd_rr_collisions) and a numpy brute force in torch.norm's fp32 form (fp32_forms); every comparison is exact --
integers equal, record floats bitwise equal: a cell's list holds every robot within the margin (csrc/multi_agent.hip, COVER), and a count
does not depend on the order of a list."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                                                        # noqa: E402
from mmd_amd.constraints import binned_collision_table, binned_constraints_from_paths   # noqa: E402
import fp32_forms as F                                                           # noqa: E402
from cases import H, D                                                           # noqa: E402
from test_binned_host import cell_index, ulps, R                                 # noqa: E402

SENTINEL = -7777


def _circle(n, radius=0.45):
    starts, goals = synth.start_goal_circle(n, radius)
    return starts, goals, synth.straight_line_paths(starts, goals, H)


def _random20():
    from mmd_amd import trials
    starts, goals = trials.get_start_goal_pos_random_in_env(20, "EnvHighways2D", seed=0)
    starts, goals = np.asarray(starts, np.float32), np.asarray(goals, np.float32)
    return starts, goals, synth.straight_line_paths(starts, goals, H)


def _planted37():
    """the 37-robot circle with the planted points of test_gpu_binned.test_table_is_the_brute_force_lists: outside the limits, the corners,
    on cell edges (and an ulp either side), pairs at the acceptance radius, three coincident robots"""
    n = 37
    paths = _circle(n)[2]
    edge = np.float32(-1.0) + np.float32(7) * np.float32(2.0 / 15)
    planted = [(1.3, -1.2), (-1.3, 1.2), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (edge, edge), (ulps(edge, 1), ulps(edge, -1)),
               (ulps(edge, -1), edge), (0.0, 0.0), (float(R), 0.0), (ulps(R, 1), 0.0), (0.0, ulps(R, -1)), (-1.0, edge), (edge, 1.0)]
    for k, p in enumerate(planted):
        paths[(5 * k + 2) % n, 1 + (11 * k) % (H - 1)] = p
        paths[(5 * k + 3) % n, H - 1 - (7 * k) % 20] = p
    paths[4, 30] = paths[9, 30] = paths[20, 30] = (0.4, -0.4)
    return paths


def _hits(paths):
    """numpy brute force: [T, N, N] bool, ||p_a(t) - p_b(t)|| < MARGIN in the pinned fp32 form, a != b"""
    p = np.ascontiguousarray(np.transpose(paths, (1, 0, 2)))                      # [T, N, 2]
    h = F.pos_norm(p[:, :, None, :], p[:, None, :, :]) < F.MARGIN
    h[:, np.arange(p.shape[1]), np.arange(p.shape[1])] = False
    return h


# ---- 1. the table with time step 0 ---------------------------------------------------------------------------------------------------
def test_bin_paths_lists_time_step_0_and_leaves_the_rest_alone():
    n = 37
    paths = _planted37()
    dev = torch.from_numpy(paths).cuda()
    old = binned_constraints_from_paths(dev, 0, n)
    new = binned_collision_table(dev)
    assert (old.first_step, new.first_step) == (1, 0) and new.grid == (15, 15) and new.n_local == n
    off0, ent0, _ = old.lists()
    off1, ent1, ids1 = new.lists()
    for t in range(1, H):                                                         # every offset, and every entry the offsets reach
        m = off0[t, -1]
        assert np.array_equal(off1[t], off0[t]) and np.array_equal(ent1[t, :m].view(np.int32), ent0[t, :m].view(np.int32)), t
    assert (off0[0] == 0).all()
    # time step 0: the brute-force lists
    cells = cell_index(paths[:, 0])                                               # [n, 2]
    cx, cy = np.divmod(np.arange(225), 15)
    near = (np.abs(cells[None, :, 0] - cx[:, None]) <= 1) & (np.abs(cells[None, :, 1] - cy[:, None]) <= 1)
    assert off1[0, 0] == 0 and off1[0, -1] == near.sum() > 4 * n
    for c in range(225):
        want = np.flatnonzero(near[c])
        assert ids1[0, off1[0, c]:off1[0, c + 1]].tolist() == want.tolist(), c
        assert np.array_equal(ent1[0, off1[0, c]:off1[0, c + 1], :2].view(np.int32), paths[want, 0].view(np.int32)), c


def test_bin_paths_first_step_1_is_the_old_function_bit_for_bit():
    """the two entry points into buffers with the same fill: the whole output, the unreached tail of every segment included"""
    from mmd_amd import _lib
    n = 37
    dev = torch.from_numpy(_planted37()).cuda()
    lo, hi = (C.c_float * 2)(-1, -1), (C.c_float * 2)(1, 1)
    out = []
    for name, extra in (("mmd_bin_constraints_from_paths", ()), ("mmd_bin_paths", (1,))):
        off = torch.full((H, 226), SENTINEL, dtype=torch.int32, device="cuda")
        ent = torch.full((H, 9 * n, 4), 123.0, dtype=torch.float32, device="cuda")
        _lib.launch(name, dev, dev.data_ptr(), n, H, 0.12, lo, hi, 15, 15, *extra, off.data_ptr(), ent.data_ptr())
        out.append((off.cpu(), ent.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
    assert (out[0][0] != SENTINEL).all() and (out[0][0][1:, -1] > 4 * n).all()


# ---- 2. the least-collisions scan ----------------------------------------------------------------------------------------------------
def _samples(paths, robot0, n_local, B, seed, scale=0.05):
    """[n_local * B, H, 4] un-normalised samples: the robot's straight line plus noise of `scale`"""
    t = np.zeros((n_local, B, H, D), np.float32)
    t[..., :2] = paths[robot0:robot0 + n_local, None]
    t += synth.synth_noise(seed, t.shape) * np.float32(scale)
    return t.reshape(n_local * B, H, D)


def _both_counts(trajs, paths, robot0, n_local):
    from mmd_amd import multi_agent as ma
    t, p = torch.from_numpy(trajs).cuda(), torch.from_numpy(paths).cuda()
    dense = ma.count_collisions(t, p, robot0, n_local)
    binned = ma.count_collisions_binned(t, binned_collision_table(p, robot0, n_local), n_local)
    assert binned.dtype == torch.int32 and binned.shape == dense.shape
    return dense.cpu().numpy(), binned.cpu().numpy()


def _brute_counts(trajs, paths, robot0, B):
    d = F.pos_norm(trajs[:, None, :, :2], paths[None]) < F.MARGIN                # [traj, robot, t]
    d[np.arange(len(trajs)), robot0 + np.arange(len(trajs)) // B] = False
    return d.sum((1, 2))


@pytest.mark.parametrize("kind,n,robot0,n_local,B", [
    ("circle", 37, 5, 3, 7),        # neighbours collide at t = 0 and t = 63: the t = 0 lists; 21 trajectories, not a multiple of 4
    ("circle", 300, 0, 2, 8),       # one cell list of ~299 entries at the centre crossing, lanes near the ends nearly none
    ("random", 20, 0, 2, 8),        # empty cells, short lists
    ("circle", 48, 46, 2, 4),       # self exclusion at the top end
], ids=["37_3x7", "300_2x8_centre", "20_random", "48_top"])
def test_binned_counts_are_the_dense_counts(kind, n, robot0, n_local, B):
    paths = _random20()[2] if kind == "random" else _circle(n)[2]
    trajs = _samples(paths, robot0, n_local, B, 500 + n)
    dense, binned = _both_counts(trajs, paths, robot0, n_local)
    print(f"{kind} {n}: counts {dense.min()} .. {dense.max()}")
    assert np.array_equal(binned, dense), (binned, dense)
    assert (dense > 0).any() and len(np.unique(dense)) > 1                        # the samples differ in their counts
    if n == 37:
        assert np.array_equal(dense.reshape(-1), _brute_counts(trajs, paths, robot0, B))
        line = np.zeros((n_local, H, D), np.float32)                              # the bare lines: their hits at t = 0 come from the t = 0 lists
        line[..., :2] = paths[robot0:robot0 + n_local]
        d0, b0 = _both_counts(line, paths, robot0, n_local)
        assert np.array_equal(b0, d0) and (F.pos_norm(paths[robot0, 0], paths[robot0 + 1, 0]) < F.MARGIN) and (d0 >= 4).all()


def test_binned_counts_at_the_margin_and_outside_the_limits():
    """sample points within an ulp or so of the margin from a table point, both sides; and an instance shifted so that table and sample
    points lie outside the map limits, in the border cells"""
    rng = np.random.default_rng(510)
    n, robot0, n_local, B = 37, 5, 3, 7
    paths = _planted37()
    other = rng.integers(0, n, (n_local * B, H))
    trajs = np.zeros((n_local * B, H, D), np.float32)
    trajs[..., :2] = F.near_points(rng, paths[other, np.arange(H)[None]], float(F.MARGIN), rel=2.4e-7)
    dist = F.pos_norm(trajs[..., :2], paths[other, np.arange(H)[None]])
    assert min(F.sides(dist)) > dist.size // 4                                    # both sides of the margin
    dense, binned = _both_counts(trajs, paths, robot0, n_local)
    assert np.array_equal(binned, dense) and np.array_equal(dense.reshape(-1), _brute_counts(trajs, paths, robot0, B))
    assert len(np.unique(dense)) > 1

    shifted = _circle(n)[2] + np.float32([0.8, -0.8])                             # x up to 1.25, y down to -1.25
    assert (np.abs(shifted) > 1.0).any(-1).mean() > 0.2
    trajs = _samples(shifted, robot0, n_local, B, 511)
    dense, binned = _both_counts(trajs, shifted, robot0, n_local)
    assert np.array_equal(binned, dense) and (dense > 0).any() and len(np.unique(dense)) > 1


# ---- 3. the conflict report ----------------------------------------------------------------------------------------------------------
PAST = 4                                                                          # rows behind a list's capacity that must stay untouched


def _dense_report(paths, cap):
    """mmd_find_conflicts(PAIRS) on an agent table of the same paths, start_time 0, length 64, into buffers filled with SENTINEL:
    (summary [16], rows [H], list [cap + PAST, 12])"""
    from mmd_amd import _lib, multi_agent as ma
    n = paths.shape[0]
    p4 = torch.zeros((n, 1, H, 4), dtype=torch.float32, device="cuda")
    p4[:, 0, :, :2] = paths
    table = ma.agent_table([p4[k] for k in range(n)], [0] * n, [0] * n)
    summ = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    rows = torch.empty(H, dtype=torch.int32, device="cuda")
    lst = torch.full((cap + PAST, 12), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.launch("mmd_find_conflicts", table, table.data_ptr(), n, H, float(F.MARGIN), ma.PAIRS, rows.data_ptr(), summ.data_ptr(),
                summ.data_ptr() + 16, lst.data_ptr() if cap else None, cap)
    return summ.cpu().numpy(), rows.cpu().numpy(), lst.cpu().numpy()


def _binned_report(paths, cap):
    """mmd_path_conflicts_binned on a table of the paths, into buffers filled with SENTINEL: (summary [16], rows [H], robots [N],
    list [cap + PAST, 12])"""
    from mmd_amd import _lib
    tab = binned_collision_table(paths)
    summ = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    rows = torch.empty(H, dtype=torch.int32, device="cuda")
    robots = torch.empty(paths.shape[0], dtype=torch.int32, device="cuda")
    lst = torch.full((cap + PAST, 12), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.launch("mmd_path_conflicts_binned", paths, paths.data_ptr(), C.byref(tab.struct), H, float(F.MARGIN), rows.data_ptr(),
                robots.data_ptr(), summ.data_ptr(), summ.data_ptr() + 16, lst.data_ptr(), cap)
    return summ.cpu().numpy(), rows.cpu().numpy(), robots.cpu().numpy(), lst.cpu().numpy()


def _check_words(summ, lst, count, cap):
    """a report written over SENTINEL: the reserved words of every written record (words 3, 10, 11: reserved, reserved2[0..1]) are 0, of
    the summary's first record too when there is one, and no row behind the last record was touched"""
    k = min(count, cap)
    assert lst.shape[0] > k and (lst[:k][:, [3, 10, 11]] == 0).all() and (lst[k:] == SENTINEL).all()
    if count > 0:
        assert (summ[4:16][[3, 10, 11]] == 0).all()


def _check_report(paths_np, cap=None, want_count=None):
    """count, first record, rows, list and per-robot counts against the all-pairs kernels and the brute force; returns the report"""
    from mmd_amd import multi_agent as ma
    paths = torch.from_numpy(paths_np).cuda()
    hits = _hits(paths_np)
    m = int(np.triu(hits.astype(np.int64).sum(0), 1).sum())
    if want_count is not None:
        assert m == want_count
    cap = m + 3 if cap is None else cap
    rows = torch.full((H,), SENTINEL, dtype=torch.int32, device="cuda")
    summ, robots, lst = ma.path_conflicts(paths, list_cap=cap, row_counts=rows)
    s, r, l = summ.cpu().numpy(), rows.cpu().numpy(), lst.cpu().numpy()
    ds, dr, dl = _dense_report(paths, cap)
    bs, br, brob, bl = _binned_report(paths, cap)                                 # the same call as path_conflicts', over SENTINEL
    k = min(m, cap)
    assert np.array_equal(bs[[0] + list(range(4, 16))], s[[0] + list(range(4, 16))]) and np.array_equal(br, r)
    assert np.array_equal(brob, robots.cpu().numpy()) and np.array_equal(bl[:k], l[:k])
    _check_words(ds, dl, m, cap)
    _check_words(bs, bl, m, cap)
    print(f"n = {paths_np.shape[0]}: {m} pairs, {int(dr[0])} at t = 0, list of {k}")
    assert s[0] == ds[0] == m
    assert np.array_equal(s[4:16], ds[4:16])                                      # the first record (t = a = b = -1 when there is none)
    assert np.array_equal(r, dr) and np.array_equal(r, hits.sum((1, 2)) // 2)     # per time step; the brute force has every pair twice
    assert np.array_equal(l[:k], dl[:k])                                          # records bitwise: t, a, b, pa, pb, mid
    t, a, b, pa, pb, mid = ma.decode_records(l[:k])
    assert (a < b).all() and hits[t, a, b].all()
    key = (t.astype(np.int64) * paths_np.shape[0] + a) * paths_np.shape[0] + b
    assert (np.diff(key) > 0).all()                                               # (t, a, b) row-major, no record twice
    mask, _ = ma.check_rr_collisions(paths, with_midpoints=False)
    per_robot = mask.sum((0, 2)).cpu().numpy()
    assert np.array_equal(robots.cpu().numpy(), per_robot) and np.array_equal(per_robot, hits.sum((0, 2)))
    assert ma.read_summary(summ)[0] == m
    return m, dr, per_robot


def test_path_conflicts_planted_circle():
    assert int(np.triu(_hits(_circle(37)[2]).sum(0), 1).sum()) == 11322           # the instance before planting
    m, rows, per_robot = _check_report(_planted37())
    assert (rows > 0).all() and rows[0] == 37 and m > 11000


def test_path_conflicts_random_instance():
    m, rows, per_robot = _check_report(_random20()[2], want_count=103)
    assert rows[0] == 0 and (rows == 0).any() and len(np.unique(per_robot)) > 1


def test_path_conflicts_truncated_list_of_300_robots():
    """806 400 pairs, a list of 1000: the count, the first 1000 records, and nothing written past the list"""
    from mmd_amd import _lib, multi_agent as ma
    paths_np = _circle(300)[2]
    paths = torch.from_numpy(paths_np).cuda()
    cap = 1000
    s, r, robots, l = _binned_report(paths, cap)
    ds, dr, dl = _dense_report(paths, cap)
    assert s[0] == ds[0] == 806400 and np.array_equal(s[4:16], ds[4:16]) and np.array_equal(r, dr)
    assert np.array_equal(l[:cap], dl[:cap])
    _check_words(ds, dl, 806400, cap)                                             # (and nothing behind record 1000, on both sides)
    _check_words(s, l, 806400, cap)
    hits = _hits(paths_np)
    assert np.array_equal(robots, hits.sum((0, 2))) and int(hits.sum()) == 2 * 806400
    # without a list and without per-robot counts
    tab = binned_collision_table(paths)
    rows = torch.empty(H, dtype=torch.int32, device="cuda")
    summ2 = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.launch("mmd_path_conflicts_binned", paths, paths.data_ptr(), C.byref(tab.struct), H, float(F.MARGIN), rows.data_ptr(), None,
                summ2.data_ptr(), summ2.data_ptr() + 16, None, 0)
    assert np.array_equal(summ2.cpu().numpy()[[0] + list(range(4, 16))], s[[0] + list(range(4, 16))])


def _parallel_lines(n=6):
    y = np.float32(-0.75) + np.float32(0.3) * np.arange(n, dtype=np.float32)
    starts = np.stack([np.full(n, -0.8, np.float32), y], 1)
    goals = np.stack([np.full(n, 0.8, np.float32), y], 1)
    return starts, goals, synth.straight_line_paths(starts, goals, H)


def test_path_conflicts_of_a_conflict_free_instance():
    from mmd_amd import multi_agent as ma
    paths_np = _parallel_lines()[2]
    m, rows, per_robot = _check_report(paths_np, want_count=0)
    summ, robots, lst = ma.path_conflicts(torch.from_numpy(paths_np).cuda())
    assert lst is None and ma.read_summary(summ) == (0, None)
    assert summ.cpu().numpy()[4:7].tolist() == [-1, -1, -1] and (robots == 0).all()


def test_path_conflicts_per_robot_counts_that_differ():
    """on the symmetric circle every robot has the same count, which would hide an indexing error: every robot shifted on its own"""
    sym = _hits(_circle(37)[2]).sum((0, 2))
    assert len(np.unique(sym)) == 1 and sym[0] == 612
    paths_np = _circle(37)[2] + synth.synth_noise(520, (37, 1, 2)) * np.float32(0.04)
    m, rows, per_robot = _check_report(paths_np)
    assert len(np.unique(per_robot)) > 5


# ---- 4. the round --------------------------------------------------------------------------------------------------------------------
T = 25


def test_round_with_the_binned_pick_is_the_dense_round():
    """MultiRobotSampler(constraint_table="binned"): the pick now counts on a collision table (mmd_count_collisions_binned); plan_round
    still gives the dense round's trajectories and best paths, and rank 1 of a world of 2, played on this GPU, rows 3-5"""
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    model = gc.hip_model(T)
    Rn, B = 6, 8
    starts, goals, paths_np = _circle(Rn)
    paths = torch.from_numpy(paths_np).cuda()
    dense = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B)
    binned = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, constraint_table="binned")
    td, bd = dense.plan_round(paths, seed=31)
    tb, bb = binned.plan_round(paths, seed=31)
    assert dense._collision is None
    assert binned._collision[0] is paths and binned._collision[1].first_step == 0 and binned.guide._binned.first_step == 1
    assert torch.isfinite(td).all() and torch.equal(tb, td) and torch.equal(bb, bd)
    assert torch.equal(binned.last_idx, dense.last_idx)
    # the counts behind the pick, and they are not all zero on this instance (the pick was a choice)
    from mmd_amd import multi_agent as ma
    u = binned.unnormalize(tb).contiguous()
    cd = ma.count_collisions(u, paths, 0, Rn)
    assert torch.equal(ma.count_collisions_binned(u, binned._collision[1], Rn), cd) and int(cd.max()) > 0
    part = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, rank=1, world_size=2, constraint_table="binned")
    assert part.robot0 == 3
    part.set_other_paths(paths)
    assert part._collision[1].robot0 == 3 and part._collision[1].n_local == 3
    tp = part.sample(seed=31)
    assert torch.equal(tp, td[3 * B:6 * B])
    assert torch.equal(part.best_paths(tp, paths), bd[3:6])
    other = paths.clone()                                                         # another tensor: the table is rebuilt for it
    assert torch.equal(part.best_paths(tp, other), bd[3:6]) and part._collision[0] is other
    binned.set_other_paths(None)
    assert binned._collision is None and binned.guide._binned is None


# ---- 5. plan() -----------------------------------------------------------------------------------------------------------------------
def _brute_report(paths):
    hits = _hits(paths.cpu().numpy())
    return int(hits.sum()) // 2, hits


@pytest.mark.parametrize("table", ["dense", "binned"])
def test_plan_is_the_hand_written_loop_of_rounds(table):
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    model = gc.hip_model(T)
    Rn, B, seed = 6, 8, 40
    starts, goals, paths_np = _circle(Rn)
    make = lambda: MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, constraint_table=table)   # noqa: E731
    hand = make()
    p0 = torch.from_numpy(paths_np).cuda()
    t1, p1 = hand.plan_round(p0, seed=seed)
    t2, p2 = hand.plan_round(p1, seed=seed + 1)
    want = [_brute_report(p)[0] for p in (p0, p1, p2)]
    print(f"{table}: conflicts per report {want}")
    res = make().plan(max_rounds=2, seed=seed)                                    # paths_local: the straight lines by default
    assert res.n_rounds == 2
    assert torch.equal(res.paths_local, p2) and torch.equal(res.trajs, t2)
    assert res.conflict_counts == want
    assert res.conflict_free == (want[-1] == 0) and (res.first_conflict is None) == (want[-1] == 0)
    hits = _brute_report(p2)[1]
    assert np.array_equal(res.robot_counts.cpu().numpy(), hits.sum((0, 2)))
    if want[-1]:
        t, a, b = (int(v) for v in np.argwhere(np.triu(hits, 1))[0])              # the first (t, a, b), a < b, row-major
        assert res.first_conflict[:3] == (t, a, b)
        assert np.array_equal(res.first_conflict[3], p2[a, t].cpu().numpy()) and np.array_equal(res.first_conflict[4], p2[b, t].cpu().numpy())
    # the same call seeded with the paths explicitly, and with a list of the final report
    res2 = make().plan(p0, max_rounds=2, seed=seed, list_cap=8)
    assert torch.equal(res2.paths_local, p2) and res2.conflict_counts == want
    # max_rounds = 0: only the report of the paths handed in
    s0 = make()
    res0 = s0.plan(p0, max_rounds=0)
    assert res0.n_rounds == 0 and res0.trajs is None and res0.conflict_counts == want[:1] and res0.paths_local is p0


def test_plan_stops_when_the_paths_are_conflict_free():
    """The early stop: the report before round 1 reads 0, so plan(max_rounds=3) runs one round.  Which paths a round of the MODEL returns
    cannot be arranged by the instance: with the synthetic weights and with the trained ones (g19) alike, samples stray from their
    straight line by up to the size of the map (the CPU oracle on two robots along opposite edges: up to 1.0; on the GPU those two, 1.6
    apart, meet after a round, and six lines 0.3 apart give 82 conflicts).  So the branch is driven by a sampler whose sample() returns
    every robot's line, sample b moved by 0.004 b in y: lines 0.3 apart stay at least 0.27 apart, far above the 0.105 margin.  Everything
    else of the loop is the real thing: the gather, the report kernels, the tables, the post-processing and the pick."""
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    starts, goals, paths_np = _parallel_lines()
    B, calls = 8, []

    class LineSampler(MultiRobotSampler):
        def sample(self, seed=None, **kw):
            calls.append(seed)
            t = torch.zeros((self.n_local, B, H, D))
            t[..., :2] = torch.from_numpy(paths_np)[self.robot0:self.robot0 + self.n_local, None]
            t[..., 1] += 0.004 * torch.arange(B, dtype=torch.float32)[None, :, None]
            return self.dataset.normalizer.normalize(t.view(-1, H, D)).to(self.device).contiguous()

    s = LineSampler(gc.hip_model(T), starts, goals, env_id="EnvEmpty2D", n_samples=B, inter_robot=True, constraint_table="binned")
    res = s.plan(max_rounds=3, seed=3)
    print(f"conflicts per report {res.conflict_counts}")
    assert calls == [3] and res.n_rounds == 1                                     # round 0 always runs; the report before round 1 stops the loop
    assert res.conflict_counts == [0, 0] and res.conflict_free and res.first_conflict is None and (res.robot_counts == 0).all()
    assert res.robot_counts.shape == (6,) and torch.equal(res.trajs, s.sample())
    assert _brute_report(res.paths_local)[0] == 0
    assert np.abs(res.paths_local.cpu().numpy() - paths_np).max() < 1e-6          # the pick: the first sample among equals, the line itself
    assert (s.last_idx == 0).all()


def test_plan_stop_rule_with_the_model():
    """the same rule on rounds of the model, whatever they return: plan(max_rounds=3) runs round k iff k == 0 or the brute-force count of
    the paths before it is not 0, and reports those counts"""
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    model = gc.hip_model(T)
    starts, goals = np.float32([[-0.8, -0.8], [-0.8, 0.8]]), np.float32([[0.8, -0.8], [0.8, 0.8]])
    make = lambda: MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=8, inter_robot=True, constraint_table="binned")   # noqa: E731
    hand, p = make(), torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    want, trajs, k = [_brute_report(p)[0]], None, 0
    while k < 3 and (k == 0 or want[-1] != 0):
        trajs, p = hand.plan_round(p, seed=3 + k)
        want.append(_brute_report(p)[0])
        k += 1
    res = make().plan(max_rounds=3, seed=3)
    print(f"conflicts per report {want}: {k} rounds")
    assert want[0] == 0 and res.n_rounds == k and res.conflict_counts == want
    assert torch.equal(res.paths_local, p) and torch.equal(res.trajs, trajs) and res.conflict_free == (want[-1] == 0)


# ---- 6. the torch ops ----------------------------------------------------------------------------------------------------------------
def test_torch_ops_are_the_ctypes_path():
    import mmd_amd.ops  # noqa: F401
    from mmd_amd import multi_agent as ma
    n, robot0, n_local, B = 37, 5, 3, 7
    paths_np = _planted37()
    paths = torch.from_numpy(paths_np).cuda()
    trajs = torch.from_numpy(_samples(paths_np, robot0, n_local, B, 537)).cuda()
    want = ma.count_collisions_binned(trajs, binned_collision_table(paths, robot0, n_local), n_local)
    got = torch.ops.mmd_amd.count_collisions_binned(trajs, paths, robot0, n_local, float(F.MARGIN))
    assert got.dtype == torch.int32 and torch.equal(got, want) and torch.equal(got, ma.count_collisions(trajs, paths, robot0, n_local))
    summ, robots, lst = ma.path_conflicts(paths, list_cap=500)
    s2, r2, l2 = torch.ops.mmd_amd.path_conflicts(paths, float(F.MARGIN), 500)
    assert torch.equal(s2[:1], summ[:1]) and torch.equal(s2[4:], summ[4:]) and torch.equal(r2, robots) and torch.equal(l2, lst)
    assert int(s2[0]) > 500
    assert torch.ops.mmd_amd.path_conflicts(paths, float(F.MARGIN), 0)[2].shape == (0, 12)
