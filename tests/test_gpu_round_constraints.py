"""-m gpu: the round table of a many-robot round (mmd_round_constraints_init, mmd_round_soft_from_paths, mmd_conflict_constraints_append;
constraints.RoundConstraints) and MultiRobotSampler.plan_rounds(repair=, local_rounds=).  The yardsticks: for the table the numpy model of
round_model (pinned to mmd_pack_constraints by tests/test_round_constraints_host.py) and soft_constraints_from_paths; for the guided
step the list form through the host pack; for plan() hand-driven loops of the public calls.  Every comparison is exact: int32 words of
the tables, torch.equal of the trajectories."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                                                        # noqa: E402
from mmd_amd.constraints import (CostConstraint, MultiPointConstraint, RoundConstraints, binned_collision_table,   # noqa: E402
                                 soft_constraints_from_paths)
import round_model as M                                                          # noqa: E402
from cases import H, D                                                           # noqa: E402

T, B = 25, 4
W_HARD, W_SOFT = 2e-1, 2e-2

_CACHE = {}


def _instance(name):
    """(paths [N, H, 2] float32, its report, the next round's paths, their report), computed once"""
    if name not in _CACHE:
        p0 = M.instance_a()[2] if name == "A" else M.instance_b()
        if name == "A":                                                           # the next round: every line bent a little, still meeting
            p1 = p0 + np.float32(0.02) * np.sin(np.linspace(0, np.pi, H, dtype=np.float32))[None, :, None]
            p1 = p1.astype(np.float32)
        else:
            p1 = M.instance_b_next()
        _CACHE[name] = (p0, M.report(p0), p1, M.report(p1))
        for v in _CACHE[name]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _CACHE[name]


SHARDS = [("A", 0, 6), ("B", 0, 48), ("B", 16, 16)]
IDS = ["A", "B", "B_16_16"]


def _table(paths_np, robot0, n_local, hard_slots):
    paths = torch.from_numpy(np.array(paths_np)).cuda()
    rc = RoundConstraints(paths.shape[0], robot0, n_local, hard_slots, w_hard=W_HARD, w_soft=W_SOFT)
    return paths, rc


def _append(rc, paths):
    rc.append_conflicts(paths, binned_collision_table(paths, rc.robot0, rc.n_local))


def _hard_words(rc):
    """int32 words [n_local, hard_slots, H, 4] of the hard blocks"""
    S = rc.slots_per_robot
    return rc.ell.view(rc.n_local, S, H, 4)[:, :rc.hard_slots].cpu().numpy().view(np.int32)


def _assert_blocks(rc, blocks):
    got = _hard_words(rc)
    fill, dropped = rc.fill.cpu().numpy(), rc.dropped.cpu().numpy()
    for r, blk in enumerate(blocks):
        assert np.array_equal(fill[r], blk.fill), (r, fill[r], blk.fill)
        assert int(dropped[r]) == blk.dropped, (r, int(dropped[r]), blk.dropped)
        assert np.array_equal(got[r], blk.ell.view(np.int32)), r


# ---- 1. the table against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,robot0,n_local", SHARDS, ids=IDS)
def test_table_is_the_model_bit_for_bit(name, robot0, n_local):
    p0, rep0, _, _ = _instance(name)
    n_all = p0.shape[0]
    cap = max(int(b.count.max()) for b in M.blocks([rep0], robot0, n_local, 1))    # the model's own largest fill of these robots
    assert cap >= 4
    paths, rc = _table(p0, robot0, n_local, cap)
    S = cap + n_all - 1
    assert rc.ell.shape == (n_local * S, H, 4) and rc.fill.shape == (n_local, H) and rc.dropped.shape == (n_local,)
    # after init: offsets, weights, an inactive hard block, zeroed counters
    gso, gw, rgo = rc.gso.cpu().numpy(), rc.gw.cpu().numpy(), rc.rgo.cpu().numpy()
    want_gso = np.stack([np.arange(n_local) * S, np.arange(n_local) * S + cap], 1).reshape(-1).tolist() + [n_local * S]
    assert gso.tolist() == want_gso and rgo.tolist() == (2 * np.arange(n_local + 1)).tolist()
    assert np.array_equal(gw, np.tile(np.float32([W_HARD, W_SOFT]), n_local))
    assert np.array_equal(_hard_words(rc), np.broadcast_to(M.INACTIVE.view(np.int32), (n_local, cap, H, 4)))
    assert not rc.fill.any() and not rc.dropped.any()
    rc.set_soft(paths)
    _append(rc, paths)
    blocks = M.blocks([rep0], robot0, n_local, cap)
    assert all(b.dropped == 0 for b in blocks) and max(int(b.fill.max()) for b in blocks) == cap      # the cap is met, nothing is lost
    _assert_blocks(rc, blocks)
    assert not rc.dropped.any()
    # the soft block: soft_constraints_from_paths' rows, word for word; offsets and weights untouched by the two calls
    soft = soft_constraints_from_paths(paths, robot0, n_local, weight=W_SOFT)[0].view(n_local, n_all - 1, H, 4)
    got = rc.ell.view(n_local, S, H, 4)[:, cap:]
    assert torch.equal(got.view(torch.int32), soft.view(torch.int32))
    assert rc.gso.cpu().numpy().tolist() == want_gso and np.array_equal(rc.gw.cpu().numpy(), gw)
    ell, g1, g2, g3, uniform = rc.tensors()
    assert ell is rc.ell and uniform == rc.radius and RoundConstraints(n_all, robot0, n_local, 2, hard_radius=0.1).tensors()[4] == 0.0
    # reset: the hard block and the counters as after init, the soft block left alone
    rc.reset()
    assert np.array_equal(_hard_words(rc), np.broadcast_to(M.INACTIVE.view(np.int32), (n_local, cap, H, 4)))
    assert not rc.fill.any() and not rc.dropped.any() and torch.equal(rc.ell.view(n_local, S, H, 4)[:, cap:], soft)


# ---- 2. the cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,robot0,n_local", SHARDS, ids=IDS)
def test_cap_keeps_the_first_points_and_counts_the_rest(name, robot0, n_local):
    p0, rep0, _, _ = _instance(name)
    full = max(int(b.count.max()) for b in M.blocks([rep0], robot0, n_local, 1))
    cap = full - 1
    assert cap >= 1
    paths, rc = _table(p0, robot0, n_local, cap)
    _append(rc, paths)
    blocks = M.blocks([rep0], robot0, n_local, cap)
    _assert_blocks(rc, blocks)
    assert sum(b.dropped for b in blocks) > 0 and int(rc.dropped.sum()) == sum(b.dropped for b in blocks)
    # nothing was written past the hard block: a soft block filled with a sentinel before the call is intact
    rc.reset()
    rc.ell.view(n_local, rc.slots_per_robot, H, 4)[:, cap:] = 123.0
    _append(rc, paths)
    assert (rc.ell.view(n_local, rc.slots_per_robot, H, 4)[:, cap:] == 123.0).all()
    _assert_blocks(rc, blocks)


# ---- 3. append -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,robot0,n_local", SHARDS, ids=IDS)
def test_second_call_appends_behind_the_first(name, robot0, n_local):
    p0, rep0, p1, rep1 = _instance(name)
    full = max(int(b.count.max()) for b in M.blocks([rep0, rep1], robot0, n_local, 1))
    assert len(rep1[0]) > 0
    for cap in (full, max(full // 2, 1)):                                         # everything kept; the second round meets a full block
        paths0, rc = _table(p0, robot0, n_local, cap)
        _append(rc, paths0)
        _append(rc, torch.from_numpy(np.array(p1)).cuda())
        _assert_blocks(rc, M.blocks([rep0, rep1], robot0, n_local, cap))


def test_torch_ops_are_the_ctypes_path():
    import mmd_amd.ops  # noqa: F401
    p0, rep0, _, _ = _instance("B")
    robot0, n_local, cap = 16, 16, 6
    paths, rc = _table(p0, robot0, n_local, cap)
    rc.set_soft(paths)
    _append(rc, paths)
    ell, gso, gw, rgo, fill, dropped = torch.ops.mmd_amd.round_constraints_init(paths, 48, n_local, cap, W_HARD, W_SOFT)
    torch.ops.mmd_amd.round_soft_from_paths(ell, paths, robot0, n_local, cap, rc.radius)
    torch.ops.mmd_amd.conflict_constraints_append(ell, fill, dropped, paths, robot0, n_local, cap, 2, float(M.F.MARGIN), rc.radius)
    assert torch.equal(ell.view(torch.int32), rc.ell.view(torch.int32)) and torch.equal(fill, rc.fill) and torch.equal(dropped, rc.dropped)
    assert torch.equal(gso, rc.gso) and torch.equal(gw, rc.gw) and torch.equal(rgo, rc.rgo) and int(dropped.sum()) > 0


# ---- 4. the guided step ----------------------------------------------------------------------------------------------------------------
def _guide(n_local):
    import gpu_common as gc
    return gc.hip_guide("EnvEmpty2D", [[] for _ in range(n_local)], n_robots=n_local)


def _samples_near(paths_np, robot0, n_local, seed, scale=0.04):
    """normalised samples [n_local * B, H, D]: every local robot's path plus noise of `scale`, so that both groups act"""
    import gpu_common as gc
    t = np.zeros((n_local, B, H, D), np.float32)
    t[..., :2] = paths_np[robot0:robot0 + n_local, None]
    t += synth.synth_noise(seed, t.shape) * np.float32(scale)
    return gc.dataset().normalizer.normalize(torch.from_numpy(t.reshape(n_local * B, H, D))).contiguous()


def _steps(guide, x, n_local, n_steps=3):
    y = x.clone().cuda()
    guide.guide_steps(y, torch.zeros(n_local, 2, D, device="cuda"), 0, n_steps)
    assert torch.isfinite(y).all()
    return y.cpu()


def _list_form_guide(paths_np, rep, robot0, n_local):
    """per robot add_extra_costs([hard, soft], [2e-1, 2e-2]) from the decoded records and PathConstraints(...).constraint_list(); a robot
    without records gets only the soft one"""
    from mmd_amd.multi_agent import PathConstraints
    n_all = paths_np.shape[0]
    batches = [torch.from_numpy(np.concatenate([paths_np[j], np.zeros((H, 2), np.float32)], 1)[None].copy()) for j in range(n_all)]
    g = _guide(n_local)
    as_cost = lambda c: CostConstraint(None, H, q_l=c.get_q_l(), traj_range_l=c.get_t_range_l(), radius_l=c.get_radius_l(),   # noqa: E731
                                       is_soft=c.get_is_soft())
    with_hard = []
    for r in range(n_local):
        tc, mid = M.robot_points(rep, robot0 + r)
        soft = PathConstraints(batches, [0] * n_all, robot0 + r, is_soft=True).constraint_list()
        assert len(soft) == 1
        costs, weights = [as_cost(soft[0])], [W_SOFT]
        if len(tc):
            hard = MultiPointConstraint(q_l=[torch.from_numpy(q.copy()) for q in mid], t_range_l=[(int(c) - 2, int(c) + 2) for c in tc])
            costs, weights = [as_cost(hard)] + costs, [W_HARD] + weights
            with_hard.append(r)
        g.add_extra_costs(costs, weights, robot=r)
    return g, with_hard


@pytest.mark.parametrize("name,robot0,n_local", SHARDS, ids=IDS)
def test_round_table_step_is_bitwise_the_list_form(name, robot0, n_local):
    p0, rep0, _, _ = _instance(name)
    x = _samples_near(p0, robot0, n_local, 640)
    paths, rc = _table(p0, robot0, n_local, 32)
    rc.set_soft(paths)
    _append(rc, paths)
    assert not rc.dropped.any()                                                   # 32 slots hold every point of these instances
    g_round = _guide(n_local)
    g_round.set_packed_constraints(rc.tensors())
    g_list, with_hard = _list_form_guide(p0, rep0, robot0, n_local)
    g_soft = _guide(n_local)
    g_soft.set_packed_constraints(soft_constraints_from_paths(paths, robot0, n_local, weight=W_SOFT))
    y_round, y_list, y_soft, y_free = (_steps(g, x, n_local) for g in (g_round, g_list, g_soft, _guide(n_local)))
    assert torch.equal(y_round, y_list), float((y_round - y_list).abs().max())
    assert len(with_hard) >= 2 and not torch.equal(y_soft, y_free)
    by_robot = lambda y: y.view(n_local, B, H, D)                                 # noqa: E731
    differ = [r for r in range(n_local) if not torch.equal(by_robot(y_round)[r], by_robot(y_soft)[r])]
    print(f"{name} [{robot0}, {robot0 + n_local}): robots with records {with_hard}, robots that differ from the soft-only run {differ}")
    assert differ == with_hard, (differ, with_hard)                               # the robots in conflict, and only they
    if name == "A":
        assert with_hard == list(range(6))                                        # everyone meets at the centre
    # the general path (two radii: no compact staging) gives the same bits as its list form would: here, the same radius passed twice
    rc2 = RoundConstraints(p0.shape[0], robot0, n_local, 32, w_hard=W_HARD, w_soft=W_SOFT)
    rc2.set_soft(paths)
    _append(rc2, paths)
    g_gen = _guide(n_local)
    g_gen.set_packed_constraints(rc2.tensors()[:4] + (0.0,))
    assert torch.equal(_steps(g_gen, x, n_local), y_round)


def test_round_table_on_conflict_free_paths_is_the_soft_table():
    """an all-inactive hard group adds +0 and changes no bit"""
    n = 6
    starts = np.float32([[-0.8, -0.375 + 0.15 * k] for k in range(n)])            # parallel lines 0.15 apart: above the 0.105 margin,
    goals = np.float32([[0.8, -0.375 + 0.15 * k] for k in range(n)])              # inside the 0.12 constraint radius of noisy samples
    p = synth.straight_line_paths(starts, goals, H)
    assert len(M.report(p)[0]) == 0
    paths, rc = _table(p, 0, n, 32)
    rc.set_soft(paths)
    _append(rc, paths)
    assert not rc.fill.any() and not rc.dropped.any()
    x = _samples_near(p, 0, n, 641)
    g_round, g_soft = _guide(n), _guide(n)
    g_round.set_packed_constraints(rc.tensors())
    g_soft.set_packed_constraints(soft_constraints_from_paths(paths, 0, n, weight=W_SOFT))
    y_round, y_soft, y_free = (_steps(g, x, n) for g in (g_round, g_soft, _guide(n)))
    assert torch.equal(y_round, y_soft) and not torch.equal(y_soft, y_free)


# ---- 5. plan_rounds(repair=True) --------------------------------------------------------------------------------------------------------------
def _sampler(**kw):
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    starts, goals, _ = M.instance_a()
    return MultiRobotSampler(gc.hip_model(T), starts, goals, env_id="EnvEmpty2D", n_samples=B, **kw)


def _repair_round(s, rc, paths_all, seed):
    """one repair round from the public pieces: table, hard points, soft block, sampling, pick"""
    table = binned_collision_table(paths_all, s.robot0, s.n_local, s.radius)
    rc.append_conflicts(paths_all, table)
    rc.set_soft(paths_all)
    s.guide.set_packed_constraints(rc.tensors())
    trajs = s.sample(seed=seed)
    return trajs, s.best_paths(trajs, paths_all, collision_table=table)


def test_plan_repair_is_deterministic_and_accumulates_the_rounds_conflicts():
    from mmd_amd import multi_agent as ma
    seed = 50
    res = [(_s, _s.plan_rounds(max_rounds=2, seed=seed, repair=True)) for _s in (_sampler(), _sampler())]
    (s1, r1), (s2, r2) = res
    assert r1.n_rounds == 2 and r1.conflict_counts[0] > 0
    assert torch.equal(r1.paths_local, r2.paths_local) and r1.conflict_counts == r2.conflict_counts
    assert torch.equal(s1.round_constraints.fill, s2.round_constraints.fill) and torch.equal(r1.trajs, r2.trajs)
    assert r1.dropped_constraints is s1.round_constraints.dropped and r1.dropped_constraints.shape == (6,)
    # by hand: the same two rounds from the public pieces
    hand = _sampler()
    rc = RoundConstraints(6, 0, 6, 32, hand.radius, W_HARD, hand.w_soft)
    p0 = torch.from_numpy(M.instance_a()[2]).cuda()
    t1, p1 = _repair_round(hand, rc, p0, seed)
    t2, p2 = _repair_round(hand, rc, p1, seed + 1)
    assert torch.equal(r1.trajs, t2) and torch.equal(r1.paths_local, p2)
    counts = [ma.read_summary(ma.path_conflicts(p)[0])[0] for p in (p0, p1, p2)]
    print(f"repair: conflicts per report {counts}, fill max {int(rc.fill.max())}, dropped {int(rc.dropped.sum())}")
    assert r1.conflict_counts == counts
    # fill and dropped: the model on the conflicts of the path sets of the rounds that sampled
    blocks = M.blocks([M.report(p0.cpu().numpy()), M.report(p1.cpu().numpy())], 0, 6, 32)
    fill, dropped = s1.round_constraints.fill.cpu().numpy(), r1.dropped_constraints.cpu().numpy()
    for r, blk in enumerate(blocks):
        assert np.array_equal(fill[r], blk.fill) and int(dropped[r]) == blk.dropped, r
    assert np.array_equal(_hard_words(s1.round_constraints), np.stack([b.ell for b in blocks]).view(np.int32))
    # the repair acted: round 0 of a soft-only plan starts from the same noise and ends elsewhere
    soft_only = _sampler().plan(max_rounds=1, seed=seed)
    assert not torch.equal(soft_only.trajs, t1) and soft_only.dropped_constraints is None
    # a second plan() on the same sampler starts from an empty hard block
    again = s1.plan_rounds(max_rounds=2, seed=seed, repair=True)
    assert torch.equal(again.paths_local, r1.paths_local) and torch.equal(s1.round_constraints.fill, s2.round_constraints.fill)


def test_plan_with_default_arguments_is_the_loop_of_plan_round_calls():
    seed = 51
    hand = _sampler()
    p0 = torch.from_numpy(M.instance_a()[2]).cuda()
    t1, p1 = hand.plan_round(p0, seed=seed)
    t2, p2 = hand.plan_round(p1, seed=seed + 1)
    s = _sampler()
    res = s.plan(max_rounds=2, seed=seed)
    assert res.n_rounds == 2 and torch.equal(res.trajs, t2) and torch.equal(res.paths_local, p2)
    res_r = _sampler().plan_rounds(max_rounds=2, seed=seed)                       # the new loop with its arguments at their defaults
    assert torch.equal(res_r.trajs, t2) and torch.equal(res_r.paths_local, p2) and res_r.conflict_counts == res.conflict_counts
    assert res.dropped_constraints is None and s.round_constraints is None and s._collision is None
    want = [len(M.report(p.cpu().numpy())[0]) for p in (p0, p1, p2)]
    assert res.conflict_counts == want


# ---- 6. plan_rounds(local_rounds=True) --------------------------------------------------------------------------------------------------------
def test_local_rounds_replan_from_the_previous_samples():
    from mmd_amd.diffusion_model import ddpm_sample_fn
    seed = 52
    s = _sampler()
    res = s.plan_rounds(max_rounds=2, seed=seed, local_rounds=True)
    assert res.n_rounds == 2
    hand = _sampler()
    p0 = torch.from_numpy(M.instance_a()[2]).cuda()
    t0, p1 = hand.plan_round(p0, seed=seed)
    hand.set_other_paths(p1)
    t1 = hand.model.run_local_inference(
        t0, 3, 3, None, hand.hard_conds, n_samples=B, n_robots=6, horizon=H, sample_fn=ddpm_sample_fn, guide=hand.guide,
        n_guide_steps=hand.n_guide_steps, t_start_guide=hand.t_start_guide, noise_std_extra_schedule_fn=lambda t: 0.5,
        n_diffusion_steps_without_noise=hand.n_extra, seed=seed + 1, traj_index_base=0, device="cuda")
    assert torch.isfinite(t1).all() and torch.equal(res.trajs, t1) and torch.equal(res.paths_local, hand.best_paths(t1, p1))
    assert not torch.equal(t1, hand.sample(seed=seed + 1))                        # not the round from noise
    assert float((t1 - t0).abs().max()) > 0
    # two ranks played on this GPU, the gather done by hand: the unsharded rows
    ranks = [_sampler(rank=g, world_size=2) for g in (0, 1)]
    assert [(r.robot0, r.n_local) for r in ranks] == [(0, 3), (3, 3)]
    t0_r, p1_r = [], []
    for r in ranks:
        r.set_other_paths(p0)
        t0_r.append(r.sample(seed=seed))
        p1_r.append(r.best_paths(t0_r[-1], p0))
    assert torch.equal(torch.cat(t0_r), t0) and torch.equal(torch.cat(p1_r), p1)
    t1_r = []
    for r, prev in zip(ranks, t0_r):
        r.set_other_paths(p1)
        t1_r.append(r.sample_local(prev, 3, 3, seed=seed + 1))
    assert torch.equal(t1_r[0], t1[:3 * B])
    assert torch.equal(t1_r[1], t1[3 * B:])                                       # rank 1 noises its rows with the unsharded draws
    # both flags together run, and local rounds see the repaired table
    both = _sampler().plan_rounds(max_rounds=2, seed=seed, repair=True, local_rounds=True)
    assert both.n_rounds == 2 and torch.isfinite(both.trajs).all() and not torch.equal(both.trajs, t1)
