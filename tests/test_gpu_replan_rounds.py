"""-m gpu: subset rounds of MultiRobotSampler (replan_round, plan_rounds_subset(replan=)).  The yardstick is the invariant the feature
rests on: a subset round is an ordinary round of the permuted instance paths_all[perm], so its rows are checked with torch.equal against
plan_round / sample_local + best_paths of a sampler built on the permuted robots, against the unsharded call, and the loop against a
hand-driven loop of the public calls.  T = 25 and B = 4 synthetic weights."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import map_textures, multi_agent as ma, synth                       # noqa: E402
from mmd_amd.constraints import binned_collision_table                           # noqa: E402
from mmd_amd.multi_robot import MultiRobotSampler                                # noqa: E402
import replan_model as S                                                         # noqa: E402
import round_model as M                                                          # noqa: E402
from cases import H, D                                                           # noqa: E402

T, B = 25, 4
TABLES = ["dense", "binned"]


def _sampler(starts, goals, **kw):
    import gpu_common as gc
    return MultiRobotSampler(gc.hip_model(T), starts, goals, env_id="EnvEmpty2D", n_samples=B, **kw)


def _select(s, paths, mode, iters=8):
    """(selection for sampler s's shard, robot_counts) of the paths"""
    table = binned_collision_table(paths, s.robot0, s.n_local, s.radius)
    _, robots, _ = ma.path_conflicts(paths, table=table)
    return ma.select_replan(paths, table, robots, mode, iters), robots


def _crossing_8():
    """8 robots on rows far apart, moving left to right; robot 5 runs right to left 0.08 above robot 2's row: only 2 and 5 meet"""
    y = np.float32([-0.8, -0.55, -0.3, 0.0, 0.25, -0.22, 0.5, 0.75])
    starts = np.stack([np.full(8, -0.8, np.float32), y], 1)
    goals = np.stack([np.full(8, 0.8, np.float32), y], 1)
    starts[5, 0], goals[5, 0] = 0.8, -0.8
    paths = synth.straight_line_paths(starts, goals, H)
    t, a, b, _ = M.report(paths)
    assert len(t) > 0 and set(a.tolist()) == {2} and set(b.tolist()) == {5}
    return starts, goals, paths


# ---- 2. all selected: the full round ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
def test_every_robot_selected_is_the_full_round(table):
    starts, goals, p0 = M.instance_a()
    p0 = torch.from_numpy(p0).cuda()
    seed = 70
    full = _sampler(starts, goals, constraint_table=table)
    t_full, best_full = full.plan_round(p0, seed=seed)
    s = _sampler(starts, goals, constraint_table=table)
    sel, _ = _select(s, p0, "conflicted")
    assert sel.perm.tolist() == list(range(6)) and sel.read_header() == (6, 0, 6, 0)
    t_sub, best_sub, ids = s.replan_round(p0, sel, seed)
    assert ids.tolist() == list(range(6)) and t_sub.shape == (6 * B, H, D) and torch.isfinite(t_sub).all()
    assert torch.equal(t_sub, t_full) and torch.equal(best_sub, best_full)
    # with prev_trajs: sample_local + best_paths
    full.set_other_paths(p0)
    t_loc = full.sample_local(t_full, 3, 3, seed=seed + 1)
    best_loc = full.best_paths(t_loc, p0)
    t_sub2, best_sub2, _ = s.replan_round(p0, sel, seed + 1, prev_trajs=t_full)
    assert torch.equal(t_sub2, t_loc) and torch.equal(best_sub2, best_loc) and not torch.equal(t_sub2, t_sub)
    # the sampler's own guide was left alone
    assert s.guide._external_cons is None and s.guide._binned is None and s._collision is None


# ---- 3. a proper subset: the permuted instance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
def test_a_subset_round_is_the_round_of_the_permuted_instance(table):
    starts, goals, paths_np = _crossing_8()
    paths = torch.from_numpy(paths_np).cuda()
    seed = 71
    s = _sampler(starts, goals, constraint_table=table)
    sel, robots = _select(s, paths, "conflicted")
    perm = sel.perm.tolist()
    assert perm == [2, 5, 0, 1, 3, 4, 6, 7] and sel.read_header() == (2, 0, 2, 0)
    uploads = map_textures.N_TEXTURE_UPLOADS
    t_sub, best_sub, ids = s.replan_round(paths, sel, seed)
    assert map_textures.N_TEXTURE_UPLOADS == uploads                                    # the subset's guide shares the resident SDF texture
    assert ids.tolist() == [2, 5] and ids.is_cuda and t_sub.shape == (2 * B, H, D) and best_sub.shape == (2, H, 2)
    other = _sampler(starts[perm], goals[perm], constraint_table=table)
    paths_perm = paths[sel.perm.long()].contiguous()
    other.set_other_paths(paths_perm)
    t_perm = other.sample(seed=seed)
    best_perm = other.best_paths(t_perm, paths_perm)
    assert torch.isfinite(t_perm).all()
    assert torch.equal(t_sub, t_perm[:2 * B]) and torch.equal(best_sub, best_perm[:2])
    # not what the robots get in their own places: the noise is keyed by the place in the permuted instance
    s.set_other_paths(paths)
    assert not torch.equal(t_sub[B:], s.sample(seed=seed)[5 * B:6 * B])
    # "independent" on a single pair re-plans robot 2 alone, against robot 5's held path
    sel1, _ = _select(s, paths, "independent")
    t_one, best_one, ids_one = s.replan_round(paths, sel1, seed)
    assert ids_one.tolist() == [2] and sel1.perm.tolist() == [2, 0, 1, 3, 4, 5, 6, 7]
    perm1 = sel1.perm.tolist()
    other1 = _sampler(starts[perm1], goals[perm1], constraint_table=table)
    paths_perm1 = paths[sel1.perm.long()].contiguous()
    other1.set_other_paths(paths_perm1)
    t_perm1 = other1.sample(seed=seed)
    assert torch.equal(t_one, t_perm1[:B]) and torch.equal(best_one, other1.best_paths(t_perm1, paths_perm1)[:1])
    assert sorted(s._subset_guides) == [1, 2]                                     # one guide per subset size, kept


# ---- 4. sharded: the unsharded rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
def test_sharded_subset_round_gives_the_unsharded_rows(table):
    p = M.instance_b()
    starts, goals = np.clip(p[:, 0], -0.95, 0.95), np.clip(p[:, -1], -0.95, 0.95)
    paths = torch.from_numpy(p).cuda()
    seed = 72
    whole = _sampler(starts, goals, constraint_table=table)
    sel, _ = _select(whole, paths, "independent")
    n_sel = sel.read_header()[0]
    assert n_sel == 15                                                            # the model's figure for instance B
    t_all, best_all, ids_all = whole.replan_round(paths, sel, seed)
    assert t_all.shape == (n_sel * B, H, D) and torch.isfinite(t_all).all()
    parts = []
    for g in (0, 1):
        rank = _sampler(starts, goals, constraint_table=table, rank=g, world_size=2)
        sel_g, _ = _select(rank, paths, "independent")
        assert torch.equal(sel_g.perm, sel.perm) and sel_g.read_header()[0] == n_sel
        t_g, best_g, ids_g = rank.replan_round(paths, sel_g, seed)
        assert ids_g.numel() == sel_g.read_header()[2] > 0
        parts.append((t_g, best_g, ids_g + rank.robot0))
    assert parts[0][0].shape[0] + parts[1][0].shape[0] == n_sel * B
    for k, want in enumerate((t_all, best_all, ids_all)):
        assert torch.equal(torch.cat([q[k] for q in parts]), want), k


def test_a_rank_with_nothing_selected_launches_nothing():
    starts, goals, paths_np = _crossing_8()
    paths = torch.from_numpy(paths_np).cuda()
    whole = _sampler(starts, goals)
    sel, _ = _select(whole, paths, "conflicted")
    t_all, best_all, _ = whole.replan_round(paths, sel, 73)
    got = {}
    for g in range(4):                                                            # two robots a rank: robot 2 on rank 1, robot 5 on rank 2
        rank = _sampler(starts, goals, rank=g, world_size=4)
        sel_g, _ = _select(rank, paths, "conflicted")
        t_g, best_g, ids_g = rank.replan_round(paths, sel_g, 73)
        got[g] = (t_g, best_g, ids_g)
        if g in (0, 3):
            assert sel_g.read_header() == (2, 0 if g == 0 else 2, 0, 0)
            assert t_g.shape == (0, H, D) and best_g.shape == (0, H, 2) and ids_g.numel() == 0 and t_g.is_cuda and ids_g.is_cuda
            assert rank._subset_guides == {} and rank._collision is None          # no guide, no table: nothing was launched
    assert got[1][2].tolist() == [0] and got[2][2].tolist() == [1]
    assert torch.equal(torch.cat([got[1][0], got[2][0]]), t_all) and torch.equal(torch.cat([got[1][1], got[2][1]]), best_all)


# ---- 5. the loop -----------------------------------------------------------------------------------------------------------------------
def _circle_8():
    starts, goals = synth.start_goal_circle(8, 0.8)
    return starts, goals, torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()


def _hand_loop(s, p0, mode, seed, max_rounds, local_rounds):
    """plan_rounds_subset from the public calls; checks on the way that robots not selected keep their rows"""
    n = s.n_robots
    count0 = ma.read_summary(ma.path_conflicts(p0)[0])[0]
    trajs, paths = s.plan_round(p0, seed=seed)
    trajs = trajs.clone()
    counts, replanned, k = [count0], [n], 1
    while True:
        table = binned_collision_table(paths, 0, n, s.radius)
        summ, robots, _ = ma.path_conflicts(paths, table=table)
        counts.append(ma.read_summary(summ)[0])
        if k == max_rounds or counts[-1] == 0:
            break
        sel = ma.select_replan(paths, table, robots, mode, 8)
        n_sel = sel.read_header()[0]
        replanned.append(n_sel)
        if mode == "conflicted":
            assert n_sel == int((robots > 0).sum())
        ids = s.selected_local_ids(sel)
        prev = trajs.view(n, B, H, D)[ids].reshape(-1, H, D) if local_rounds else None
        t_sub, best_sub, ids = s.replan_round(paths, sel, seed + k, prev)
        old_paths, old_trajs = paths, trajs.clone()
        paths = paths.clone().index_copy_(0, ids, best_sub)
        trajs.view(n, B, H, D).index_copy_(0, ids, t_sub.view(-1, B, H, D))
        held = (sel.selected == 0).nonzero().view(-1)
        assert held.numel() == n - n_sel
        assert torch.equal(paths[held], old_paths[held]) and torch.equal(trajs.view(n, B, H, D)[held], old_trajs.view(n, B, H, D)[held])
        assert not torch.equal(trajs.view(n, B, H, D)[ids], old_trajs.view(n, B, H, D)[ids])
        k += 1
    return paths, trajs, counts, replanned, k


@pytest.mark.parametrize("local_rounds", [False, True], ids=["from_noise", "local_rounds"])
@pytest.mark.parametrize("mode", ["conflicted", "independent"])
def test_plan_rounds_subset_is_the_hand_driven_loop(mode, local_rounds):
    starts, goals, p0 = _circle_8()
    seed = 74
    res = _sampler(starts, goals).plan_rounds_subset(max_rounds=3, seed=seed, replan=mode, local_rounds=local_rounds)
    paths, trajs, counts, replanned, k = _hand_loop(_sampler(starts, goals), p0, mode, seed, 3, local_rounds)
    print(f"{mode}, local_rounds={local_rounds}: rounds {res.n_rounds}, conflicts {res.conflict_counts}, replanned {res.replanned_counts}")
    assert res.n_rounds == k >= 2 and res.conflict_counts == counts and res.replanned_counts == replanned
    assert res.replanned_counts[0] == 8 and all(0 < m <= 8 for m in res.replanned_counts[1:])
    assert torch.equal(res.paths_local, paths) and torch.equal(res.trajs, trajs)
    assert res.conflict_free == (counts[-1] == 0) and res.dropped_constraints is None
    if mode == "independent":
        assert all(m < 8 for m in res.replanned_counts[1:])                       # an independent set of a graph with an edge


def test_replan_all_is_plan_and_last_idx_keeps_the_held_robots():
    starts, goals, p0 = _circle_8()
    seed = 75
    a = _sampler(starts, goals).plan(max_rounds=2, seed=seed)
    s = _sampler(starts, goals)
    b = s.plan_rounds_subset(max_rounds=2, seed=seed, replan="all")
    assert torch.equal(a.paths_local, b.paths_local) and torch.equal(a.trajs, b.trajs) and a.conflict_counts == b.conflict_counts
    assert a.replanned_counts is None and b.replanned_counts is None and a.n_rounds == b.n_rounds == 2
    # last_idx: the picks of round 0, overwritten in round 1 for the selected robots only; every pick names the row of paths_local
    s1 = _sampler(starts, goals)
    r0 = s1.plan_rounds_subset(max_rounds=1, seed=seed, replan="independent")
    idx0 = s1.last_idx.clone()
    s2 = _sampler(starts, goals)
    r1 = s2.plan_rounds_subset(max_rounds=2, seed=seed, replan="independent")
    assert r0.n_rounds == 1 and r1.n_rounds == 2 and r1.replanned_counts[1] < 8
    sel, _ = _select(s1, r0.paths_local, "independent")
    held = (sel.selected == 0).nonzero().view(-1)
    assert torch.equal(s2.last_idx[held], idx0[held])
    tv = s2.unnormalize(r1.trajs).view(8, B, H, D)
    assert torch.equal(tv[torch.arange(8, device="cuda"), s2.last_idx.long()][..., :2], r1.paths_local)
