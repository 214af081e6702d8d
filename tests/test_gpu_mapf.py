"""-m gpu: the multi-agent search layer on the device (mmd_find_conflicts, mmd_scan_candidates, mmd_path_constraints) and the planners over it
(mmd_amd.multi_agent_planners: CBS / ECBS / XECBS, PrioritizedPlanning) against golden g23 -- the reference's searches driven by the
scripted planner of mapf_stub -- and end to end over real MPD / MPDEnsemble planners."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp32_forms                        # noqa: E402
import mapf_stub as st                   # noqa: E402
from mmd_amd import synth                # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_mapf.npz")
H = 64


@pytest.fixture(scope="module")
def g23():
    return np.load(GOLDEN)


def _case(g, name):
    for c in st.CASES:
        if c[0] == name:
            _, kind, flags, n, lengths, stagger, fail_at = c
            return kind, flags, n, lengths, [stagger * k for k in range(n)], st.make_script(n, lengths, fail_at, int(g[name + ".meta"][4]))
    raise KeyError(name)


def _dev_batches(script, n, entry):
    return [torch.from_numpy(script[k][entry][0]).cuda() for k in range(n)]


def _records(lst):
    from mmd_amd import multi_agent as ma
    t, a, b, pa, pb, mid = ma.decode_records(lst.cpu().numpy())
    return np.concatenate([np.stack([t, a, b], 1).astype(np.float32), pa, pb, mid], 1)


@pytest.mark.parametrize("name", [c[0] for c in st.CASES])
def test_find_conflicts_matches_g23(g23, name):
    """Both modes, staggered starts, mixed lengths: count, order, agent ids, t, positions and midpoints bitwise the reference's get_conflicts."""
    from mmd_amd import multi_agent as ma
    kind, _, n, lengths, starts, script = _case(g23, name)
    mode = ma.ORDERED if kind == "CBS" else ma.PAIRS
    for si in range(3):
        ix = [int(v) for v in g23[f"{name}.state{si}_ix"]]
        want = g23[f"{name}.state{si}_conflicts"]
        batches = _dev_batches(script, n, si % st.N_ENTRIES)
        table = ma.agent_table(batches, ix, starts)
        Tg = ma.global_horizon(lengths, starts)
        summ, _ = ma.find_conflicts(table, n, Tg, mode)
        count, first = ma.read_summary(summ)
        assert count == want.shape[0]
        _, lst = ma.find_conflicts(table, n, Tg, mode, list_cap=max(count, 1))
        got = _records(lst)[:count]
        cols = 9 if kind == "CBS" else 7
        np.testing.assert_array_equal(got[:, :cols], want[:, :cols])
        if count:
            assert (first[0], first[1], first[2]) == tuple(int(v) for v in want[0, :3])
            np.testing.assert_array_equal(np.concatenate([first[3], first[4]]), want[0, 3:7])
            # a short buffer: the first records, the count says how many there were
            _, short = ma.find_conflicts(table, n, Tg, mode, list_cap=2)
            np.testing.assert_array_equal(_records(short)[:min(2, count), :cols], want[:2, :cols])


def _loop_counts(ma, batches, ix, starts, lengths, agent, cand, mode):
    """The reference's loop: one get_conflicts per candidate."""
    out = []
    for c in cand:
        ixc = list(ix)
        ixc[agent] = int(c)
        table = ma.agent_table(batches, ixc, starts)
        out.append(ma.read_summary(ma.find_conflicts(table, len(batches), ma.global_horizon(lengths, starts), mode)[0])[0])
    return out


@pytest.mark.parametrize("name", ["pp_mixed", "ecbs", "xecbs"])
def test_scan_candidates_matches_the_reference_loop(g23, name):
    """The 'least_collisions' choice for every agent of a state: CBS (first free index with the smallest count) and PP (from idx_best_traj,
    strict '<'), in both counting modes; plus a case built so that the two rules pick different samples."""
    from mmd_amd import multi_agent as ma
    _, _, n, lengths, starts, script = _case(g23, name)
    ix = [int(v) for v in g23[f"{name}.state0_ix"]]
    batches = _dev_batches(script, n, 0)
    differed = False
    for agent in range(n):
        free = script[agent][1][1]
        if free.size == 0:
            free = np.arange(st.B)
        init = int(free[-1])
        cand_batch = batches[agent].clone()
        best_first = None
        for mode in (ma.ORDERED, ma.PAIRS):
            counts = _loop_counts(ma, batches, ix, starts, lengths, agent, free, mode)
            table = ma.agent_table(batches, ix, starts)
            Tg = ma.global_horizon(lengths, starts)
            res, got_counts = ma.scan_candidates(table, n, Tg, agent, cand_batch, torch.from_numpy(free).cuda(), mode, ma.SELECT_CBS,
                                                 with_counts=True)
            assert got_counts.cpu().tolist() == counts
            k = int(np.argmin(counts))
            assert res.cpu().tolist() == [int(free[k]), counts[k]]
            best_first = int(free[k])
            init_count = _loop_counts(ma, batches, ix, starts, lengths, agent, [init], mode)[0]
            pick, pick_count = init, init_count
            for c, cnt in zip(free, counts):
                if cnt < pick_count:
                    pick, pick_count = int(c), cnt
            res = ma.scan_candidates(table, n, Tg, agent, cand_batch, torch.from_numpy(free).cuda(), mode, ma.SELECT_PP, init_idx=init)
            assert res.cpu().tolist() == [pick, pick_count]
        # the last free sample made a copy of the CBS choice: the CBS rule keeps the first, the PP rule (from the last) keeps the last
        if best_first != init:
            tied = batches[agent].clone()
            tied[init] = tied[best_first]
            bt = list(batches)
            bt[agent] = tied
            table = ma.agent_table(bt, ix, starts)
            Tg = ma.global_horizon(lengths, starts)
            a = ma.scan_candidates(table, n, Tg, agent, tied, torch.from_numpy(free).cuda(), ma.ORDERED, ma.SELECT_CBS).cpu().tolist()
            b = ma.scan_candidates(table, n, Tg, agent, tied, torch.from_numpy(free).cuda(), ma.ORDERED, ma.SELECT_PP,
                                   init_idx=init).cpu().tolist()
            assert a[0] == best_first and b[0] == init and a[1] == b[1]
            differed = True
    assert differed


def _ref_pack(pc, weight):
    from mmd_amd.constraints import CostConstraint, pack_constraints
    cl = pc.constraint_list()
    groups = [[(CostConstraint(None, H, q_l=c.get_q_l(), traj_range_l=c.get_t_range_l(), radius_l=c.radius_l, is_soft=c.is_soft),
                weight) for c in cl]]
    return pack_constraints(groups, "cuda")


@pytest.mark.parametrize("name", ["pp", "pp_mixed", "ecbs", "xecbs"])
def test_path_constraints_table_is_the_packed_list(g23, name):
    """mmd_path_constraints (ECBS soft, PP hard; agent in the state or not) is bitwise the pack_constraints table of the equivalent list."""
    from mmd_amd import multi_agent as ma
    _, _, n, lengths, starts, script = _case(g23, name)
    ix = [int(v) for v in g23[f"{name}.state1_ix"]]
    batches = _dev_batches(script, n, 1)
    seen = 0
    for agent in range(n):
        if lengths[agent] != H:
            continue                                   # (an MPD agent: a 2-tile agent takes the list form)
        for n_state, soft in ((n, True), (agent, True), (agent, False)):
            pc = ma.PathConstraints(batches[:n_state], ix[:n_state], agent, starts, n_state=n_state, is_soft=soft)
            has, slots = pc.extent()
            ref = _ref_pack(pc, 0.5)
            if not has:
                assert ref is None
                continue
            ell, gso, gw, rgo = pc.build(0.5)
            if slots == 0:
                assert int(ref[1][-1]) == 0
                continue
            assert torch.equal(ell, ref[0][:slots]) and ref[0].shape[0] == slots
            assert torch.equal(gso, ref[1]) and torch.equal(gw, ref[2]) and torch.equal(rgo, ref[3])
            seen += 1
    assert seen >= 3


def _mpd(env, start, goal, seed, B=16, T=25, **over):
    from mmd_amd.planners import MPD
    kw = dict(model_id=env + "-RobotPlanarDisk", planner_alg="mmd", start_state_pos=torch.as_tensor(start), goal_state_pos=torch.as_tensor(goal),
              device="cuda", seed=seed, n_samples=B, model_state_dict=synth.synth_unet_state_dict(0), model_args=dict(n_diffusion_steps=T),
              trained_models_dir="")
    kw.update(over)
    return MPD(**kw)


def _same(a, b):
    for name in ("trajs_iters", "trajs_final", "trajs_final_free_idxs", "trajs_final_coll_idxs"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.idx_best_traj is None) == (b.idx_best_traj is None)
    if a.idx_best_traj is not None:
        assert int(a.idx_best_traj) == int(b.idx_best_traj)


def test_mpd_path_constraints_equal_the_constraint_list():
    """MPD(..., path_constraints=) is bitwise MPD(..., constraints_l=list) with the same seed -- soft after hard constraints, hard alone, a
    re-plan from an experience -- on its own and through plan_batched."""
    from mmd_amd import multi_agent as ma
    from mmd_amd.constraints import MultiPointConstraint
    from mmd_amd.planners import PathBatchExperience, plan_batched
    starts, goals = synth.start_goal_circle(6, 0.5)
    lines = synth.straight_line_paths(starts, goals, H)
    batches = [torch.from_numpy(np.concatenate([np.repeat(lines[k:k + 1], 4, 0), np.zeros((4, H, 2), np.float32)], -1)).cuda()
               for k in range(6)]
    times = [5 * k for k in range(6)]
    hard = [MultiPointConstraint(q_l=[torch.tensor([0.1, 0.2])], t_range_l=[(20, 27)])]
    r = 2
    p = _mpd("EnvEmpty2D", starts[r], goals[r], 31)
    s, g = torch.from_numpy(starts[r]), torch.from_numpy(goals[r])
    first = p(s, g, seed=500)
    exp = PathBatchExperience(first.trajs_final)
    pcs = [ma.PathConstraints(batches, [0, 1, 2, 3, 0, 1], r, times, is_soft=True),
           ma.PathConstraints(batches[:r], [0, 1], r, times, n_state=r, is_soft=False),
           ma.PathConstraints(batches, [3, 3, 3, 3, 3, 3], r, times, is_soft=True)]
    for k, (pc, h, e) in enumerate(((pcs[0], hard, None), (pcs[1], [], None), (pcs[2], hard, exp))):
        a = p(s, g, list(h) + pc.constraint_list(), e, seed=510 + k)
        b = p(s, g, h, e, path_constraints=pc, seed=510 + k)
        _same(a, b)
        assert p.guide.extra_cost_l == [[]]
    assert not torch.equal(p(s, g, hard, seed=510).trajs_final, p(s, g, hard, path_constraints=pcs[0], seed=510).trajs_final)
    # plan_batched: three agents' calls (path constraints as the sixth element) in one launch sequence == the list-form calls one by one
    ps = [_mpd("EnvEmpty2D", starts[k], goals[k], 40 + k) for k in range(3)]
    calls = [(ps[k], torch.from_numpy(starts[k]), torch.from_numpy(goals[k]), hard if k else None, None,
              ma.PathConstraints(batches, [0] * 6, k, times, is_soft=k != 1)) for k in range(3)]
    seeds = [700, 701, 702]
    got = plan_batched(calls, seeds=seeds)
    for k, c in enumerate(calls):
        want = c[0](c[1], c[2], list(c[3] or []) + c[5].constraint_list(), seed=seeds[k])
        _same(got[k], want)


class _FreeTask:
    def compute_collision(self, x, **kw):
        return torch.zeros(x.shape[:-1], dtype=torch.bool, device=x.device)


def _replay(g23, name, batch_expansions=True):
    from mmd_amd.multi_agent_planners import CBS, PrioritizedPlanning, PointConflict
    from mmd_amd.constraints import MultiPointConstraint
    from mmd_amd.planners import RobotPlanarDiskFacade
    kind, flags, n, lengths, starts, script = _case(g23, name)
    log = []
    robot = RobotPlanarDiskFacade("cuda")
    planners = [st.ScriptedPlanner(k, script[k], log, robot, _FreeTask(), device="cuda") for k in range(n)]
    s, g = st.starts_goals(n)
    sl, gl = [torch.from_numpy(v).cuda() for v in s], [torch.from_numpy(v).cuda() for v in g]
    if kind == "PP":
        alg = PrioritizedPlanning(planners, sl, gl, start_time_l=starts)
    else:
        alg = CBS(planners, sl, gl, start_time_l=starts, conflict_type_to_constraint_types={PointConflict: {MultiPointConstraint}},
                  batch_expansions=batch_expansions, **flags)
        alg.open_l = st.RecordingList()
    return kind, alg, log, alg.plan(runtime_limit=1e9)


@pytest.mark.parametrize("name", [c[0] for c in st.CASES])
def test_search_replays_g23(g23, name):
    """PrioritizedPlanning, CBS, ECBS, XECBS over the scripted planner: the call log (agents, constraints bitwise, experiences), every
    node's choices and conflict count, expansions, status, n_conflicts and the padded paths bitwise."""
    kind, alg, log, (paths, n_exp, status, n_conf) = _replay(g23, name)
    calls, cons, pts = st.log_to_arrays(log)
    np.testing.assert_array_equal(calls, g23[name + ".calls"])
    np.testing.assert_array_equal(cons, g23[name + ".cons"])
    np.testing.assert_array_equal(pts, g23[name + ".points"])
    if kind == "CBS":
        assert [r[0] for r in alg.open_l.record] == g23[name + ".nodes_ix"].tolist()
        assert [r[1] for r in alg.open_l.record] == g23[name + ".nodes_count"].tolist()
    else:
        assert [ix for _, ix, _ in alg.node_log] == g23[name + ".nodes_ix"][0].tolist()
        assert [c for _, _, c in alg.node_log] == g23[name + ".nodes_count"].tolist()
    assert [n_exp, status.value, n_conf] == g23[name + ".result"].tolist()
    np.testing.assert_array_equal(torch.stack(paths).cpu().numpy(), g23[name + ".result_paths"])


def _host_conflicts(paths):
    p = torch.stack(paths)[..., :2].cpu().numpy()                # [n, Tg, 2], already padded
    hit = fp32_forms.pos_norm(p[:, None], p[None]) < fp32_forms.MARGIN          # torch.norm's fp32 form
    hit[np.arange(len(p)), np.arange(len(p))] = False
    return int(hit.sum())


@pytest.mark.parametrize("alg_name", ["PP", "ECBS"])
def test_end_to_end_over_mpd(alg_name):
    """Synthetic weights, EnvEmpty2D, 5 robots on a circle, 16 samples, T = 25: the search finishes within its runtime limit; SUCCESS iff an
    independent host recomputation finds no conflict on the returned paths; batch_expansions True / False give bitwise the same result."""
    from mmd_amd import diffusion_model as dm
    from mmd_amd.multi_agent_planners import CBS, PrioritizedPlanning, TrialSuccessStatus
    starts, goals = synth.start_goal_circle(5, 0.7)
    results = []
    for batch in (True, False):
        dm._GLOBAL_DRAWS = 0                                     # (the same seed stream for both runs)
        ps = [_mpd("EnvEmpty2D", starts[k], goals[k], 60 + k) for k in range(5)]
        sl, gl = [torch.from_numpy(v) for v in starts], [torch.from_numpy(v) for v in goals]
        alg = PrioritizedPlanning(ps, sl, gl) if alg_name == "PP" else CBS(ps, sl, gl, is_ecbs=True, batch_expansions=batch)
        out = alg.plan(runtime_limit=120)
        paths, n_exp, status, n_conf = out
        assert status in (TrialSuccessStatus.SUCCESS, TrialSuccessStatus.FAIL_COLLISION_AGENTS, TrialSuccessStatus.FAIL_RUNTIME_LIMIT,
                          TrialSuccessStatus.FAIL_NO_SOLUTION)
        if status in (TrialSuccessStatus.SUCCESS, TrialSuccessStatus.FAIL_COLLISION_AGENTS):
            host = _host_conflicts(paths)
            assert (status is TrialSuccessStatus.SUCCESS) == (host == 0)
            assert n_conf == (host if alg_name == "ECBS" else host // 2)
        results.append(out)
        if alg_name == "PP":
            break
    if len(results) == 2:
        a, b = results
        assert a[1:] == b[1:]
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


def test_end_to_end_over_mpd_ensemble():
    """A 1 x 2 MPDEnsemble instance (paths of 128 steps) with start times staggered by 5: PP and ECBS finish, their status agrees with the
    host recomputation."""
    from mmd_amd.multi_agent_planners import CBS, PrioritizedPlanning, TrialSuccessStatus
    from mmd_amd.planners import MPDEnsemble
    sd = synth.synth_unet_state_dict(0)
    tr = {0: torch.tensor([0.0, 0.0]), 1: torch.tensor([2.0, 0.0])}
    ys = [0.5, 0.0, -0.5]
    starts = [torch.tensor([-0.6, y]) + tr[0] for y in ys]
    goals = [torch.tensor([0.6, -y]) + tr[1] for y in ys]
    for name in ("PP", "ECBS"):
        ps = [MPDEnsemble(model_ids=("EnvEmptyNoWait2D-RobotPlanarDisk",) * 2, transforms=tr, planner_alg="mmd", start_state_pos=starts[k],
                          goal_state_pos=goals[k], n_samples=16, model_state_dicts=[sd, sd], model_args=dict(n_diffusion_steps=25),
                          device="cuda", seed=80 + k) for k in range(3)]
        times = [0, 5, 10]
        alg = PrioritizedPlanning(ps, starts, goals, start_time_l=times) if name == "PP" else \
            CBS(ps, starts, goals, start_time_l=times, is_ecbs=True)
        paths, n_exp, status, n_conf = alg.plan(runtime_limit=120)
        assert paths[0].shape[0] == 128 + 10
        if status in (TrialSuccessStatus.SUCCESS, TrialSuccessStatus.FAIL_COLLISION_AGENTS):
            assert (status is TrialSuccessStatus.SUCCESS) == (_host_conflicts(paths) == 0)
