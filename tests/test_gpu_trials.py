"""-m gpu: mmd_solution_stats (csrc/trial_stats.hip) against golden g24 and, at sizes g24 does not hold, the NumPy restatement
(tests/trial_stats_ref.py); run_multi_agent_trial end to end against the same planners and search built by hand.
Exactness: pair collisions and adherence scores are exact (the +- 4e-7 cases included); path length and mean acceleration within
SUM_BOUND(Tg) = 2 Tg 2^-24 relative to the reference value (two summation orders of Tg non-negative fp32 terms; 2.5e-5 at Tg = 207)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases                              # noqa: E402
import trial_cases as TC                  # noqa: E402
import trial_stats_ref as R               # noqa: E402
from mmd_amd import synth                 # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_trial_stats.npz")


@pytest.fixture(scope="module")
def g24():
    return np.load(GOLDEN)


def _assert_sums_close(got, want, Tg, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    rel = float((err / np.maximum(np.abs(want), 1e-30)).max()) if err.size else 0.0
    print(f"{what}: max relative error {rel:.3e} (bound {R.SUM_BOUND(Tg):.3e})")
    assert (err <= R.SUM_BOUND(Tg) * np.abs(want)).all(), (what, rel, R.SUM_BOUND(Tg))


def _through_op(paths, tiles):
    import mmd_amd.ops  # noqa: F401
    from mmd_amd import trials as T
    out = torch.ops.mmd_amd.solution_stats(torch.from_numpy(paths).cuda(), torch.tensor(tiles, dtype=torch.float64).reshape(-1, 5),
                                           float(T.COLLISION_DIST))
    return T.SolutionStats(out.cpu().numpy(), paths.shape[0], len(tiles))


@pytest.mark.parametrize("via", ["ctypes", "op"])
@pytest.mark.parametrize("name", list(TC.G24_CASES))
def test_solution_stats_matches_g24(g24, name, via):
    from mmd_amd import trials as T
    paths, tiles = TC.G24_CASES[name]()
    np.testing.assert_array_equal(paths, g24[name + ".paths"])
    st = T.solution_stats(torch.from_numpy(paths).cuda(), tiles) if via == "ctypes" else _through_op(paths, tiles)
    assert st.pair_collisions == int(g24[name + ".pair_collisions"])
    np.testing.assert_array_equal(st.adherence, g24[name + ".adherence"])
    Tg = paths.shape[1]
    _assert_sums_close(st.path_length, g24[name + ".path_length"], Tg, name + " path_length")
    _assert_sums_close(st.mean_accel, g24[name + ".mean_accel"], Tg, name + " mean_accel")
    if tiles:
        got = R.trial_means(len(paths), tiles, st.adherence, st.path_length, st.mean_accel)
        want = g24[name + ".trial"]
        assert got[0] == want[0]
        _assert_sums_close(got[1:], want[1:3], Tg, name + " trial means")


@pytest.mark.parametrize("n_agents,stagger", [(64, 5), (256, 3)])
def test_solution_stats_at_scale(n_agents, stagger):
    """64 and 256 agents x 3 tiles with staggered starts (Tg = 507 / 957), every rule and piece family, margin pairs planted into random
    rows: against the NumPy restatement, which g24 pins."""
    from mmd_amd import trials as T
    paths, tiles = TC.scale_case(n_agents, stagger, 2410 + n_agents)
    assert paths.shape == (n_agents, 192 + (n_agents - 1) * stagger, 4) and len(tiles) == 3 * n_agents
    for t in tiles:                                       # the condition on highways inputs: the sign of the sum is decided
        if t[4] == R.RULE_HIGHWAYS:
            s = R.highways_sum(R.tile_points(paths, t))
            assert np.isnan(s) or abs(s) >= 1e-2
    want = R.solution_stats(paths, tiles)
    st = T.solution_stats(torch.from_numpy(paths).cuda(), tiles)
    assert want["pair_collisions"] > 0 and st.pair_collisions == want["pair_collisions"]
    np.testing.assert_array_equal(st.adherence, want["adherence"])
    assert len(set(want["adherence"].tolist())) > 2
    _assert_sums_close(st.path_length, want["path_length"], paths.shape[1], "path_length")
    _assert_sums_close(st.mean_accel, want["mean_accel"], paths.shape[1], "mean_accel")
    again = T.solution_stats(torch.from_numpy(paths).cuda(), tiles)                  # fixed-order sums: bitwise repeatable
    np.testing.assert_array_equal(again.path_length, st.path_length)
    np.testing.assert_array_equal(again.mean_accel, st.mean_accel)


def test_solution_stats_error_returns():
    """Argument checks only: nothing here reaches a kernel."""
    from mmd_amd import trials as T
    paths = torch.zeros((2, 100, 4), device="cuda")
    with pytest.raises(RuntimeError, match="unknown adherence rule 7"):
        T.solution_stats(paths, [(0, 0, 0.0, 0.0, 7)])
    with pytest.raises(RuntimeError, match="do not fit"):
        T.solution_stats(paths, [(0, 0, 0.0, 0.0, 0), (1, 37, 0.0, 0.0, 0)])
    with pytest.raises(RuntimeError, match="do not fit"):
        T.solution_stats(paths, [(0, -1, 0.0, 0.0, 0)])
    with pytest.raises(RuntimeError, match="agent 2 of 2"):
        T.solution_stats(paths, [(2, 0, 0.0, 0.0, 0)])
    with pytest.raises(RuntimeError, match="n_agents = 0"):
        T.solution_stats(torch.zeros((0, 100, 4), device="cuda"), [])
    st = T.solution_stats(paths, [(1, 36, 0.0, 0.0, 0)])                             # the last tile that fits
    assert st.pair_collisions == 100 and st.adherence.tolist() == [0.0] and st.path_length.tolist() == [0.0, 0.0]


def test_one_device_to_host_transfer_per_trial_statistics(monkeypatch):
    """The statistics of a solution cross to the host in ONE copy: one .cpu() of the summary buffer, no .item() / .tolist() / .numpy() of a
    device tensor anywhere in the call."""
    from mmd_amd import trials as T
    paths, tiles = TC.multi_tile_case()
    dev = [p for p in torch.from_numpy(paths).cuda()]                               # as the searches return a solution
    calls = []

    def counting(name):
        real = getattr(torch.Tensor, name)

        def wrapper(self, *a, **k):
            if self.is_cuda:
                calls.append((name, tuple(self.shape)))
            return real(self, *a, **k)
        return wrapper
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__"):
        monkeypatch.setattr(torch.Tensor, name, counting(name))
    st = T.solution_stats(dev, tiles)
    monkeypatch.undo()
    assert calls == [("cpu", (1 + 2 * len(dev) + len(tiles),))], calls
    assert st.pair_collisions == R.pair_collisions(paths)


# ---- run_multi_agent_trial end to end -----------------------------------------------------------------------------------------------------
def _weights(name):
    return cases.trained_state_dict() if name == "g19" else synth.synth_unet_state_dict(0)


def _trial_config(case):
    from mmd_amd import trials as T
    c = T.MultiAgentPlanningSingleTrialConfig()
    c.runtime_limit, c.time_str, c.instance_name = 120, "test", case
    if case == "ecbs_empty_circle":
        c.num_agents, c.multi_agent_planner_class, c.single_agent_planner_class = 5, "ECBS", "MPD"
        c.start_state_pos_l, c.goal_state_pos_l, c.global_model_ids, c.agent_skeleton_l = T.get_planning_problem("EnvEmpty2DRobotPlanarDiskCircle", 5)
    elif case == "pp_highways_small_circle":
        c.num_agents, c.multi_agent_planner_class, c.single_agent_planner_class = 5, "PP", "MPD"
        c.start_state_pos_l, c.goal_state_pos_l, c.global_model_ids, c.agent_skeleton_l = \
            T.get_planning_problem("EnvHighways2DRobotPlanarDiskSmallCircle", 5)
    else:                                                 # a 1 x 2 grid of EnvEmptyNoWait2D, 3 agents left to right, start times 0, 5, 10
        c.num_agents, c.multi_agent_planner_class, c.single_agent_planner_class, c.stagger_start_time_dt = 3, "XECBS", "MPDEnsemble", 5
        c.global_model_ids = [["EnvEmptyNoWait2D-RobotPlanarDisk", "EnvEmptyNoWait2D-RobotPlanarDisk"]]
        c.agent_skeleton_l = [[[0, 0], [0, 1]]] * 3
        c.start_state_pos_l = [torch.tensor([-0.6, y]) for y in (0.5, 0.0, -0.5)]
        c.goal_state_pos_l = [torch.tensor([0.6, -y]) for y in (0.5, 0.0, -0.5)]
    return c


def _planner_kwargs(case, weights):
    sd = _weights(weights)
    kw = dict(n_samples=16, model_args=dict(n_diffusion_steps=25))
    if case == "xecbs_ensemble_1x2":
        kw["model_state_dicts"] = [sd, sd]
    else:
        kw["model_state_dict"] = sd
    return kw


def _by_hand(case, weights, seed):
    """The same planners and search with the same seeds, wired here as tests/test_gpu_mapf.py wires them."""
    from mmd_amd import diffusion_model as dm
    from mmd_amd.multi_agent_planners import CBS, PrioritizedPlanning
    from mmd_amd.planners import MPD, MPDEnsemble
    sd = _weights(weights)
    common = dict(planner_alg="mmd", n_samples=16, model_args=dict(n_diffusion_steps=25), device="cuda", trained_models_dir="")
    if case == "xecbs_ensemble_1x2":
        tr = {0: torch.tensor([0.0, 0.0]), 1: torch.tensor([2.0, 0.0])}
        starts = [torch.tensor([-0.6, y]) + tr[0] for y in (0.5, 0.0, -0.5)]
        goals = [torch.tensor([0.6, -y]) + tr[1] for y in (0.5, 0.0, -0.5)]
        ps = [MPDEnsemble(model_ids=("EnvEmptyNoWait2D-RobotPlanarDisk",) * 2, transforms=tr, start_state_pos=starts[k], goal_state_pos=goals[k],
                          model_state_dicts=[sd, sd], seed=seed + k, **common) for k in range(3)]
        times = [0, 5, 10]
    else:
        env, (s, g) = ("EnvEmpty2D", synth.start_goal_circle(5, 0.8)) if case == "ecbs_empty_circle" else \
            ("EnvHighways2D", synth.start_goal_circle(5, 0.45))
        starts, goals = [torch.from_numpy(v) for v in s], [torch.from_numpy(v) for v in g]
        ps = [MPD(model_id=env + "-RobotPlanarDisk", start_state_pos=starts[k], goal_state_pos=goals[k], model_state_dict=sd, seed=seed + k,
                  **common) for k in range(5)]
        times = [0] * 5
    if case == "pp_highways_small_circle":
        alg = PrioritizedPlanning(ps, starts, goals, start_time_l=times)
    else:
        alg = CBS(ps, starts, goals, start_time_l=times, is_ecbs=True, is_xcbs=case == "xecbs_ensemble_1x2")
    dm._GLOBAL_DRAWS = 0
    return alg.plan(runtime_limit=120), times


# (case, weights): random-init weights as tests/test_gpu_mapf.py::test_end_to_end_over_mpd*; the briefly trained network of g19 (it denoises:
# smooth, free samples) where the statistics branch must be reached
TRIALS = [("ecbs_empty_circle", "g19"), ("pp_highways_small_circle", "synth"), ("xecbs_ensemble_1x2", "synth")]
REACHED = {}


@pytest.mark.parametrize("case,weights", TRIALS)
def test_run_multi_agent_trial_end_to_end(case, weights, tmp_path):
    """run_multi_agent_trial adds wiring, not behaviour: paths, expansions and search status bitwise those of the hand-built search; the
    four statistics equal the restatement on result.agent_path_l; success_status by the reference's rule; a second run is bitwise equal.
    Any search status is accepted except FAIL_RUNTIME_LIMIT, after which two runs have no reason to agree (the limit is 120 s; these
    searches take seconds).  The case that must reach the statistics branch is (ECBS, MPD, EnvEmpty2D circle radius 0.8, 5 agents) with the
    g19 network (see test_a_trial_reaches_the_statistics)."""
    from mmd_amd import trials as T
    from mmd_amd.multi_agent_planners import TrialSuccessStatus as S
    seed = 300
    config = _trial_config(case)
    r = T.run_multi_agent_trial(config, _planner_kwargs(case, weights), seed=seed, results_dir=str(tmp_path))
    (paths, n_exp, status, n_conf), times = _by_hand(case, weights, seed)
    print(case, weights, "search status", status, "expansions", n_exp, "conflicts", n_conf, "planning_time", round(r.planning_time, 2))
    assert status is not S.FAIL_RUNTIME_LIMIT
    assert r.search_status is status and len(r.agent_path_l) == len(paths)
    assert all(torch.equal(a, b) for a, b in zip(r.agent_path_l, paths))
    r2 = T.run_multi_agent_trial(config, _planner_kwargs(case, weights), seed=seed)
    assert r2.search_status is status and all(torch.equal(a, b) for a, b in zip(r2.agent_path_l, paths))
    for name in ("success_status", "num_collisions_in_solution", "data_adherence", "path_length_per_agent", "mean_path_acceleration_per_agent",
                 "num_ct_expansions"):
        assert getattr(r, name) == getattr(r2, name), name
    REACHED[case] = bool(status)
    if not status:                                        # the reference returns the search's status and leaves the statistics at 0
        assert r.success_status is status and r.num_collisions_in_solution == n_conf
        assert (r.data_adherence, r.path_length_per_agent, r.mean_path_acceleration_per_agent, r.num_ct_expansions) == (0.0, 0.0, 0.0, 0)
        return
    assert r.num_ct_expansions == n_exp
    host = torch.stack(paths).cpu().numpy()
    rule = T.ADHERENCE_RULE[config.global_model_ids[0][0].split("-")[0]]
    K = len(config.agent_skeleton_l[0])
    tiles = [(a, times[a] + k * 64, 2.0 * k, 0.0, rule) for a in range(len(paths)) for k in range(K)]
    want = R.solution_stats(host, tiles)
    assert r.num_collisions_in_solution == n_conf + want["pair_collisions"]
    assert r.success_status is (S.FAIL_COLLISION_AGENTS if r.num_collisions_in_solution > 0 else S.SUCCESS)
    adherence, length, accel = R.trial_means(len(paths), tiles, want["adherence"], want["path_length"], want["mean_accel"])
    print(case, "data_adherence", r.data_adherence, "path_length_per_agent", r.path_length_per_agent, "mean_accel",
          r.mean_path_acceleration_per_agent, "pair collisions", want["pair_collisions"])
    assert r.data_adherence == adherence
    _assert_sums_close([r.path_length_per_agent, r.mean_path_acceleration_per_agent], [length, accel], host.shape[1], case + " trial means")
    d = T.get_result_dir_from_trial_config(config, str(tmp_path))
    assert sorted(os.listdir(d)) == ["config.json", "results.json", "results.txt"]


def test_a_trial_reaches_the_statistics():
    """At least one of the three trials ends its search with SUCCESS, so the statistics branch above was compared (runs after them)."""
    assert len(REACHED) == len(TRIALS) and any(REACHED.values()), REACHED
