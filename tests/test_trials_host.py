"""CPU: the trial layer's host side (mmd_amd.trials) and the NumPy restatement of the solution statistics (tests/trial_stats_ref.py)
against golden g24 -- the genuine reference functions (tools/make_golden_trials.py) on the inputs of tests/trial_cases.py.
Decisions (pair collisions, adherence) are exact, the +- 4e-7 cases included; path length and mean acceleration are bounded by
SUM_BOUND(Tg) = 2 Tg 2^-24 relative to the reference value (two summation orders of Tg non-negative fp32 terms)."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import trial_cases as TC
import trial_stats_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_trial_stats.npz")
MAPS = ("EnvEmpty2D", "EnvHighways2D", "EnvConveyor2D", "EnvDropRegion2D")
# the single-map problems of the reference (mmd/config/mmd_experiment_configs.py:53-167)
PROBLEMS = ("EnvEmpty2DRobotPlanarDiskCircle", "EnvEmpty2DRobotPlanarDiskRandom", "EnvHighways2DRobotPlanarDiskRandom",
            "EnvEmpty2DRobotPlanarDiskBoundary", "EnvConveyor2DRobotPlanarDiskBoundary", "EnvConveyor2DRobotPlanarDiskRandom",
            "EnvDropRegion2DRobotPlanarDiskRandom", "EnvHighways2DRobotPlanarDiskSmallCircle", "EnvDropRegion2DRobotPlanarDiskBoundary")


@pytest.fixture(scope="module")
def g24():
    return np.load(GOLDEN)


def assert_sums_close(got, want, Tg, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    assert (err <= R.SUM_BOUND(Tg) * np.abs(want)).all(), (what, float((err / np.maximum(np.abs(want), 1e-30)).max()), R.SUM_BOUND(Tg))


@pytest.mark.parametrize("name", list(TC.G24_CASES))
def test_restatement_matches_g24(g24, name):
    paths, tiles = TC.G24_CASES[name]()
    np.testing.assert_array_equal(paths, g24[name + ".paths"])                  # the regenerated inputs are the recorded ones
    np.testing.assert_array_equal(np.array(tiles, np.float64).reshape(-1, 5), g24[name + ".tiles"])
    st = R.solution_stats(paths, tiles)
    assert st["pair_collisions"] == int(g24[name + ".pair_collisions"])
    np.testing.assert_array_equal(st["adherence"], g24[name + ".adherence"])
    Tg = paths.shape[1]
    assert_sums_close(st["path_length"], g24[name + ".path_length"], Tg, "path_length")
    assert_sums_close(st["mean_accel"], g24[name + ".mean_accel"], Tg, "mean_accel")
    if tiles:
        want = g24[name + ".trial"]
        got = R.trial_means(len(paths), tiles, st["adherence"], st["path_length"], st["mean_accel"])
        assert got[0] == want[0]
        assert_sums_close(got[1:], want[1:3], Tg, "trial means")
        assert int(want[3]) == (2 if st["pair_collisions"] else 0)           # FAIL_COLLISION_AGENTS / SUCCESS


def test_g24_holds_the_cases_it_must(g24):
    """Both outcomes of every rule, the NaN cases, the decided highways sums, the row-63 quirk, collisions on padded rows."""
    for name in ("line", "highways", "conveyor", "drop_region"):
        a = g24[name + ".adherence"]
        assert (a == 0).any() and (a == 1).any(), name
    assert ((g24["line.adherence"] > 0) & (g24["line.adherence"] < 1)).any()
    np.testing.assert_array_equal(g24["line.adherence"], g24["line.adherence_nowait"])
    s = g24["highways.highways_sum"]
    assert np.isnan(s).sum() == 1 and (np.abs(s[~np.isnan(s)]) >= 1e-2).all() and (s > 0).any() and (s < 0).any()
    drop = g24["drop_region.adherence"]
    assert list(drop[:4]) == [1.0, 0.0, 0.0, 1.0]                # 16 rows, 15 rows, rows 48 .. 63, rows 47 .. 62
    conv = g24["conveyor.adherence"]
    assert list(conv[:6]) == [1.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    paths = g24["pairs.paths"]
    assert paths.shape[0] >= 6 and (paths[2, 0] == paths[2, 2]).all() and int(g24["pairs.pair_collisions"]) > 0
    assert g24["multi_tile.paths"].shape == (4, 192 + 15, 4) and len(set(g24["multi_tile.tiles"][:3, 4])) == 3
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("n", [3, 10, 12])
def test_formations_are_the_reference_values(g24, n):
    from mmd_amd import trials as T
    for name, (s, g) in (("circle", T.get_start_goal_pos_circle(n, radius=0.8)), ("small_circle", T.get_start_goal_pos_circle(n, radius=0.45)),
                         ("boundary", T.get_start_goal_pos_boundary(n, dist=0.87))):
        np.testing.assert_array_equal(torch.stack(s).numpy(), g24[f"{name}.{n}.start"])
        np.testing.assert_array_equal(torch.stack(g).numpy(), g24[f"{name}.{n}.goal"])
    np.testing.assert_array_equal(torch.stack(T.get_state_pos_column(n, -0.6)).numpy(), g24[f"column.{n}"])
    s, g, ids, skel = T.get_planning_problem("EnvHighways2DRobotPlanarDiskSmallCircle", n)
    first = min(n, 10)
    if n <= 10:
        np.testing.assert_array_equal(torch.stack(s).numpy(), g24[f"small_circle.{n}.start"])
    else:                                                    # the second ring above 10 agents
        np.testing.assert_array_equal(torch.stack(s[:first]).numpy(), g24["small_circle.10.start"])
        np.testing.assert_array_equal(torch.stack(g[first:]).numpy(), T.synth.start_goal_circle(n - 10, 0.65)[1])
    assert ids == [["EnvHighways2D-RobotPlanarDisk"]] and skel == [[[0, 0]]] * n


class _GridTask:
    """compute_collision of the reference task on the host: occupancy of the map's SDF at the robot radius."""

    def __init__(self, env):
        self.env = env

    def compute_collision(self, x, **kw):
        from mmd_amd import environments
        return environments.map_sdf(x[..., :2], self.env) < 0.05


class _HostRobot:
    radius = 0.05

    def check_rr_collisions(self, q):
        d = torch.norm(q[:, None] - q[None], dim=-1)
        hit = d < 2.1 * self.radius
        hit.fill_diagonal_(False)
        return hit, None


@pytest.mark.parametrize("env", MAPS)
def test_random_starts_and_goals(env):
    from mmd_amd import trials as T
    from mmd_amd.multi_agent_planners import is_multi_agent_start_goal_states_valid
    n = 20
    s, g = T.get_start_goal_pos_random_in_env(n, env, seed=3)
    s2, g2 = T.get_start_goal_pos_random_in_env(n, env, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(s + g, s2 + g2))
    s3, _ = T.get_start_goal_pos_random_in_env(n, env, seed=4)
    assert not torch.equal(torch.stack(s), torch.stack(s3))
    for pts in (torch.stack(s), torch.stack(g)):
        assert pts.shape == (n, 2) and pts.dtype == torch.float32 and float(pts.abs().max()) <= 0.95
        assert (T._grid_sdf(env, pts.numpy()) > 0.16).all()
        d = torch.cdist(pts.double(), pts.double()) + 10 * torch.eye(n)
        assert float(d.min()) > 0.15
    assert is_multi_agent_start_goal_states_valid(_HostRobot(), _GridTask(env), s, g)


def test_random_placement_gives_up():
    from mmd_amd import trials as T
    with pytest.raises(RuntimeError, match="EnvHighways2D.*margin=0.15.*obstacle_margin=0.16"):
        T.get_start_goal_pos_random_in_env(64, "EnvHighways2D", max_draws=2000)


def test_planning_problems_resolve():
    from mmd_amd import trials as T
    assert set(PROBLEMS) == set(T.PLANNING_PROBLEMS)
    for name in PROBLEMS:
        s, g, ids, skel = T.get_planning_problem(name, 4, seed=1)
        assert len(s) == len(g) == len(skel) == 4 and len(ids) == 1 and len(ids[0]) == 1
        assert name.startswith(ids[0][0].split("-")[0]) and ids[0][0].split("-")[0] in T.ADHERENCE_RULE
    for bad in ("EnvTestTwoByTwoRobotPlanarDiskRandom", "nope"):
        with pytest.raises(KeyError):
            T.get_planning_problem(bad, 4)


def test_experiment_expansion_order_and_sharing():
    """experiments.py:68-98: agent count -> planner class -> trial number; the problem of a trial number is drawn once and shared."""
    from mmd_amd import trials as T
    e = T.MultiAgentPlanningExperimentConfig()
    e.instance_name, e.num_agents_l, e.multi_agent_planner_class_l = "EnvEmpty2DRobotPlanarDiskRandom", [3, 5], ["ECBS", "PP"]
    e.single_agent_planner_class, e.num_trials_per_combination, e.stagger_start_time_dt, e.time_str = "MPD", 2, 1, "t"
    cs = e.get_single_trial_configs_from_experiment_config(seed=7)
    assert [(c.num_agents, c.multi_agent_planner_class, c.trial_number) for c in cs] == \
        [(n, p, k) for n in (3, 5) for p in ("ECBS", "PP") for k in (0, 1)]
    assert cs[0].start_state_pos_l is cs[2].start_state_pos_l and cs[1].goal_state_pos_l is cs[3].goal_state_pos_l
    assert not torch.equal(torch.stack(cs[0].start_state_pos_l), torch.stack(cs[1].start_state_pos_l))
    assert all(c.stagger_start_time_dt == 1 and c.single_agent_planner_class == "MPD" and c.runtime_limit == 60 for c in cs)
    again = e.get_single_trial_configs_from_experiment_config(seed=7)
    assert all(torch.equal(torch.stack(a.start_state_pos_l), torch.stack(b.start_state_pos_l)) for a, b in zip(cs, again))


def test_results_are_saved_readable_and_aggregated(tmp_path):
    from mmd_amd import trials as T
    results = []
    for k, (status, method) in enumerate([(T.TrialSuccessStatus.SUCCESS, "ECBS"), (T.TrialSuccessStatus.FAIL_COLLISION_AGENTS, "ECBS"),
                                          (T.TrialSuccessStatus.SUCCESS, "PP")]):
        c = T.MultiAgentPlanningSingleTrialConfig()
        c.num_agents, c.multi_agent_planner_class, c.single_agent_planner_class, c.instance_name, c.trial_number = 3, method, "MPD", "x", k
        c.start_state_pos_l = [torch.zeros(2)] * 3
        r = T.MultiAgentPlanningSingleTrialResult()
        r.trial_config, r.success_status, r.data_adherence, r.path_length_per_agent, r.num_collisions_in_solution = c, status, 0.5 + k, 2.0, k
        r.agent_path_l = [torch.zeros(3, 4)]
        d = T.get_result_dir_from_trial_config(c, str(tmp_path))
        r.save(d)
        c.save(d)
        assert sorted(os.listdir(d)) == ["config.json", "results.json", "results.txt"]
        assert json.load(open(os.path.join(d, "results.json")))["success_status"] == status.name
        assert "data_adherence" in open(os.path.join(d, "results.txt")).read()
        results.append(r)
    rows = list(csv.DictReader(open(T.combine_and_save_results_for_experiment(results, str(tmp_path)))))
    assert [(r["method"], r["num_agents"], r["num_trials"]) for r in rows] == [("ECBS", "3", "2"), ("PP", "3", "1")]
    assert float(rows[0]["success_rate"]) == 0.5 and float(rows[0]["fail_rate_collision_agents"]) == 0.5
    assert float(rows[0]["avg_data_adherence"]) == 0.5 and float(rows[1]["avg_data_adherence"]) == 2.5


def test_unknown_planner_classes_raise():
    from mmd_amd import trials as T
    c = T.MultiAgentPlanningSingleTrialConfig()
    c.num_agents, c.global_model_ids, c.agent_skeleton_l = 1, [["EnvEmpty2D-RobotPlanarDisk"]], [[[0, 0]]]
    c.start_state_pos_l, c.goal_state_pos_l = [torch.zeros(2)], [torch.ones(2) * 0.5]
    c.multi_agent_planner_class, c.single_agent_planner_class = "ECBS", "RRT"
    with pytest.raises(ValueError, match="single agent planner"):
        T.build_trial(c)
    c.multi_agent_planner_class, c.single_agent_planner_class = "A*", "MPD"
    with pytest.raises(ValueError, match="multi agent planner"):
        T.build_trial(c)
    c.multi_agent_planner_class, c.global_model_ids = "PP", [["EnvMaze2D-RobotPlanarDisk"]]
    with pytest.raises(ValueError, match="adherence"):
        T.build_trial(c)


def test_solution_stats_argument_checks_need_no_gpu():
    """mmd_solution_stats checks its host tile table and sizes before anything touches a device: the error returns and their text."""
    from mmd_amd import _lib, trials as T
    lib = _lib.load()
    for tiles, n, Tg, text in (([(0, 0, 0.0, 0.0, 7)], 2, 100, "tile 0 has unknown adherence rule 7"),
                               ([(0, 0, 0.0, 0.0, 0), (1, 37, 0.0, 0.0, 0)], 2, 100, "64 rows of tile 1 from row 37 do not fit in horizon_global = 100"),
                               ([(0, -1, 0.0, 0.0, 3)], 2, 100, "do not fit"),
                               ([(2, 0, 0.0, 0.0, 0)], 2, 100, "tile 0 names agent 2 of 2"),
                               ([], 0, 100, "n_agents = 0"),
                               ([], 2, 0, "horizon_global = 0")):
        rc = lib.mmd_solution_stats(0x1000, n, Tg, 0.1, T.tile_table(tiles), len(tiles), 0x2000, 0x3000, None)   # (never dereferenced)
        assert rc != 0 and text in lib.mmd_last_error().decode(), (text, lib.mmd_last_error())
