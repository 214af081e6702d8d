"""The trial layer: named planning problems, one-call trials and the statistics of the returned solution.

Mirrors reference scripts/inference/inference_multi_agent.py:81-366 (run_multi_agent_trial), mmd/config/mmd_experiment_configs.py:36-167
(the single-map planning problems), mmd/common/multi_agent_utils.py:146-225 (start / goal generators), mmd/common/experiments/experiments.py:
47-275 (config / result types) and experiment_utils.py:84-196 (the aggregated table): same class, function and field names.  The statistics
of a solution (agent pairs in collision at 2.0 r, data adherence per tile, path length and mean acceleration per agent) come from ONE device
call (mmd_solution_stats, csrc/trial_stats.hip) and ONE device -> host copy; the reference's loop syncs once per (t, i, j).

Seeds.  `run_multi_agent_trial(config, seed=s)` builds agent k's planner with seed s + k (the reference gives every planner
MMDParams.seed) and sets the process-wide draw counter of mmd_amd.diffusion_model to 0 before the search, so every sampling call of the
trial draws the stream seed (planner seed << 24) + call number: two trials with the same config and seed are bitwise equal.

Deviations from the reference:
  * get_start_goal_pos_random_in_env draws from numpy.random.Generator(PCG64(seed)) -- the reference draws from the global torch
    generator, so values cannot and need not match -- and gives up after `max_draws` draws with a RuntimeError (the reference loops forever);
  * the two multi-tile problems (hand-written skeleton tables) are not named problems: multi-tile trials take global_model_ids and
    agent_skeleton_l from the caller;
  * a tile env without an adherence rule raises ValueError (env_base.py:281 opens a plot window and returns -inf);
  * results are saved as results.txt / results.json / config.json, no pickles; nothing is rendered; the reference robot / task are built
    from the tile maps directly, not from one more planner (which would load one more set of weights only to be dropped).
"""
import csv
import json
import os
import time
from typing import List

import numpy as np
import torch

from . import _lib, environments, synth
from .multi_agent_planners import CBS, PrioritizedPlanning, TrialSuccessStatus

__all__ = ["get_start_goal_pos_circle", "get_start_goal_pos_boundary", "get_state_pos_column", "get_start_goal_pos_random_in_env",
           "get_planning_problem", "PLANNING_PROBLEMS", "MultiAgentPlanningSingleTrialConfig", "MultiAgentPlanningSingleTrialResult",
           "MultiAgentPlanningExperimentConfig", "TrialSuccessStatus", "run_multi_agent_trial", "run_experiment", "solution_stats",
           "SolutionStats", "ADHERENCE_RULE", "get_result_dir_from_trial_config", "combine_and_save_results_for_experiment"]

HORIZON = 64                                   # mmd_params.py:34
ROBOT_RADIUS = 0.05                            # mmd_params.py:30
COLLISION_DIST = 2.0 * ROBOT_RADIUS            # inference_multi_agent.py:291
RUNTIME_LIMIT = 60                             # mmd_params.py:56
TILE_WIDTH = TILE_HEIGHT = 2.0                 # inference_multi_agent.py:146-147
ADHERENCE_RULE = {"EnvEmpty2D": _lib.ADHERENCE_LINE, "EnvEmptyNoWait2D": _lib.ADHERENCE_LINE, "EnvHighways2D": _lib.ADHERENCE_HIGHWAYS,
                  "EnvConveyor2D": _lib.ADHERENCE_CONVEYOR, "EnvDropRegion2D": _lib.ADHERENCE_DROP_REGION}


# ---- start / goal generators (multi_agent_utils.py:146-225), tile frame ---------------------------------------------------------------
def _as_list(a):
    return [torch.from_numpy(np.ascontiguousarray(v)) for v in a]


def get_start_goal_pos_circle(num_agents: int, radius=0.8):
    """multi_agent_utils.py:146-154: float64 cos / sin cast to float32 (CPU tensors; the planners move them)."""
    starts, goals = synth.start_goal_circle(num_agents, radius)
    return _as_list(starts), _as_list(goals)


def get_start_goal_pos_boundary(num_agents: int, dist=0.87):
    """multi_agent_utils.py:157-173."""
    starts, goals = synth.start_goal_boundary(num_agents, dist)
    return _as_list(starts), _as_list(goals)


def get_state_pos_column(num_agents: int, x_pos: float):
    """multi_agent_utils.py:176-180."""
    return _as_list(np.array([[x_pos, 0.8 * (1 - 2 * i / num_agents)] for i in range(num_agents)], dtype=np.float32))


def _grid_sdf(env_name, points):
    """The map's SDF GRID value at float32 points [n, 2]: GridMapSDF's cell lookup (grid_map_sdf.py:81-99) on the grid of
    environments.sdf_grid_texture."""
    return environments.texel_values(environments.sdf_grid_texture(env_name), points)[0]


def get_start_goal_pos_random_in_env(num_agents, env_name, margin=0.15, obstacle_margin=0.16, seed=0, max_draws=200000):
    """multi_agent_utils.py:183-225: points uniform in +-0.95, accepted one after the other iff the map's SDF grid value is
    > obstacle_margin and every distance to the points before is > margin; starts and goals drawn separately.  Drawn from
    numpy.random.Generator(PCG64(seed)): the reference uses the global torch generator, so its values cannot and need not match.  The
    reference's loop never gives up; this one raises RuntimeError after max_draws draws (64 agents do not fit on EnvHighways2D at the
    default margins)."""
    env_name = getattr(env_name, "__name__", env_name)
    rng = np.random.Generator(np.random.PCG64(seed))
    draws, out = 0, []
    for _ in range(2):
        state_b = np.zeros((0, 2), np.float32)
        while len(state_b) < num_agents:
            if draws >= max_draws:
                raise RuntimeError(f"get_start_goal_pos_random_in_env: {num_agents} agents not placed on {env_name} after {max_draws} draws "
                                   f"(margin={margin}, obstacle_margin={obstacle_margin})")
            draws += 1
            new_state = (rng.random((1, 2), dtype=np.float32) * np.float32(1.9) - np.float32(0.95)).astype(np.float32)
            if not _grid_sdf(env_name, new_state)[0] > obstacle_margin:
                continue
            d = new_state - state_b
            if len(state_b) and not np.all(np.sqrt(np.sum(d * d, axis=1)) > margin):
                continue
            state_b = np.concatenate([state_b, new_state])
        out.append(_as_list(state_b))
    return out[0], out[1]


# ---- planning problems (mmd_experiment_configs.py:36-167) -----------------------------------------------------------------------------
def _small_circle(num_agents, seed):
    starts, goals = get_start_goal_pos_circle(min(num_agents, 10), radius=0.45)
    if num_agents > 10:                                                  # a second ring (mmd_experiment_configs.py:148-152)
        more_starts, more_goals = get_start_goal_pos_circle(num_agents - 10, radius=0.65)
        starts, goals = starts + more_starts, goals + more_goals
    return starts, goals


def _random(env):
    return lambda n, seed: get_start_goal_pos_random_in_env(n, env, margin=0.15, seed=seed)


# the single-map problems of mmd_experiment_configs.py:53-167 (nine classes): name -> (env, generator(num_agents, seed))
PLANNING_PROBLEMS = {
    "EnvEmpty2DRobotPlanarDiskCircle": ("EnvEmpty2D", lambda n, seed: get_start_goal_pos_circle(n, radius=0.8)),
    "EnvEmpty2DRobotPlanarDiskRandom": ("EnvEmpty2D", _random("EnvEmpty2D")),
    "EnvHighways2DRobotPlanarDiskRandom": ("EnvHighways2D", _random("EnvHighways2D")),
    "EnvEmpty2DRobotPlanarDiskBoundary": ("EnvEmpty2D", lambda n, seed: get_start_goal_pos_boundary(n, dist=0.87)),
    "EnvConveyor2DRobotPlanarDiskBoundary": ("EnvConveyor2D", lambda n, seed: get_start_goal_pos_boundary(n, dist=0.87)),
    "EnvConveyor2DRobotPlanarDiskRandom": ("EnvConveyor2D", _random("EnvConveyor2D")),
    "EnvDropRegion2DRobotPlanarDiskRandom": ("EnvDropRegion2D", _random("EnvDropRegion2D")),
    "EnvHighways2DRobotPlanarDiskSmallCircle": ("EnvHighways2D", _small_circle),
    "EnvDropRegion2DRobotPlanarDiskBoundary": ("EnvDropRegion2D", lambda n, seed: get_start_goal_pos_boundary(n)),
}


def get_planning_problem(planning_problem_class_name: str, num_agents: int, seed=0):
    """-> (start_state_pos_l, goal_state_pos_l, global_model_ids, agent_skeleton_l) of a single-map problem; `seed` feeds the random
    placements only."""
    if planning_problem_class_name not in PLANNING_PROBLEMS:
        raise KeyError(f"unknown planning problem {planning_problem_class_name!r} (known: {sorted(PLANNING_PROBLEMS)}; multi-tile trials "
                       f"take global_model_ids and agent_skeleton_l from the caller)")
    env, generate = PLANNING_PROBLEMS[planning_problem_class_name]
    starts, goals = generate(num_agents, seed)
    return starts, goals, [[env + "-RobotPlanarDisk"]], [[[0, 0]]] * num_agents


# ---- config / result types (experiments.py:47-275) ------------------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy().tolist()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, TrialSuccessStatus):
        return v.name
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return v


class MultiAgentPlanningSingleTrialConfig:
    def __init__(self):
        self.time_str = None
        self.trial_number = 0
        self.runtime_limit = 10
        self.num_agents = 1
        self.stagger_start_time_dt = 0
        self.multi_agent_planner_class = ""                # "CBS", "ECBS", "XCBS", "XECBS" or "PP"
        self.single_agent_planner_class = ""               # "MPD" or "MPDEnsemble"
        self.render_animation = False
        self.instance_name = ""
        self.start_state_pos_l = []                        # tile frame of the first / last skeleton tile
        self.goal_state_pos_l = []
        self.global_model_ids = []                         # [row][col] -> model id
        self.agent_skeleton_l = []                         # per agent: [[row, col], ...]

    def to_dict(self):
        return {k: _plain(v) for k, v in vars(self).items()}

    def save(self, results_dir: str):
        os.makedirs(results_dir, exist_ok=True)
        with open(os.path.join(results_dir, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=1)

    def __str__(self):
        return (f"Trial Config:\n    Time Str: {self.time_str}\n    Trial Number: {self.trial_number}\n    Num Agents: {self.num_agents}\n"
                f"    Stagger Start Time: {self.stagger_start_time_dt}\n    Multi-agent Planner Class: {self.multi_agent_planner_class}\n"
                f"    Single Agent Planner: {self.single_agent_planner_class}\n    Instance: {self.instance_name}\n")


class MultiAgentPlanningSingleTrialResult:
    def __init__(self):
        self.trial_config = None
        self.agent_path_l = []                             # globally padded, [Tg, 4] each
        self.num_ct_expansions = 0
        self.success_status = TrialSuccessStatus.UNKNOWN
        self.num_collisions_in_solution = 0
        self.data_adherence = 0.0
        self.planning_time = 0.0
        self.path_length_per_agent = 0.0
        self.mean_path_acceleration_per_agent = 0.0
        self.start_state_pos_l = []                        # global frame
        self.goal_state_pos_l = []
        self.global_model_ids = []
        self.agent_skeleton_l = []

    def to_dict(self, with_paths=True):
        d = {k: _plain(v) for k, v in vars(self).items() if k not in ("trial_config", "agent_path_l")}
        d["trial_config"] = self.trial_config.to_dict() if self.trial_config is not None else None
        if with_paths:
            d["agent_path_l"] = _plain(self.agent_path_l)
        return d

    def save(self, results_dir: str):
        os.makedirs(results_dir, exist_ok=True)
        with open(os.path.join(results_dir, "results.json"), "w") as f:
            json.dump(self.to_dict(), f)
        with open(os.path.join(results_dir, "results.txt"), "w") as f:
            f.write(str(self))

    def __str__(self):
        c = self.trial_config
        head = "" if c is None else (f"Trial Config Summary:\n    Method: {c.multi_agent_planner_class}\n    Num Agents: {c.num_agents}\n"
                                     f"    Instance: {c.instance_name}\n    Stagger Start Time: {c.stagger_start_time_dt}\n"
                                     f"    Single Agent Planner: {c.single_agent_planner_class}\n")
        return (head + f"Planning Problem:\n    start_state_pos_l: {_plain(self.start_state_pos_l)}\n    goal_state_pos_l: {_plain(self.goal_state_pos_l)}\n"
                f"    global_model_ids: {self.global_model_ids}\n    agent_skeleton_l: {self.agent_skeleton_l}\n"
                f"Trial Results:\n    success_status: {self.success_status}\n    num_collisions_in_solution: {self.num_collisions_in_solution}\n"
                f"    data_adherence: {self.data_adherence}\n    planning_time: {self.planning_time}\n"
                f"    path_length_per_agent: {self.path_length_per_agent}\n"
                f"    mean_path_acceleration_per_agent: {self.mean_path_acceleration_per_agent}\n    num_ct_expansions: {self.num_ct_expansions}\n")


class MultiAgentPlanningExperimentConfig:
    def __init__(self):
        self.time_str = None
        self.instance_name = None
        self.num_agents_l: List[int] = []
        self.stagger_start_time_dt = 0
        self.multi_agent_planner_class_l: List[str] = []
        self.single_agent_planner_class = None
        self.runtime_limit = RUNTIME_LIMIT
        self.num_trials_per_combination = 1
        self.render_animation = False

    def get_single_trial_configs_from_experiment_config(self, seed=0):
        """experiments.py:68-98: per agent count the problems are drawn ONCE per trial number and shared by the planner classes; the
        configs come agent count -> planner class -> trial number.  Trial k of the j-th agent count draws its problem with seed
        `seed + j * num_trials_per_combination + k`."""
        configs = []
        for j, num_agents in enumerate(self.num_agents_l):
            problems = [get_planning_problem(self.instance_name, num_agents, seed=seed + j * self.num_trials_per_combination + k)
                        for k in range(self.num_trials_per_combination)]
            for planner_class in self.multi_agent_planner_class_l:
                for trial_number in range(self.num_trials_per_combination):
                    c = MultiAgentPlanningSingleTrialConfig()
                    c.time_str, c.trial_number, c.num_agents = self.time_str, trial_number, num_agents
                    c.stagger_start_time_dt = self.stagger_start_time_dt
                    c.multi_agent_planner_class, c.single_agent_planner_class = planner_class, self.single_agent_planner_class
                    c.instance_name, c.runtime_limit, c.render_animation = self.instance_name, self.runtime_limit, self.render_animation
                    c.start_state_pos_l, c.goal_state_pos_l, c.global_model_ids, c.agent_skeleton_l = problems[trial_number]
                    configs.append(c)
        return configs

    def to_dict(self):
        return {k: _plain(v) for k, v in vars(self).items()}

    def save(self, results_dir: str):
        os.makedirs(results_dir, exist_ok=True)
        with open(os.path.join(results_dir, "experiment_config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=1)


def get_result_dir_from_trial_config(trial_config, results_dir, trial_number=None):
    """experiments.py:259-274 below a caller-given root."""
    n = trial_config.trial_number if trial_number is None else trial_number
    return os.path.join(results_dir, f"instance_name___{trial_config.instance_name}", f"num_agents___{trial_config.num_agents}",
                        f"planner___{trial_config.multi_agent_planner_class}",
                        f"single_agent_planner___{trial_config.single_agent_planner_class}", str(n))


# ---- the statistics of a solution ------------------------------------------------------------------------------------------------------
class SolutionStats:
    """The host view of mmd_solution_stats' one buffer."""

    def __init__(self, words, n_agents, n_tiles):
        self.pair_collisions = int(words[:1].view(np.int32)[0])
        self.path_length = words[1:1 + n_agents]
        self.mean_accel = words[1 + n_agents:1 + 2 * n_agents]
        self.adherence = words[1 + 2 * n_agents:1 + 2 * n_agents + n_tiles]


def _to_host(stats_dev):
    """The ONE device -> host copy of a trial's statistics."""
    return stats_dev.cpu()


def tile_table(tiles):
    """The mmd_tile_ref table of (agent, t0, offset_x, offset_y, rule) tuples, on the host."""
    table = (_lib.TileRef * max(len(tiles), 1))()
    for k, (agent, t0, ox, oy, rule) in enumerate(tiles):
        table[k].agent, table[k].t0, table[k].rule = int(agent), int(t0), int(rule)
        table[k].offset[0], table[k].offset[1] = float(ox), float(oy)
    return table


def solution_stats_dev(paths, tiles, collision_dist=COLLISION_DIST):
    """mmd_solution_stats through ctypes: paths [n_agents, Tg, 4] contiguous float32 device tensor (the padded solution), tiles a sequence
    of (agent, t0, offset_x, offset_y, rule) -> the float32 device buffer [1 + 2 n + n_tiles] (word 0 holds an int32)."""
    _lib.require_gpu(paths, "paths")
    if paths.ndim != 3 or paths.shape[-1] != 4:
        raise ValueError("solution_stats: paths must be [n_agents, Tg, 4]")
    n, Tg, m = int(paths.shape[0]), int(paths.shape[1]), len(tiles)
    table = tile_table(tiles)
    table_dev = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(paths.device)
    stats = torch.empty(1 + 2 * n + m, dtype=torch.float32, device=paths.device)
    _lib.launch("mmd_solution_stats", paths, paths.data_ptr(), n, Tg, float(collision_dist), table, m, table_dev.data_ptr(), stats.data_ptr())
    return stats


def solution_stats(paths, tiles, collision_dist=COLLISION_DIST) -> SolutionStats:
    """The statistics of a solution: `paths` a list of [Tg, 4] tensors (CBS.plan's / PrioritizedPlanning.plan's first result) or one
    [n, Tg, 4] tensor; `tiles` (agent, t0, offset_x, offset_y, rule) per (agent, skeleton step), rule = ADHERENCE_RULE[env].  One launch
    sequence, one device -> host copy."""
    if not isinstance(paths, torch.Tensor):
        paths = torch.stack(list(paths))
    paths = paths.to(dtype=torch.float32).contiguous()
    if not paths.is_cuda:
        paths = paths.cuda()
    host = _to_host(solution_stats_dev(paths, tiles, collision_dist)).numpy()
    return SolutionStats(host, int(paths.shape[0]), len(tiles))


# ---- the trial (inference_multi_agent.py:81-366) ---------------------------------------------------------------------------------------
def _reference_task(model_ids, transforms, single_agent_planner_class, device):
    """The reference robot / task over ALL tiles (inference_multi_agent.py:140-188), built from the tile maps."""
    from .guides import GuideManagerTrajectoriesWithVelocity
    from .normalization import TrajectoryDatasetFacade
    from .planners import PlanningTaskEnsembleFacade, PlanningTaskFacade, RobotPlanarDiskFacade
    robot = RobotPlanarDiskFacade(device)
    ds = TrajectoryDatasetFacade(synth.NORM_MINS, synth.NORM_MAXS)
    if single_agent_planner_class == "MPD":
        guide = GuideManagerTrajectoriesWithVelocity(ds, env_id=model_ids[0].split("-")[0], n_support_points=HORIZON, device=device)
        return robot, PlanningTaskFacade(guide, robot)
    guides = {k: GuideManagerTrajectoriesWithVelocity(ds, env_id=m.split("-")[0], obstacle_cutoff_margin=0.01, n_support_points=HORIZON,
                                                      device=device) for k, m in enumerate(model_ids)}
    return robot, PlanningTaskEnsembleFacade(guides, dict(enumerate(transforms)), robot)


def build_trial(test_config, planner_kwargs=None, seed=0, device="cuda"):
    """The wiring of a trial (inference_multi_agent.py:85-254) -> (multi-agent planner, start_l, goal_l [global frame], start_time_l,
    agent_model_ids_l, agent_model_transforms_l)."""
    from .planners import MPD, MPDEnsemble
    c = test_config
    n = c.num_agents
    start_time_l = [i * c.stagger_start_time_dt for i in range(n)]
    if c.single_agent_planner_class not in ("MPD", "MPDEnsemble"):
        raise ValueError(f"Unknown single agent planner class: {c.single_agent_planner_class}")
    if c.multi_agent_planner_class not in ("XECBS", "ECBS", "XCBS", "CBS", "PP"):
        raise ValueError(f"Unknown multi agent planner class: {c.multi_agent_planner_class}")
    ids = c.global_model_ids
    transforms = [[torch.tensor([x * TILE_WIDTH, -y * TILE_HEIGHT], dtype=torch.float32) for x in range(len(ids[0]))] for y in range(len(ids))]
    for row in ids:
        for model_id in row:
            if model_id.split("-")[0] not in ADHERENCE_RULE:
                raise ValueError(f"no data-adherence rule for the environment of {model_id!r}")
    skel = c.agent_skeleton_l
    start_l = [torch.as_tensor(c.start_state_pos_l[i], dtype=torch.float32).cpu() + transforms[skel[i][0][0]][skel[i][0][1]] for i in range(n)]
    goal_l = [torch.as_tensor(c.goal_state_pos_l[i], dtype=torch.float32).cpu() + transforms[skel[i][-1][0]][skel[i][-1][1]] for i in range(n)]
    agent_model_ids_l = [[ids[r][col] for r, col in skel[i]] for i in range(n)]
    agent_model_transforms_l = [{k: transforms[r][col] for k, (r, col) in enumerate(skel[i])} for i in range(n)]
    kw = dict(planner_alg="mmd", device=device, trained_models_dir="")
    kw.update(planner_kwargs or {})
    planners = []
    for i in range(n):
        kwi = dict(kw, start_state_pos=start_l[i], goal_state_pos=goal_l[i], seed=int(seed) + i)
        if c.single_agent_planner_class == "MPD":
            kwi.pop("model_state_dicts", None)
            planners.append(MPD(model_id=agent_model_ids_l[i][0], **kwi))
        else:
            kwi.pop("model_state_dict", None)
            planners.append(MPDEnsemble(model_ids=tuple(agent_model_ids_l[i]), transforms=agent_model_transforms_l[i], **kwi))
    reference_ids = [ids[r][col] for r in range(len(ids)) for col in range(len(ids[0]))]
    reference_transforms = [transforms[r][col] for r in range(len(ids)) for col in range(len(ids[0]))]
    robot, task = _reference_task(reference_ids, reference_transforms, c.single_agent_planner_class, device)
    if c.multi_agent_planner_class == "PP":
        alg = PrioritizedPlanning(planners, start_l, goal_l, start_time_l=start_time_l, reference_robot=robot, reference_task=task)
    else:
        alg = CBS(planners, start_l, goal_l, start_time_l=start_time_l, is_xcbs=c.multi_agent_planner_class in ("XECBS", "XCBS"),
                  is_ecbs=c.multi_agent_planner_class in ("ECBS", "XECBS"), reference_robot=robot, reference_task=task)
    return alg, start_l, goal_l, start_time_l, agent_model_ids_l, agent_model_transforms_l


def trial_tiles(start_time_l, agent_model_ids_l, agent_model_transforms_l):
    """The tile references of a solution: one per (agent, skeleton step), t0 = start_time + step * 64 (inference_multi_agent.py:304-313)."""
    tiles = []
    for a, model_ids in enumerate(agent_model_ids_l):
        for k, model_id in enumerate(model_ids):
            env = model_id.split("-")[0]
            if env not in ADHERENCE_RULE:
                raise ValueError(f"no data-adherence rule for environment {env!r}")
            t = agent_model_transforms_l[a][k]
            tiles.append((a, start_time_l[a] + k * HORIZON, float(t[0]), float(t[1]), ADHERENCE_RULE[env]))
    return tiles


def run_multi_agent_trial(test_config, planner_kwargs=None, seed=0, results_dir=None, device="cuda"):
    """inference_multi_agent.py:81-350 -> MultiAgentPlanningSingleTrialResult.  planner_kwargs go to every low-level planner (e.g.
    model_state_dict(s), model_args, n_samples, trained_models_dir); results_dir: where results.txt / results.json / config.json go
    (below the reference's instance / agents / planner / trial directories), None = nothing is written."""
    from . import diffusion_model as dm
    alg, start_l, goal_l, start_time_l, agent_model_ids_l, agent_model_transforms_l = build_trial(test_config, planner_kwargs, seed, device)
    n = test_config.num_agents
    with dm._DRAW_LOCK:
        dm._GLOBAL_DRAWS = 0                       # (see "Seeds" above)
    startt = time.time()
    paths_l, num_ct_expansions, trial_success_status, num_collisions_in_solution = alg.plan(runtime_limit=test_config.runtime_limit)
    planning_time = time.time() - startt

    r = MultiAgentPlanningSingleTrialResult()
    r.trial_config = test_config
    r.start_state_pos_l = [s.cpu().numpy().tolist() for s in start_l]
    r.goal_state_pos_l = [g.cpu().numpy().tolist() for g in goal_l]
    r.global_model_ids, r.agent_skeleton_l = test_config.global_model_ids, test_config.agent_skeleton_l
    r.agent_path_l = paths_l
    r.success_status = trial_success_status
    r.num_collisions_in_solution = num_collisions_in_solution
    r.planning_time = planning_time
    r.search_status = trial_success_status         # what the search returned, before the collision rule below
    if len(paths_l) > 0 and trial_success_status:
        tiles = trial_tiles(start_time_l, agent_model_ids_l, agent_model_transforms_l)
        stats = solution_stats(paths_l, tiles)
        r.num_collisions_in_solution += stats.pair_collisions                 # inference_multi_agent.py:286-296
        if r.num_collisions_in_solution > 0:
            r.success_status = TrialSuccessStatus.FAIL_COLLISION_AGENTS
        # inference_multi_agent.py:299-342: the reference computes these whenever the SEARCH succeeded
        r.data_adherence = 0.0
        k = 0
        for agent_id in range(n):
            agent_data_adherence = 0.0
            for _ in agent_model_ids_l[agent_id]:
                agent_data_adherence += float(stats.adherence[k])
                k += 1
            agent_data_adherence /= len(agent_model_ids_l[agent_id])
            r.data_adherence += agent_data_adherence
        r.data_adherence /= n
        r.num_ct_expansions = num_ct_expansions
        r.path_length_per_agent = 0.0
        r.mean_path_acceleration_per_agent = 0.0
        for agent_id in range(n):
            r.path_length_per_agent += float(stats.path_length[agent_id])
            r.mean_path_acceleration_per_agent += float(stats.mean_accel[agent_id])
        r.path_length_per_agent /= n
        r.mean_path_acceleration_per_agent /= n
    if results_dir is not None:
        d = get_result_dir_from_trial_config(test_config, results_dir)
        r.save(d)
        test_config.save(d)
    return r


# ---- experiments (experiment_utils.py:84-196) ------------------------------------------------------------------------------------------
AGGREGATE_COLUMNS = ("avg_data_adherence", "avg_planning_time", "avg_path_length_per_agent", "avg_mean_path_acceleration_per_agent",
                     "success_rate", "fail_rate_runtime_limit", "fail_rate_no_solution", "fail_rate_collision_agents",
                     "avg_num_collisions_in_solution", "avg_ct_expansions")


def aggregate_results(results):
    """experiment_utils.py:100-164: rows (method, num_agents, num_trials, AGGREGATE_COLUMNS...) per agent count x planner class, in order
    of first appearance; rates over all trials, the averages over successful trials (avg_num_collisions_in_solution: the sum over
    successful trials divided by all trials, as the reference does)."""
    groups = {}
    for r in results:
        groups.setdefault((r.trial_config.num_agents, r.trial_config.multi_agent_planner_class), []).append(r)
    rows = []
    for (num_agents, method), rs in groups.items():
        ok = [r for r in rs if r.success_status == TrialSuccessStatus.SUCCESS]
        row = dict.fromkeys(AGGREGATE_COLUMNS, 0.0)
        for name, status in (("success_rate", TrialSuccessStatus.SUCCESS), ("fail_rate_runtime_limit", TrialSuccessStatus.FAIL_RUNTIME_LIMIT),
                             ("fail_rate_no_solution", TrialSuccessStatus.FAIL_NO_SOLUTION),
                             ("fail_rate_collision_agents", TrialSuccessStatus.FAIL_COLLISION_AGENTS)):
            row[name] = sum(r.success_status == status for r in rs) / len(rs)
        if ok:
            for name, attr in (("avg_ct_expansions", "num_ct_expansions"), ("avg_data_adherence", "data_adherence"),
                               ("avg_planning_time", "planning_time"), ("avg_path_length_per_agent", "path_length_per_agent"),
                               ("avg_mean_path_acceleration_per_agent", "mean_path_acceleration_per_agent")):
                row[name] = sum(getattr(r, attr) for r in ok) / len(ok)
            row["avg_num_collisions_in_solution"] = sum(r.num_collisions_in_solution for r in ok) / len(rs)
        rows.append(dict(method=method, num_agents=num_agents, num_trials=len(rs), **row))
    return rows


def combine_and_save_results_for_experiment(results, results_dir):
    """One CSV, aggregated_results_all_agents.csv, written with the standard library."""
    os.makedirs(results_dir, exist_ok=True)
    path = os.path.join(results_dir, "aggregated_results_all_agents.csv")
    rows = aggregate_results(results)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=("method", "num_agents", "num_trials") + AGGREGATE_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return path


def run_experiment(experiment_config, planner_kwargs=None, seed=0, results_dir=None, device="cuda"):
    """The trials of get_single_trial_configs_from_experiment_config() one after the other (trial i runs with seed `seed + i`) and, with a
    results_dir, the per-trial files and the aggregated CSV -> (results, aggregated rows)."""
    results = []
    for i, c in enumerate(experiment_config.get_single_trial_configs_from_experiment_config(seed=seed)):
        results.append(run_multi_agent_trial(c, planner_kwargs, seed=seed + i, results_dir=results_dir, device=device))
    if results_dir is not None:
        experiment_config.save(results_dir)
        combine_and_save_results_for_experiment(results, results_dir)
    return results, aggregate_results(results)
