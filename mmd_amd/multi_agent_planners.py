"""The multi-agent planners over MPD / MPDEnsemble: Conflict-Based Search and its variants (ECBS, XCBS, XECBS) and Prioritized Planning.

Mirrors reference mmd/planners/multi_agent/{cbs.py, prioritized_planning.py}, mmd/common/{conflicts.py, conflict_conversion.py,
multi_agent_utils.py:120-143} and mmd/common/experiments/experiments.py:168-176: same class, method and keyword names, the same
search.  The search layer runs on the device (mmd_amd/csrc/multi_agent.hip):
  * get_conflicts: ONE launch sequence over the chosen paths with their own lengths and start times (mmd_find_conflicts); the host
    reads back the count and the first conflict -- all the search reads (the sort key len(conflict_l), expand's conflict_l[0]);
    the rest of the list is fetched only if a caller indexes past the first entry;
  * the 'least_collisions' choice among the free samples of a re-planned agent (cbs.py:446-458, prioritized_planning.py:172-182):
    one launch sequence for every candidate (mmd_scan_candidates) instead of one get_conflicts per candidate;
  * the soft (ECBS) / hard (PP) constraints from the other agents' paths: for an MPD built on the device (PathConstraints ->
    mmd_path_constraints), for any other low-level planner handed over in the reference's MultiPointConstraint form.
CBS re-plans the two children of an expansion as ONE launch sequence (planners.plan_batched) when its low-level planners are MPD /
MPDEnsemble; their seeds are drawn in child order before planning, so `batch_expansions=False` gives bitwise the same tree.

Deviations from the reference, all documented at the place they occur:
  * PrioritizedPlanning(start_time_l=None) means all zeros (the reference never sets self.start_time_l then and fails,
    prioritized_planning.py:66-69);
  * CBS(conflict_type_to_constraint_types=None) means {PointConflict: {MultiPointConstraint}} (what the reference's script passes;
    the reference fails on None, cbs.py:183);
  * conflict settings other than {PointConflict: {MultiPointConstraint}} (CBS) raise NotImplementedError: in the reference an
    EdgeConstraint or VertexConstraint cannot reach MPD;
  * the search prints nothing; render_paths, visualisation and the experiment launcher are not part of this package.
"""
import time
from enum import Enum
from typing import Dict, List, Type

import numpy as np
import torch

from . import multi_agent as ma
from .constraints import MultiPointConstraint, VERTEX_CONSTRAINT_RADIUS

__all__ = ["CBS", "PrioritizedPlanning", "SearchState", "TrialSuccessStatus", "PointConflict", "VertexConflict", "EdgeConflict",
           "Conflict", "ConflictList", "convert_conflicts_to_constraints", "global_pad_paths", "is_multi_agent_start_goal_states_valid"]

LOW_LEVEL_CHOOSE_PATH_FROM_BATCH_STRATEGY = "least_collisions"      # mmd_params.py:53
HORIZON = 64                                                        # mmd_params.py:34 (PP's clamp, prioritized_planning.py:155-158)


class TrialSuccessStatus(Enum):
    """experiments.py:168-176."""
    UNKNOWN = -1
    SUCCESS = 0
    FAIL_RUNTIME_LIMIT = 1
    FAIL_COLLISION_AGENTS = 2
    FAIL_NO_SOLUTION = 3

    def __bool__(self):
        return self == TrialSuccessStatus.SUCCESS


# ---- conflicts (mmd/common/conflicts.py) --------------------------------------------------------------------------------------------
class Conflict:
    def __init__(self):
        self.time_interval = None

    def get_t_range(self):
        raise NotImplementedError


class VertexConflict(Conflict):
    def __init__(self, agent_ids: List, q_l: List, t: int):
        super().__init__()
        self.agent_ids = agent_ids
        self.q_map = {agent_id: q for agent_id, q in zip(agent_ids, q_l)}
        self.t = t

    def get_t_range(self):
        return self.t, self.t


class EdgeConflict(Conflict):
    def __init__(self, agent_ids: List, q_from_l: List, q_to_l: List, t_from: int, t_to: int):
        super().__init__()
        self.agent_ids = agent_ids
        self.agent_id_to_q_from = {agent_id: q for agent_id, q in zip(agent_ids, q_from_l)}
        self.agent_id_to_q_to = {agent_id: q for agent_id, q in zip(agent_ids, q_to_l)}
        self.t_from, self.t_to = t_from, t_to

    def get_t_range(self):
        return self.t_from, self.t_to


class PointConflict(Conflict):
    def __init__(self, agent_ids: List, q_l: List, p_l: List, t_from: int, t_to: int):
        super().__init__()
        self.agent_ids = agent_ids
        self.agent_id_to_p = {agent_id: p for agent_id, p in zip(agent_ids, p_l)}
        self.agent_id_to_q = {agent_id: q for agent_id, q in zip(agent_ids, q_l)}
        self.t_from, self.t_to = t_from, t_to

    def get_t_range(self):
        return self.t_from, self.t_to


def _make_conflict(kind, t, a, b, pa, pb, mid):
    pa, pb, mid = (torch.from_numpy(np.array(v, dtype=np.float32)) for v in (pa, pb, mid))
    if kind == "point":          # cbs.py:232-244: p_l = both positions, q_l = the midpoint twice, t_from = t_to = t
        return PointConflict([int(a), int(b)], q_l=[mid, mid.clone()], p_l=[pa, pb], t_from=int(t), t_to=int(t))
    return VertexConflict([int(a), int(b)], [pa, pb], int(t))          # prioritized_planning.py:287-295


class ConflictList:
    """The conflict list of a search state as the device found it: len() and [0] from the one summary the host read back; the whole list
    (iteration, any other index) fetched from the device on first use."""

    def __init__(self, count, first, kind, fetch):
        self._count, self._first, self._kind, self._fetch, self._all = int(count), first, kind, fetch, None

    def __len__(self):
        return self._count

    def __bool__(self):
        return self._count > 0

    def _full(self):
        if self._all is None:
            self._all = self._fetch() if self._count else []
        return self._all

    def __getitem__(self, i):
        if isinstance(i, int) and (i == 0 or i == -self._count) and self._first is not None:
            return _make_conflict(self._kind, *self._first)
        return self._full()[i]

    def __iter__(self):
        return iter(self._full())


# ---- conflicts -> constraints (mmd/common/conflict_conversion.py:32-82) -------------------------------------------------------------
def convert_conflicts_to_constraints(conflict: Conflict, conflict_type_to_constraint_types: Dict[Type[Conflict], Type], t_pad: int = 2):
    """PointConflict -> one MultiPointConstraint per agent at the midpoint, range (t_from - t_pad, t_to + t_pad).  The other conflict types
    become EdgeConstraint / VertexConstraint in the reference, which MPD cannot take: NotImplementedError."""
    constraints = []
    if isinstance(conflict, PointConflict):
        if MultiPointConstraint in conflict_type_to_constraint_types[PointConflict]:
            for agent_id in conflict.agent_ids:
                constraints.append((agent_id, MultiPointConstraint(q_l=[conflict.agent_id_to_q[agent_id]],
                                                                   t_range_l=[(conflict.t_from - t_pad, conflict.t_to + t_pad)],
                                                                   radius_l=[VERTEX_CONSTRAINT_RADIUS])))
        else:
            raise NotImplementedError()
    elif isinstance(conflict, (EdgeConflict, VertexConflict)):
        raise NotImplementedError(f"{type(conflict).__name__}: its constraint type cannot reach MPD")
    return constraints


def shift_and_clamp_t_ranges(t_range_l, start_time, path_length):
    """cbs.py:395-406: the range moved to the agent's local time, then clamped to [0, L - 1]."""
    shifted = [(t0 - start_time, t1 - start_time) for t0, t1 in t_range_l]
    return [(max(0, min(t0, path_length - 1)), min(path_length - 1, t1)) for t0, t1 in shifted]


def global_pad_paths(path_l: List[torch.Tensor], start_time_l: List[int]) -> List[torch.Tensor]:
    """multi_agent_utils.py:120-143: every path repeated at its start before s_k and at its end after s_k + L_k - 1, to a common length."""
    path_l = [p.clone() for p in path_l]
    if len(path_l) == 0:
        return path_l
    max_t = max(len(path) + start_time_l[k] for k, path in enumerate(path_l))
    for k, path in enumerate(path_l):
        if len(path) + start_time_l[k] < max_t:
            path = torch.cat([path, path[-1].repeat(max_t - len(path) - start_time_l[k], 1)])
        if start_time_l[k] > 0:
            path = torch.cat([path[0].repeat(start_time_l[k], 1), path])
        path_l[k] = path
    return path_l


def is_multi_agent_start_goal_states_valid(reference_robot, reference_task, start_state_pos_l, goal_state_pos_l,
                                           is_enforce_min_dist=True) -> bool:
    """multi_agent_utils.py:54-98."""
    if is_enforce_min_dist:
        for i in range(len(start_state_pos_l)):
            for j in range(i + 1, len(goal_state_pos_l)):
                if torch.norm(start_state_pos_l[i] - start_state_pos_l[j]) < 0.15:
                    return False
                if torch.norm(goal_state_pos_l[i] - goal_state_pos_l[j]) < 0.15:
                    return False
    for states in (start_state_pos_l, goal_state_pos_l):
        coll, _ = reference_robot.check_rr_collisions(torch.stack(list(states)))
        if torch.any(coll):
            return False
    for states in (start_state_pos_l, goal_state_pos_l):
        if torch.any(reference_task.compute_collision(torch.stack(list(states)))):
            return False
    return True


# ---- the constraint-tree node (cbs.py:67-108) ----------------------------------------------------------------------------------------
class SearchState:
    def __init__(self, ix_best_path_in_batch_l, path_bl, constraints=None):
        self.path_bl = path_bl                                    # n_agents x [B, L, q_dim]
        self.ix_best_path_in_batch_l = ix_best_path_in_batch_l
        self.conflict_l = []
        self.constraints = {} if constraints is None else constraints
        self._g, self._g_src = float("inf"), None

    @property
    def g(self):
        """The cost of update_g_l2, evaluated from the paths and choices of the time of that call (on first read)."""
        if self._g_src is not None:
            paths, ixs = self._g_src
            g = 0
            for path_b, ix in zip(paths, ixs):
                path = path_b[ix]
                g += torch.norm(path[1:] - path[:-1], dim=-1).sum()
            self._g, self._g_src = g, None
        return self._g

    @g.setter
    def g(self, value):
        self._g, self._g_src = value, None

    def update_g_l2(self):
        """Sum over agents of the L2 step lengths of the chosen path, over the full state (cbs.py:79-87)."""
        self._g_src = (list(self.path_bl), list(self.ix_best_path_in_batch_l))

    def add_constraint(self, agent_id, constraint):
        self.constraints.setdefault(agent_id, []).append(constraint)

    def get_copy(self, share_paths=False):
        """cbs.py:97-108.  share_paths=True (the search's own copies): the batches are shared, not cloned -- the search only ever
        replaces an agent's batch, it never writes into one."""
        new_path_bl = list(self.path_bl) if share_paths else [path_b.clone() for path_b in self.path_bl]
        new_constraints = {k: [c.get_copy() for c in v] for k, v in self.constraints.items()}
        new_state = SearchState(list(self.ix_best_path_in_batch_l), new_path_bl, new_constraints)
        new_state.conflict_l = self.conflict_l
        new_state._g, new_state._g_src = self._g, self._g_src
        return new_state


# ---- shared by both searches ---------------------------------------------------------------------------------------------------------
def _is_device_planner(planner):
    from .planners import MPD, MPDEnsemble
    return isinstance(planner, (MPD, MPDEnsemble))


def _is_mpd(planner):
    from .planners import MPD
    return isinstance(planner, MPD)


class _SearchBase:
    mode = ma.ORDERED
    kind = "point"

    def _init_common(self, low_level_planner_l, start_l, goal_l, start_time_l, reference_robot, reference_task):
        self.low_level_choose_path_from_batch_strategy = LOW_LEVEL_CHOOSE_PATH_FROM_BATCH_STRATEGY
        self.low_level_planner_l = low_level_planner_l
        self.num_agents = len(start_l)
        self.start_state_pos_l = start_l
        self.goal_state_pos_l = goal_l
        self.start_time_l = [0] * self.num_agents if start_time_l is None else [int(s) for s in start_time_l]
        self.reference_robot = low_level_planner_l[0].robot if reference_robot is None else reference_robot
        self.reference_task = low_level_planner_l[0].task if reference_task is None else reference_task
        self.tensor_args = getattr(low_level_planner_l[0], "tensor_args", None)
        self.results_dir = getattr(low_level_planner_l[0], "results_dir", None)
        self.margin = 2.1 * float(getattr(self.reference_robot, "radius", ma.ROBOT_RADIUS))        # robot_planar_disk.py:186
        # (agent, chosen sample, conflict count) of every low-level choice, in order
        self.node_log = []
        self.timing = {"low_level": 0.0, "search": 0.0}
        if not is_multi_agent_start_goal_states_valid(self.reference_robot, self.reference_task, self.start_state_pos_l,
                                                      self.goal_state_pos_l):
            raise ValueError("Start or goal states are invalid.")

    # the device view of a state
    def _state_view(self, state):
        batches = [p if p.is_contiguous() else p.contiguous() for p in state.path_bl]
        starts = self.start_time_l[:len(batches)]
        Tg = ma.global_horizon([b.shape[1] for b in batches], starts)
        return batches, starts, Tg

    def get_conflicts(self, state: SearchState):
        """CBS.get_conflicts (cbs.py:166-246) / PrioritizedPlanning.get_conflicts (prioritized_planning.py:249-298) on the device."""
        n = len(state.path_bl)
        if n == 0:
            return []
        batches, starts, Tg = self._state_view(state)
        table = ma.agent_table(batches, state.ix_best_path_in_batch_l, starts)
        summ, _ = ma.find_conflicts(table, n, Tg, self.mode, margin=self.margin)
        count, first = ma.read_summary(summ)
        mode, kind, margin, state_ix = self.mode, self.kind, self.margin, list(state.ix_best_path_in_batch_l)

        def fetch():                                                      # (the closure keeps `batches`, which the table points into, alive)
            _, lst = ma.find_conflicts(ma.agent_table(batches, state_ix, starts), n, Tg, mode, list_cap=count, margin=margin)
            t, a, b, pa, pb, mid = ma.decode_records(lst.cpu().numpy())
            return [_make_conflict(kind, t[k], a[k], b[k], pa[k], pb[k], mid[k]) for k in range(count)]
        return ConflictList(count, first, kind, fetch)

    def _scan(self, state, agent, planner_output, rule, init_idx=None):
        """The 'least_collisions' choice for `agent` among planner_output's free samples -> (sample index, conflict count)."""
        batches, starts, Tg = self._state_view(state)
        table = ma.agent_table(batches, state.ix_best_path_in_batch_l, starts)
        res = ma.scan_candidates(table, len(batches), Tg, agent, batches[agent], planner_output.trajs_final_free_idxs, self.mode, rule,
                                 init_idx=init_idx, margin=self.margin)
        ix, count = (int(v) for v in res.cpu().numpy())
        return ix, count

    def _path_constraints(self, state, agent_id, is_soft):
        return ma.PathConstraints(state.path_bl, state.ix_best_path_in_batch_l, agent_id, self.start_time_l,
                                  n_state=len(state.path_bl), is_soft=is_soft)

    def create_soft_constraints_from_other_agents_paths(self, state: SearchState, agent_id: int) -> List[MultiPointConstraint]:
        """cbs.py:468-508 / prioritized_planning.py:212-247 in the reference's list form."""
        if len(state.path_bl) == 0:
            return []
        return self._path_constraints(state, agent_id, True).constraint_list()

    @staticmethod
    def _n_free(planner_output):
        return int(planner_output.trajs_final_free_idxs.shape[0]) if planner_output.trajs_final_free_idxs is not None else 0

    def _final_paths(self, state):
        best_path_l = [state.path_bl[i][ix].squeeze(0) for i, ix in enumerate(state.ix_best_path_in_batch_l)]
        return global_pad_paths(best_path_l, self.start_time_l)


def _call_planner(planner, start, goal, constraints_l, experience=None, path_constraints=None, seed=None):
    kw = {}
    if path_constraints is not None:
        kw["path_constraints"] = path_constraints
    if seed is not None:
        kw["seed"] = seed
    return planner(start, goal, constraints_l=constraints_l, experience=experience, **kw)


# ---- CBS (cbs.py:111-508) -----------------------------------------------------------------------------------------------------------
class CBS(_SearchBase):
    """Conflict-Based Search over the low-level planners (one per agent).  is_ecbs: soft constraints from the other agents' paths;
    is_xcbs: re-plans start from the agent's previous batch (PathBatchExperience).  batch_expansions: the two children of an expansion
    re-planned as one launch sequence (MPD / MPDEnsemble planners; bitwise the tree of one call after the other)."""

    mode = ma.ORDERED
    kind = "point"

    def __init__(self, low_level_planner_l, start_l: List[torch.Tensor], goal_l: List[torch.Tensor], start_time_l: List[int] = None,
                 is_xcbs=False, is_ecbs=True, conflict_type_to_constraint_types: Dict[Type[Conflict], Type] = None,
                 reference_robot=None, reference_task=None, batch_expansions=True, **kwargs):
        if conflict_type_to_constraint_types is None:
            conflict_type_to_constraint_types = {PointConflict: {MultiPointConstraint}}
        if set(conflict_type_to_constraint_types) != {PointConflict} or \
                MultiPointConstraint not in conflict_type_to_constraint_types[PointConflict]:
            raise NotImplementedError("CBS: only {PointConflict: {MultiPointConstraint}} reaches MPD (edge / vertex constraints do not)")
        self.is_xcbs = is_xcbs
        self.is_ecbs = is_ecbs
        self.conflict_type_to_constraint_types = conflict_type_to_constraint_types
        self.batch_expansions = batch_expansions
        self._init_common(low_level_planner_l, start_l, goal_l, start_time_l, reference_robot, reference_task)
        self.open_l = []

    def _soft_args(self, state, agent_id, constraint_l):
        """(constraints_l, path_constraints) of a call: ECBS soft constraints built on the device for an MPD, in list form otherwise."""
        if not self.is_ecbs or len(state.path_bl) == 0:
            return constraint_l, None
        pc = self._path_constraints(state, agent_id, True)
        if _is_mpd(self.low_level_planner_l[agent_id]):
            return constraint_l, pc
        return constraint_l + pc.constraint_list(), None

    def _choose(self, state, agent_id, planner_output):
        if self.low_level_choose_path_from_batch_strategy == "least_cost":
            state.ix_best_path_in_batch_l[agent_id] = int(planner_output.idx_best_traj)
            state.conflict_l = self.get_conflicts(state)
        elif self.low_level_choose_path_from_batch_strategy == "least_collisions":
            ix, count = self._scan(state, agent_id, planner_output, ma.SELECT_CBS)
            state.ix_best_path_in_batch_l[agent_id] = ix
            state.conflict_l = self.get_conflicts(state)
            assert len(state.conflict_l) == count
        else:
            raise ValueError("Invalid low level choose-path-from-batch strategy.")
        self.node_log.append((agent_id, state.ix_best_path_in_batch_l[agent_id], len(state.conflict_l)))

    def plan(self, runtime_limit=1000):
        startt = time.time()
        success_status = TrialSuccessStatus.UNKNOWN
        root = SearchState([], [])
        state = root
        for i in range(len(self.low_level_planner_l)):
            constraint_l, pc = self._soft_args(root, i, [])
            t0 = time.time()
            planner_output = _call_planner(self.low_level_planner_l[i], self.start_state_pos_l[i], self.goal_state_pos_l[i], constraint_l,
                                           path_constraints=pc)
            self.timing["low_level"] += time.time() - t0
            if self._n_free(planner_output) == 0:
                success_status = TrialSuccessStatus.FAIL_NO_SOLUTION
                state = root
                break
            root.path_bl.append(planner_output.trajs_final)
            root.ix_best_path_in_batch_l.append(int(planner_output.idx_best_traj))
            if time.time() - startt > runtime_limit:
                success_status = TrialSuccessStatus.FAIL_RUNTIME_LIMIT
                state = root
                break
        if success_status == TrialSuccessStatus.UNKNOWN:
            root.update_g_l2()
            root.conflict_l = self.get_conflicts(root)
            self.open_l.append(root)

        num_ct_expansions = 0
        while success_status == TrialSuccessStatus.UNKNOWN:
            if not self.open_l:
                success_status = TrialSuccessStatus.FAIL_NO_SOLUTION
                break
            self.open_l.sort(key=lambda x: len(x.conflict_l))          # stable (cbs.py:365-367)
            state = self.open_l.pop(0)
            if not state.conflict_l:
                success_status = TrialSuccessStatus.SUCCESS
                break
            self.expand(state)
            num_ct_expansions += 1
            if time.time() - startt > runtime_limit:
                success_status = TrialSuccessStatus.FAIL_RUNTIME_LIMIT
                break
        self.timing["search"] = time.time() - startt - self.timing["low_level"]
        return self._final_paths(state), num_ct_expansions, success_status, len(state.conflict_l)

    def expand(self, state: SearchState):
        """cbs.py:382-466: branch on conflict_l[0]; one child per (agent, constraint)."""
        from .planners import PathBatchExperience
        conflict = state.conflict_l[0]
        constraints = convert_conflicts_to_constraints(conflict, self.conflict_type_to_constraint_types)
        children = []
        for agent_id, constraint in constraints:
            constraint.t_range_l = shift_and_clamp_t_ranges(constraint.t_range_l, self.start_time_l[agent_id],
                                                            len(state.path_bl[agent_id][0]))
            new_state = state.get_copy(share_paths=True)
            new_state.add_constraint(agent_id, constraint)
            constraint_l, pc = self._soft_args(new_state, agent_id, new_state.constraints[agent_id].copy())
            experience = PathBatchExperience(new_state.path_bl[agent_id]) if self.is_xcbs else None
            children.append((agent_id, new_state, constraint_l, experience, pc))
        planners = [self.low_level_planner_l[a] for a, *_ in children]
        device = all(_is_device_planner(p) for p in planners)
        seeds = None
        if device:                                   # drawn in child order BEFORE planning, in both modes
            from .planners import _default_seeds
            seeds = _default_seeds([(p,) for p in planners])
        t0 = time.time()
        if device and self.batch_expansions and len(children) > 1:
            from .planners import plan_batched
            calls = [(planners[k], self.start_state_pos_l[a], self.goal_state_pos_l[a], cl, exp, pc)
                     for k, (a, _, cl, exp, pc) in enumerate(children)]
            from . import diffusion_model as dm
            with dm._DRAW_LOCK:
                mark = dm._GLOBAL_DRAWS
            outputs = plan_batched(calls, seeds=seeds)
            # a packed group draws one base stream seed that its per-call seeds override: put the global stream back where one call
            # after the other leaves it, so that both modes draw the same seeds for the rest of the search
            with dm._DRAW_LOCK:
                dm._GLOBAL_DRAWS = mark
        else:
            outputs = None
        self.timing["low_level"] += time.time() - t0
        for k, (agent_id, new_state, constraint_l, experience, pc) in enumerate(children):
            if outputs is not None:
                planner_output = outputs[k]
            else:
                t0 = time.time()
                planner_output = _call_planner(planners[k], self.start_state_pos_l[agent_id], self.goal_state_pos_l[agent_id], constraint_l,
                                               experience, pc, seed=None if seeds is None else int(seeds[k]))
                self.timing["low_level"] += time.time() - t0
            if self._n_free(planner_output) == 0:
                return                                  # cbs.py:434-436: the other child is not kept
            new_state.path_bl[agent_id] = planner_output.trajs_final
            self._choose(new_state, agent_id, planner_output)
            new_state.update_g_l2()
            self.open_l.append(new_state)


# ---- Prioritized Planning (prioritized_planning.py:46-298) ---------------------------------------------------------------------------
class PrioritizedPlanning(_SearchBase):
    """Agents planned one after the other; agent i takes the paths of agents 0 .. i-1 as hard constraints."""

    mode = ma.PAIRS
    kind = "vertex"

    def __init__(self, low_level_planner_l, start_l: List[torch.Tensor], goal_l: List[torch.Tensor], start_time_l: List[int] = None,
                 reference_robot=None, reference_task=None, **kwargs):
        # start_time_l=None: all zeros (the reference leaves self.start_time_l unset then and fails, prioritized_planning.py:66-69)
        self._init_common(low_level_planner_l, start_l, goal_l, start_time_l, reference_robot, reference_task)

    def plan(self, runtime_limit=1000):
        startt = time.time()
        success_status = TrialSuccessStatus.UNKNOWN
        root = SearchState([], [])
        for i in range(len(self.low_level_planner_l)):
            planner = self.low_level_planner_l[i]
            pc = self._path_constraints(root, i, False) if len(root.path_bl) else None
            if pc is not None and not _is_mpd(planner):
                constraint_l, pc = pc.constraint_list(), None
            else:
                constraint_l = []
            t0 = time.time()
            planner_output = _call_planner(planner, self.start_state_pos_l[i], self.goal_state_pos_l[i], constraint_l, path_constraints=pc)
            self.timing["low_level"] += time.time() - t0
            if self._n_free(planner_output) == 0:
                success_status = TrialSuccessStatus.FAIL_NO_SOLUTION
                break
            ix_best_traj = int(planner_output.idx_best_traj)
            root.path_bl.append(planner_output.trajs_final)
            root.ix_best_path_in_batch_l.append(ix_best_traj)
            ix, count = self._scan(root, i, planner_output, ma.SELECT_PP, init_idx=ix_best_traj)
            root.ix_best_path_in_batch_l[i] = ix
            self.node_log.append((i, ix, count))
            if time.time() - startt > runtime_limit:
                success_status = TrialSuccessStatus.FAIL_RUNTIME_LIMIT
                break
        conflict_l = self.get_conflicts(root)
        root.conflict_l = conflict_l
        if success_status == TrialSuccessStatus.UNKNOWN:
            success_status = TrialSuccessStatus.FAIL_COLLISION_AGENTS if len(conflict_l) > 0 else TrialSuccessStatus.SUCCESS
        self.timing["search"] = time.time() - startt - self.timing["low_level"]
        return self._final_paths(root), 0, success_status, len(conflict_l)

    def create_soft_constraints_from_other_agents_paths(self, state: SearchState, agent_id: int) -> List[MultiPointConstraint]:
        return super().create_soft_constraints_from_other_agents_paths(state, agent_id)
