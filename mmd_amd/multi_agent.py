"""Device-side multi-agent helpers next to the sampler: robot-robot collisions of the best paths
(RobotPlanarDisk.check_rr_collisions as CBS.get_conflicts uses it, cbs.py:166-246) and the 'least_collisions' batch scan
(cbs.py:446-458), both also on a cell table of the best paths (count_collisions_binned, path_conflicts: O(N) work per round instead of
O(N^2)).  Thin wrappers over the C ABI (mmd_rr_collisions, mmd_count_collisions, mmd_count_collisions_binned, mmd_path_conflicts_binned), and the
choice of the robots a round re-plans from that report (select_replan: mmd_round_select)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

H = 64
ROBOT_RADIUS = 0.05
RR_MARGIN = 2.1 * ROBOT_RADIUS           # robot_planar_disk.py:186


def check_rr_collisions(paths, margin=RR_MARGIN, with_midpoints=True):
    """paths [N,T,2] un-normalised positions on the GPU -> (collisions [T,N,N] bool, midpoints [T,N,N,2] | None)."""
    n, T = paths.shape[0], paths.shape[1]
    mask = torch.empty((T, n, n), dtype=torch.uint8, device=paths.device)
    mid = torch.empty((T, n, n, 2), dtype=torch.float32, device=paths.device) if with_midpoints else None
    _lib.launch("mmd_rr_collisions", paths, _lib.require_gpu(paths.contiguous(), "paths"), n, T, float(margin),
                                             mask.data_ptr(), mid.data_ptr() if mid is not None else None)
    return mask.bool(), mid


def _count_launch(name, trajs, n_local, before, after):
    """An entry point (trajs, *before, n_local, B, *after, counts) on trajs [n_local * B, H, 4] -> its counts, int32 [n_local, B]."""
    B = trajs.shape[0] // n_local
    counts = torch.empty(n_local * B, dtype=torch.int32, device=trajs.device)
    _lib.launch(name, trajs, _lib.require_gpu(trajs.contiguous(), "trajs"), *before, n_local, B, *after, counts.data_ptr())
    return counts.view(n_local, B)


def count_collisions(trajs, paths_all, robot0, n_local, margin=RR_MARGIN):
    """trajs [n_local*B,H,4] un-normalised sample batches of the local robots, paths_all [N,H,2] best paths of all
    robots -> int32 [n_local, B] number of (t, other robot) collision pairs per sample."""
    return _count_launch("mmd_count_collisions", trajs, n_local, (_lib.require_gpu(paths_all.contiguous(), "paths_all"), robot0),
                         (paths_all.shape[0], H, float(margin)))


def _collision_table(table, what):
    if getattr(table, "first_step", None) != 0:
        raise ValueError(f"{what}: a collision table lists time step 0 (constraints.binned_collision_table), this one starts at "
                         f"{getattr(table, 'first_step', None)}")
    return table


def count_collisions_binned(trajs, table, n_local, margin=RR_MARGIN):
    """count_collisions on a cell table of the best paths (constraints.binned_collision_table(paths_all, robot0, n_local)) instead of
    the paths: a sample point meets only the robots near its cell.  -> int32 [n_local, B], the same integers."""
    _collision_table(table, "count_collisions_binned")
    return _count_launch("mmd_count_collisions_binned", trajs, n_local, (C.byref(table.struct),), (float(margin),))


def least_collision_samples(trajs, paths_all, robot0, n_local):
    """Index of the first sample with the fewest collisions per local robot (strict '<' scan of cbs.py:452)."""
    return torch.argmin(count_collisions(trajs, paths_all, robot0, n_local), dim=1)


# ---- the search layer of CBS / PrioritizedPlanning (mmd_find_conflicts, mmd_scan_candidates, mmd_path_constraints) ---------------
ORDERED, PAIRS = _lib.CONFLICTS_ORDERED, _lib.CONFLICTS_PAIRS        # CBS PointConflict order / PrioritizedPlanning VertexConflict order
SELECT_CBS, SELECT_PP = _lib.SELECT_CBS, _lib.SELECT_PP
VERTEX_CONSTRAINT_RADIUS = 0.05 * 2.4                                  # mmd_params.py:52
_CONFLICT_WORDS = 12                                                   # sizeof(mmd_conflict) / 4


def global_horizon(lengths, starts):
    """Tg = max_k (L_k + s_k): the length of global_pad_paths' output (multi_agent_utils.py:120-143)."""
    return max(int(L) + int(s) for L, s in zip(lengths, starts))


def agent_table(batches, indices, starts, device=None):
    """The mmd_agent_path table of a search state, on the device: agent k = sample indices[k] of batches[k] [B_k, L_k, 4] (contiguous
    float32 device tensors, kept alive by the caller), starting at global time starts[k].  One host -> device copy."""
    n = len(batches)
    arr = (_lib.AgentPath * max(n, 1))()
    for k, (b, i, s) in enumerate(zip(batches, indices, starts)):
        _lib.require_gpu(b, f"batches[{k}]")
        arr[k].batch_dev, arr[k].index, arr[k].length, arr[k].start_time = b.data_ptr(), int(i), int(b.shape[1]), int(s)
    dev = device if device is not None else (batches[0].device if n else torch.device("cuda"))
    return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(dev)


def _new_report(device, list_cap):
    """A report for an entry point to fill: (summary int32 [16], list [list_cap, 12] words or None, the entry point's four arguments
    for them: count, first record, list, list_cap)."""
    summ = torch.empty(16, dtype=torch.int32, device=device)
    lst = torch.empty((list_cap, _CONFLICT_WORDS), dtype=torch.int32, device=device) if list_cap > 0 else None
    return summ, lst, (summ.data_ptr(), summ.data_ptr() + 16, lst.data_ptr() if lst is not None else None, int(list_cap))


def find_conflicts(table, n, Tg, mode, list_cap=0, margin=RR_MARGIN):
    """mmd_find_conflicts -> (summary int32 [1 + 3 + 12] on the device: [0] = count, [4:16] = the first mmd_conflict record,
    list [list_cap, 12] words or None).  Read the summary with `read_summary` (one device -> host copy)."""
    summ, lst, report_args = _new_report(table.device, list_cap)
    rows = torch.empty(max(int(Tg), 1), dtype=torch.int32, device=table.device)
    _lib.launch("mmd_find_conflicts", table, table.data_ptr(), int(n), int(Tg), float(margin), int(mode), rows.data_ptr(), *report_args)
    return summ, lst


def path_conflicts(paths_all, margin=RR_MARGIN, list_cap=0, table=None, row_counts=None):
    """The conflict report of a round's best paths [N, 64, 2] (equal start times) on a cell table (mmd_path_conflicts_binned), built here
    when none is passed (constraints.binned_collision_table) -> (summary, robot_counts, list): the summary has find_conflicts' 16-word
    layout ([0] = count, [4:16] = the first record; `read_summary` / `decode_records` read it) and is what find_conflicts(..., PAIRS)
    gives for these paths; robot_counts int32 [N] = the (t, other robot) collisions of every robot; list [list_cap, 12] words or None.
    row_counts: an optional int32 [64] device tensor that receives the count per time step.  No N^2 buffer, no host synchronisation."""
    paths_all = paths_all.contiguous()
    if paths_all.shape[0] < 2 and table is None:               # one robot: nothing to collide with (and no table of fewer than two)
        summ, lst, _ = _new_report(paths_all.device, list_cap)
        summ.zero_()
        summ[4:7] = -1
        if row_counts is not None:
            row_counts.zero_()
        return summ, torch.zeros(paths_all.shape[0], dtype=torch.int32, device=paths_all.device), lst
    if table is None:
        from .constraints import binned_collision_table
        table = binned_collision_table(paths_all)
    _collision_table(table, "path_conflicts")
    n = paths_all.shape[0]
    if table.n_all != n or paths_all.shape[1] != H:
        raise ValueError(f"path_conflicts: paths {tuple(paths_all.shape)} and a table of {table.n_all} robots")
    dev = paths_all.device
    summ, lst, report_args = _new_report(dev, list_cap)
    rows = torch.empty(H, dtype=torch.int32, device=dev) if row_counts is None else row_counts
    if not (rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() == H):
        raise ValueError(f"path_conflicts: row_counts must be a contiguous int32 device tensor of {H} words")
    robots = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.launch("mmd_path_conflicts_binned", paths_all, _lib.require_gpu(paths_all, "paths_all"), C.byref(table.struct), H, float(margin),
                rows.data_ptr(), robots.data_ptr(), *report_args)
    return summ, robots, lst


REPLAN_MODES = {"conflicted": _lib.REPLAN_CONFLICTED, "independent": _lib.REPLAN_INDEPENDENT}


@dataclass
class ReplanSelection:
    """What select_replan returns, all on the device: selected int32 [N] (0 / 1), perm int32 [N] (the stable partition: the selected ids
    ascending, then the others ascending), header int32 [4] = (robots selected, of them below the table's robot0, of them in its shard,
    robots left undecided)."""
    selected: torch.Tensor
    perm: torch.Tensor
    header: torch.Tensor

    def read_header(self):
        """-> (n_selected, sel_before, n_sel_local, n_undecided) as ints: one 16-byte device -> host copy, made by the first call and
        kept (later calls copy nothing)."""
        host = self.__dict__.get("_header_host")
        if host is None:
            host = self.__dict__["_header_host"] = tuple(int(v) for v in self.header.cpu().numpy())
        return host


def select_replan(paths_all, table, robot_counts, mode="conflicted", iters=8, n_local=None, margin=RR_MARGIN):
    """The robots a round re-plans (mmd_round_select), from the round's best paths [N, 64, 2], their collision cell table
    (constraints.binned_collision_table) and path_conflicts' robot_counts of them.  mode "conflicted": every robot with a conflict;
    "independent": an independent set of the conflict graph, `iters` Jacobi iterations of priority propagation (a robot with more
    collisions beats one with fewer, the lower id wins a tie) -- no two selected robots meet, so each is re-planned against neighbours
    that keep their paths.  The shard of the header is [table.robot0, table.robot0 + n_local); n_local defaults to the table's.
    -> ReplanSelection.  No host synchronisation."""
    if mode not in REPLAN_MODES:
        raise ValueError(f"select_replan: mode must be one of {sorted(REPLAN_MODES)}, got {mode!r}")
    _collision_table(table, "select_replan")
    paths_all = paths_all.contiguous()
    n = paths_all.shape[0]
    if table.n_all != n or paths_all.shape[1] != H:
        raise ValueError(f"select_replan: paths {tuple(paths_all.shape)} and a table of {table.n_all} robots")
    if not (robot_counts.is_cuda and robot_counts.dtype == torch.int32 and robot_counts.is_contiguous() and robot_counts.numel() == n):
        raise ValueError(f"select_replan: robot_counts must be a contiguous int32 device tensor of {n} words")
    dev = paths_all.device
    state = torch.empty((2, n), dtype=torch.int32, device=dev)
    selected, perm, header = (torch.empty(m, dtype=torch.int32, device=dev) for m in (n, n, 4))
    _lib.launch("mmd_round_select", paths_all, _lib.require_gpu(paths_all, "paths_all"), C.byref(table.struct), robot_counts.data_ptr(),
                int(table.n_local if n_local is None else n_local), H, float(margin), REPLAN_MODES[mode], int(iters), state.data_ptr(),
                selected.data_ptr(), perm.data_ptr(), header.data_ptr())
    return ReplanSelection(selected, perm, header)


def decode_records(words):
    """int32 [m, 12] mmd_conflict records (host numpy) -> (t, a, b int arrays, pa, pb, mid float32 [m, 2] arrays)."""
    words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, _CONFLICT_WORDS)
    f = words.view(np.float32)
    return words[:, 0].copy(), words[:, 1].copy(), words[:, 2].copy(), f[:, 4:6].copy(), f[:, 6:8].copy(), f[:, 8:10].copy()


def read_summary(summ):
    """-> (count, first record as (t, a, b, pa, pb, mid) or None)."""
    h = summ.cpu().numpy()
    count = int(h[0])
    if count == 0:
        return 0, None
    t, a, b, pa, pb, mid = decode_records(h[4:16])
    return count, (int(t[0]), int(a[0]), int(b[0]), pa[0], pb[0], mid[0])


def scan_candidates(table, n, Tg, agent, cand_batch, cand_idx, mode, rule, init_idx=None, margin=RR_MARGIN, with_counts=False):
    """mmd_scan_candidates: the 'least_collisions' choice for agent `agent` over the samples cand_idx (device integer tensor, the order
    of trajs_final_free_idxs) of cand_batch [B, L, 4].  rule SELECT_PP starts from init_idx (idx_best_traj: an int or a device
    scalar).  -> int32 [2] device tensor (chosen index, count)[, int32 [n_free] every candidate's count]."""
    dev = table.device
    idx = cand_idx.reshape(-1).to(device=dev, dtype=torch.int32)
    n_free = int(idx.shape[0])
    if rule == SELECT_PP:
        if init_idx is None:
            raise ValueError("scan_candidates: the PP rule starts from init_idx (idx_best_traj)")
        idx = torch.cat((idx, torch.as_tensor(init_idx, device=dev).reshape(1).to(torch.int32)))
    scratch = torch.empty(int(Tg) + n_free + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(max(n_free, 1), dtype=torch.int32, device=dev) if with_counts else None
    result = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.launch("mmd_scan_candidates", table, table.data_ptr(), int(n), int(Tg), int(agent), _lib.require_gpu(cand_batch, "cand_batch"),
                idx.data_ptr(), n_free, float(margin), int(mode), int(rule), scratch.data_ptr(),
                counts.data_ptr() if counts is not None else None, result.data_ptr())
    return (result, counts[:n_free]) if with_counts else result


def path_constraint_extent(lengths, starts, agent, n_state, agent_start, agent_last, hard, horizon=H):
    """(whether the reference's point list is non-empty, slots of the ELL block) of the constraints the other agents' paths put on
    `agent` (cbs.py:468-508, prioritized_planning.py:149-159): a function of lengths and start times only."""
    fill = np.zeros(horizon, dtype=np.int64)
    any_point = False
    for j in range(n_state):
        if j == agent:
            continue
        last = agent_last if agent_last >= 0 else int(lengths[j]) - 1
        t_i = np.arange(int(lengths[j])) + int(starts[j]) - int(agent_start)
        t_i = t_i[(t_i >= 1) & (t_i <= last)]
        any_point |= t_i.size > 0
        t_i = t_i[t_i <= (horizon - 2 if hard else horizon - 1)]
        fill[t_i] += 1
    return any_point, int(fill.max()) if horizon else 0


def path_constraints_table(table, n_state, agent, agent_start, agent_last, hard, n_slots, radius=VERTEX_CONSTRAINT_RADIUS,
                           weight=2e-2, ell_out=None):
    """mmd_path_constraints -> (ell [n_slots, H, 4], grp_slot_off [2], grp_weight [1], robot_grp_off [2]).  With `ell_out` (a slice of
    a packed table) only the block is written there, no offsets."""
    dev = table.device
    if ell_out is not None:
        _lib.launch("mmd_path_constraints", table, table.data_ptr(), int(n_state), int(agent), int(agent_start), int(agent_last),
                    int(bool(hard)), H, float(radius), float(weight), int(n_slots), ell_out.data_ptr(), None, None, None)
        return ell_out
    from .constraints import group_tensors
    ell, gso, gw, rgo = group_tensors(max(n_slots, 1), 1, 1, dev)
    _lib.launch("mmd_path_constraints", table, table.data_ptr(), int(n_state), int(agent), int(agent_start), int(agent_last),
                int(bool(hard)), H, float(radius), float(weight), int(n_slots), ell.data_ptr(), gso.data_ptr(), gw.data_ptr(),
                rgo.data_ptr())
    return ell[:n_slots], gso, gw, rgo


class PathConstraints:
    """The constraints the other agents' chosen paths put on agent `agent`, as the two searches build them:
      * soft (is_soft=True): CBS.create_soft_constraints_from_other_agents_paths (cbs.py:468-508), ECBS;
      * hard (is_soft=False): the same points with the ranges clamped to [0, H-1], PrioritizedPlanning.plan (prioritized_planning.py:149-159).
    `paths`: the chosen-path batches of the agents in the state (SearchState.path_bl, device [B_k, L_k, 4]), `indices` their chosen samples,
    `start_times` every agent's start time (agent `agent` included), `n_state` the agents in the state (agents 0 .. n_state-1).  When the
    agent has a path in the state (agent < n_state) its points keep 1 <= t <= L_agent - 1, else 1 <= t <= L_j - 1 (the reference's rule).
    Handed to MPD.__call__(..., path_constraints=) and plan_batched, the group is built on the device (mmd_path_constraints) after the
    groups of constraints_l; `constraint_list()` is the reference's MultiPointConstraint form of the same group (MPDEnsemble, tests)."""

    def __init__(self, paths, indices, agent, start_times=None, n_state=None, is_soft=True, radius=VERTEX_CONSTRAINT_RADIUS):
        self.paths = list(paths)
        self.indices = [int(i) for i in indices]
        self.n_state = len(self.paths) if n_state is None else int(n_state)
        self.agent = int(agent)
        n_all = max(self.n_state, self.agent + 1)
        self.start_times = [0] * n_all if start_times is None else [int(s) for s in start_times]
        self.is_soft = bool(is_soft)
        self.radius = float(radius)
        if len(self.indices) < self.n_state or len(self.paths) < self.n_state or len(self.start_times) < n_all:
            raise ValueError("PathConstraints: a path, an index and a start time for every agent in the state")

    @property
    def lengths(self):
        return [int(p.shape[1]) for p in self.paths[:self.n_state]]

    def agent_last_t(self):
        return int(self.paths[self.agent].shape[1]) - 1 if self.agent < self.n_state else -1

    def extent(self):
        return path_constraint_extent(self.lengths, self.start_times, self.agent, self.n_state, self.start_times[self.agent],
                                      self.agent_last_t(), not self.is_soft)

    def table(self, device=None):
        return agent_table(self.paths[:self.n_state], self.indices[:self.n_state], self.start_times[:self.n_state], device)

    def build(self, weight, ell_out=None, n_slots=None, table=None):
        n_slots = self.extent()[1] if n_slots is None else n_slots
        table = self.table() if table is None else table
        return path_constraints_table(table, self.n_state, self.agent, self.start_times[self.agent], self.agent_last_t(),
                                      not self.is_soft, n_slots, self.radius, weight, ell_out)

    def points(self):
        """The reference's point list (q [n, 2] host float32, t_range list of (t0, t1)) in its order: other agent j ascending, t_j ascending."""
        q_l, r_l = [], []
        s_i, last_i = self.start_times[self.agent], self.agent_last_t()
        for j in range(self.n_state):
            if j == self.agent:
                continue
            L_j = int(self.paths[j].shape[1])
            last = last_i if last_i >= 0 else L_j - 1
            t_i = np.arange(L_j) + self.start_times[j] - s_i
            keep = (t_i >= 1) & (t_i <= last)
            if not keep.any():
                continue
            q_l.append(self.paths[j][self.indices[j], :, :2].detach().cpu().numpy()[keep])
            r_l.extend((int(t), int(t) + 1) for t in t_i[keep])
        q = np.concatenate(q_l).astype(np.float32) if q_l else np.zeros((0, 2), np.float32)
        if not self.is_soft:
            r_l = [(max(0, min(t0, H - 1)), min(H - 1, t1)) for t0, t1 in r_l]        # prioritized_planning.py:155-158
        return q, r_l

    def constraint_list(self):
        """[MultiPointConstraint] as the reference builds it (empty if there are no points)."""
        from .constraints import MultiPointConstraint
        q, r_l = self.points()
        if not r_l:
            return []
        return [MultiPointConstraint(q_l=torch.from_numpy(q), t_range_l=r_l, radius_l=[self.radius] * len(r_l), is_soft=self.is_soft)]
