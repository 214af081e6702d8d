"""The scripted low-level planner of golden g23 (tools/make_golden.py) and its replay (tests/test_gpu_mapf.py, tests/test_mapf_host.py).

A ScriptedPlanner stands in for MPD: call n of agent k returns entry n (mod the script length) of that agent's script -- a synthetic
[B, L, 4] batch, its free indices and idx_best_traj -- and logs what it was called with (the constraints, whether an experience came).
The searches drive it the same way whether they are the reference's or this package's, so the logs and results must agree exactly."""
import numpy as np
import torch

B = 8
H = 64
STAGGER = 5
N_ENTRIES = 4


def script_batch(agent, entry, n_agents, length, seed):
    """Agent `agent` goes from its circle position to the antipode over `length` steps; sample b detours sideways by an amplitude that
    grows with |b - 3.5| and with the entry (later re-plans detour further)."""
    ang = 2 * np.pi * agent / n_agents
    s = np.array([0.6 * np.cos(ang), 0.6 * np.sin(ang)], np.float32)
    g = -s
    u = np.linspace(0.0, 1.0, length, dtype=np.float32)
    perp = np.array([-s[1], s[0]], np.float32) / np.float32(0.6)
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((B, length, 4), np.float32)
    for b in range(B):
        amp = np.float32(0.05 * (b - 3.5) * (1 + entry))
        pos = s[None] * (1 - u[:, None]) + g[None] * u[:, None] + amp * np.sin(np.pi * u)[:, None] * perp[None]
        pos = pos + np.float32(0.004) * rng.standard_normal(pos.shape).astype(np.float32)
        pos[0], pos[-1] = s, g
        out[b, :, :2] = pos
        out[b, :, 2:] = np.gradient(pos, axis=0)
    return out


def script_free(agent, entry, fail=False):
    """The free indices of an entry (increasing, as trajs_final_free_idxs) and idx_best_traj (a free index in the middle)."""
    if fail:
        return np.zeros(0, np.int64), -1
    free = np.array([b for b in range(B) if (b + agent + entry) % 3 != 0], np.int64)
    return free, int(free[len(free) // 2])


def make_script(n_agents, lengths, fail_at=None, seed=0):
    """{agent: [(batch, free, best), ...]}; fail_at = (agent, entry): that entry has no free sample."""
    script = {}
    for k in range(n_agents):
        script[k] = []
        for e in range(N_ENTRIES):
            batch = script_batch(k, e, n_agents, lengths[k], seed + 100 * k + e)
            free, best = script_free(k, e, fail_at == (k, e))
            script[k].append((batch, free, best))
    return script


class _Out:
    pass


class ScriptedPlanner:
    def __init__(self, agent, entries, log, robot, task, device="cpu"):
        self.agent, self.entries, self.log, self.robot, self.task = agent, entries, log, robot, task
        self.device = torch.device(device)
        self.tensor_args = {"device": self.device, "dtype": torch.float32}
        self.results_dir = "logs"
        self.n_calls = 0

    def __call__(self, start_state_pos, goal_state_pos, constraints_l=None, experience=None, *args, **kwargs):
        batch, free, best = self.entries[self.n_calls % len(self.entries)]
        self.n_calls += 1
        cons = []
        for c in constraints_l or []:
            q = torch.stack([torch.as_tensor(v).reshape(-1)[:2].to("cpu", torch.float32) for v in c.q_l]).numpy() \
                if len(c.q_l) else np.zeros((0, 2), np.float32)
            r = np.asarray(c.t_range_l, dtype=np.float64).reshape(-1, 2)
            cons.append((q.astype(np.float32), r, np.asarray(c.radius_l, np.float64).reshape(-1), bool(c.is_soft)))
        self.log.append((self.agent, cons, experience is not None))
        out = _Out()
        out.trajs_final = torch.from_numpy(batch.copy()).to(self.device)
        out.trajs_final_free_idxs = torch.from_numpy(free.copy()).to(self.device)
        out.idx_best_traj = torch.tensor(best, device=self.device) if best >= 0 else None
        return out


def log_to_arrays(log):
    """The call log as numeric arrays: calls [n, 3] (agent, number of constraints, experience passed), cons [m, 2] (points, is_soft),
    points [p, 5] (qx, qy, t0, t1, radius)."""
    calls, cons, pts = [], [], []
    for agent, cl, exp in log:
        calls.append((agent, len(cl), int(exp)))
        for q, r, rad, soft in cl:
            cons.append((q.shape[0], int(soft)))
            for k in range(q.shape[0]):
                pts.append((q[k, 0], q[k, 1], r[k, 0], r[k, 1], rad[k]))
    return (np.array(calls, np.int64).reshape(-1, 3), np.array(cons, np.int64).reshape(-1, 2), np.array(pts, np.float64).reshape(-1, 5))


class RecordingList(list):
    """An open list that records (chosen indices, number of conflicts) of every node appended to it."""

    def __init__(self):
        super().__init__()
        self.record = []

    def append(self, state):
        self.record.append((list(int(i) for i in state.ix_best_path_in_batch_l), len(state.conflict_l)))
        super().append(state)


def starts_goals(n_agents):
    ang = 2 * np.pi * np.arange(n_agents) / n_agents
    s = np.stack([0.6 * np.cos(ang), 0.6 * np.sin(ang)], 1).astype(np.float32)
    return s, -s


# the g23 cases: (name, planner, flags, n agents, lengths, start stagger, failing entry)
CASES = [
    ("pp", "PP", {}, 4, [64, 64, 64, 64], STAGGER, None),
    ("pp_mixed", "PP", {}, 4, [64, 128, 64, 64], STAGGER, None),
    ("cbs", "CBS", dict(is_ecbs=False, is_xcbs=False), 4, [64, 64, 64, 64], STAGGER, (1, 1)),
    ("ecbs", "CBS", dict(is_ecbs=True, is_xcbs=False), 4, [64, 64, 64, 64], STAGGER, None),
    ("xecbs", "CBS", dict(is_ecbs=True, is_xcbs=True), 4, [64, 128, 64, 64], STAGGER, (0, 1)),
]
