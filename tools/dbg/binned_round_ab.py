"""A/B of the stages of a many-robot round that follow the sampler, all-pairs against cell table, on one GPU in ONE process:
  pick:    mmd_count_collisions against mmd_count_collisions_binned, rank 0's share of an N-robot round (32 local robots x 64 samples =
           2048 trajectories: the robots' straight lines plus noise of 0.05) against the N best paths; the cell-table side is timed twice,
           the count alone and the count with the table build (mmd_bin_paths) it needs once per round
  report:  mmd_find_conflicts(PAIRS) against mmd_bin_paths + mmd_path_conflicts_binned (count, rows, first record, per-robot counts, no list)
on the circle instance (every path crosses the centre: one long list) and a random instance (starts and goals uniform in +-0.95, seeded),
N = 32, 128, 512, 1024.
HIP events around every call; every shape is warmed up; the two sides alternate in blocks of 20 calls until each has filled half a second;
the outputs are compared for equality on every shape (the yardstick is the all-pairs side).  No N^2 mask is allocated anywhere.
Usage: python tools/dbg/binned_round_ab.py [--out FILE] [N ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from mmd_amd import multi_agent as ma, synth
from mmd_amd.constraints import binned_collision_table

H, B, LOCAL = 64, 64, 32
args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def instance(kind, n):
    if kind == "circle":
        starts, goals = synth.start_goal_circle(n, 0.8)
    else:                                     # (trials.get_start_goal_pos_random_in_env keeps robots 0.15 apart: 64 do not fit, 1024 cannot)
        rng = np.random.Generator(np.random.PCG64(n))
        starts, goals = rng.uniform(-0.95, 0.95, (n, 2)), rng.uniform(-0.95, 0.95, (n, 2))
    return synth.straight_line_paths(np.asarray(starts, np.float32), np.asarray(goals, np.float32), H)


def alternate(sides, budget_ms=500.0, block=20, max_calls=4000):
    """{name: callable} -> {name: mean us per call}, HIP events around every call, the sides alternating in blocks"""
    for f in sides.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    total, calls = {k: 0.0 for k in sides}, {k: 0 for k in sides}
    while min(total.values()) < budget_ms and max(calls.values()) < max_calls:
        for name, f in sides.items():
            ev = []
            for _ in range(block):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            total[name] += sum(a.elapsed_time(b) for a, b in ev)
            calls[name] += block
    return {k: total[k] * 1e3 / calls[k] for k in sides}, calls


say(f"{torch.cuda.get_device_name(0)}; pick: {LOCAL} local robots x {B} samples = {LOCAL * B} trajectories against N best paths; report: the N best "
    f"paths; us per call, HIP events")
say(f"{'instance':>8} {'N':>5} {'entries/list':>12} | {'pick dense':>10} {'pick binned':>11} {'+ table':>8} {'ratio':>6} | {'report dense':>12} "
    f"{'report binned':>13} {'ratio':>6} | {'pairs':>9}")
for kind in ("circle", "random"):
    for N in [int(a) for a in args] or [32, 128, 512, 1024]:
        paths_np = instance(kind, N)
        paths = torch.from_numpy(paths_np).cuda()
        tr = np.zeros((LOCAL, B, H, 4), np.float32)
        tr[..., :2] = paths_np[:LOCAL, None]
        tr += synth.synth_noise(N, tr.shape) * np.float32(0.05)
        trajs = torch.from_numpy(tr.reshape(LOCAL * B, H, 4)).cuda()
        tab = binned_collision_table(paths, 0, LOCAL)
        off = tab.cell_off.cpu()
        per_list = float((off[:, 1:] - off[:, :-1]).float().mean())
        p4 = torch.zeros((N, 1, H, 4), device="cuda")
        p4[:, 0, :, :2] = paths
        agents = ma.agent_table([p4[k] for k in range(N)], [0] * N, [0] * N)

        dense = ma.count_collisions(trajs, paths, 0, LOCAL)
        assert torch.equal(ma.count_collisions_binned(trajs, tab, LOCAL), dense), (kind, N)
        sd, _ = ma.find_conflicts(agents, N, H, ma.PAIRS)
        sb, robots, _ = ma.path_conflicts(paths)
        assert torch.equal(sd[:1], sb[:1]) and torch.equal(sd[4:], sb[4:]), (kind, N)
        assert int(robots.sum()) == 2 * int(sd[0]), (kind, N)

        pick, calls = alternate({
            "dense": lambda: ma.count_collisions(trajs, paths, 0, LOCAL),
            "binned": lambda: ma.count_collisions_binned(trajs, tab, LOCAL),
            "binned+table": lambda: ma.count_collisions_binned(trajs, binned_collision_table(paths, 0, LOCAL), LOCAL)})
        rep, calls_r = alternate({
            "dense": lambda: ma.find_conflicts(agents, N, H, ma.PAIRS),
            "binned": lambda: ma.path_conflicts(paths)})
        say(f"{kind:>8} {N:>5} {per_list:>12.1f} | {pick['dense']:>10.1f} {pick['binned']:>11.1f} {pick['binned+table']:>8.1f} "
            f"{pick['binned+table'] / pick['dense']:>6.2f} | {rep['dense']:>12.1f} {rep['binned']:>13.1f} {rep['binned'] / rep['dense']:>6.2f} | "
            f"{int(sd[0]):>9}   ({calls['dense']} + {calls['binned']} + {calls['binned+table']} pick calls, {calls_r['dense']} + "
            f"{calls_r['binned']} report calls, outputs equal)")
say("ratio = cell table (table build included) / all-pairs; the event pairs include the host's enqueue gaps of the Python wrappers on both sides")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
