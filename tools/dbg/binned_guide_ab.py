"""A/B of the two inter-robot constraint tables on one GPU, in ONE process: the all-pairs table (mmd_soft_constraints_from_paths, N - 1
slots per robot) against the cell table (mmd_bin_constraints_from_paths), on the weak-scaling instances of tools/dbg/shard_cost.py --
rank 0 of an N / 32-GPU job: 32 local robots x 64 samples of an N-robot circle instance, N = 32, 64, 128, 256.
  guided step: the kernel time of one guide launch (mmd_guide_steps: 20 guide iterations on the 2048 trajectories a round ends with,
               which is what the guided step kernel adds to a UNet launch), HIP events around every launch, the two tables alternating in
               blocks of 10 launches until each has filled a second
  round:       table build + guided sampling call (T = 100 + 1) + best-path pick, host clock around a synchronised round, alternating
Every shape is warmed up first; the two tables' outputs are compared bit for bit on every run (the yardstick is the dense path).
Usage: python tools/dbg/binned_guide_ab.py [--out FILE] [N ...]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from mmd_amd import synth, _lib
from mmd_amd.diffusion_model import GaussianDiffusionModel
from mmd_amd.multi_robot import MultiRobotSampler
from mmd_amd.temporal_unet import TemporalUnet

H, B, LOCAL, N_GUIDE = 64, 64, 32, 20
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


unet = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=32, dim_mults=(1, 2, 4))
unet.load_state_dict(synth.synth_unet_state_dict(0))
model = GaussianDiffusionModel(model=unet, variance_schedule="exponential", n_diffusion_steps=100, predict_epsilon=True)
say(f"{torch.cuda.get_device_name(0)}; {LOCAL} local robots x {B} samples = {LOCAL * B} trajectories; guided step = one launch of {N_GUIDE} guide "
    f"iterations; round = table + sampling call (T = 100 + 1) + best-path pick")
say(f"{'robots':>6} {'slots':>6} {'entries/list':>12} | {'step dense us':>13} {'step binned us':>14} {'ratio':>6} | {'round dense ms':>14} "
    f"{'round binned ms':>15} {'ratio':>6} | {'table dense MB':>14} {'table binned MB':>15}")
crossover = None
for N in [int(a) for a in args] or [32, 64, 128, 256]:
    starts, goals = synth.start_goal_circle(N, 0.8)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    S = {t: MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, rank=0, world_size=N // LOCAL, device="cuda",
                              constraint_table=t) for t in ("dense", "binned")}

    def one_round(t, seed):
        s = S[t]
        s.set_other_paths(paths)
        tr = s.sample(seed=seed)
        return tr, s.best_paths(tr, paths)

    # ---- rounds: warm up both, then alternate
    for _ in range(2):
        ref = {t: one_round(t, 1) for t in S}
    assert torch.equal(ref["dense"][0], ref["binned"][0]) and torch.equal(ref["dense"][1], ref["binned"][1])
    round_ms = {t: 0.0 for t in S}
    n_rounds = 4
    for k in range(n_rounds):
        got = {}
        for t in S:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            got[t] = one_round(t, 10 + k)
            torch.cuda.synchronize(); round_ms[t] += (time.perf_counter() - t0) * 1e3 / n_rounds
        assert torch.equal(got["dense"][0], got["binned"][0]) and torch.equal(got["dense"][1], got["binned"][1]), (N, k)

    # ---- the guide launch on the trajectories the round ended with
    x0 = ref["dense"][0].contiguous()
    hard = torch.stack([S["dense"].hard_conds[0], S["dense"].hard_conds[H - 1]], 1).contiguous()
    y = {t: torch.empty_like(x0) for t in S}

    def block(t, n, events=None):
        g = S[t].guide
        for _ in range(n):
            y[t].copy_(x0)
            if events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            g.guide_steps(y[t], hard, _lib.HARD_ROWS_START_GOAL, N_GUIDE)
            if events is not None:
                e1.record()
                events.append((e0, e1))

    for t in S:
        block(t, 5)
    torch.cuda.synchronize()
    assert torch.equal(y["dense"], y["binned"]) and not torch.equal(y["dense"], x0)
    step_us, n_launch = {t: 0.0 for t in S}, {t: 0 for t in S}
    while min(step_us.values()) < 1e6 and max(n_launch.values()) < 20000:
        for t in S:
            ev = []
            block(t, 10, ev)
            torch.cuda.synchronize()
            step_us[t] += sum(a.elapsed_time(b) for a, b in ev) * 1e3
            n_launch[t] += len(ev)
        assert torch.equal(y["dense"], y["binned"]), N
    us = {t: step_us[t] / n_launch[t] for t in S}
    tab = S["binned"].guide._binned
    off = tab.cell_off.cpu()
    per_list = float((off[1:, 1:] - off[1:, :-1]).float().mean())
    dense_mb = S["dense"].guide._external_cons[0].numel() * 4 / 1e6
    binned_mb = (tab.cell_off.numel() + tab.entries.numel()) * 4 / 1e6
    say(f"{N:>6} {N - 1:>6} {per_list:>12.1f} | {us['dense']:>13.1f} {us['binned']:>14.1f} {us['binned'] / us['dense']:>6.2f} | "
        f"{round_ms['dense']:>14.2f} {round_ms['binned']:>15.2f} {round_ms['binned'] / round_ms['dense']:>6.2f} | {dense_mb:>14.1f} "
        f"{binned_mb:>15.1f}   ({n_launch['dense']} + {n_launch['binned']} guide launches, {n_rounds} + {n_rounds} rounds, outputs equal)")
    if crossover is None and us["binned"] < us["dense"]:
        crossover = N
say(f"guided step: the cell table is the faster one from N = {crossover} on" if crossover else
    "guided step: the cell table is slower than the all-pairs table at every N measured")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
