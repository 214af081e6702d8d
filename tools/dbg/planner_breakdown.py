"""Where the wall time of ONE MPD planner call goes (B = 64, T = 25): host work before the first kernel, the device
span of the sampling loop, post-processing + the one device -> host transfer.  Usage: planner_breakdown.py [n_samples] [T]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from mmd_amd import planners, synth
from mmd_amd.planners import MPD

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T = int(sys.argv[2]) if len(sys.argv) > 2 else 25
starts, goals = synth.start_goal_circle(10, 0.45)
p = MPD(model_id="EnvHighways2D-RobotPlanarDisk", planner_alg="mmd", start_state_pos=torch.from_numpy(starts[3]),
        goal_state_pos=torch.from_numpy(goals[3]), n_samples=B, device="cuda", model_state_dict=synth.synth_unet_state_dict(0),
        model_args=dict(n_diffusion_steps=T), trained_models_dir="")
s, g = torch.from_numpy(starts[3]), torch.from_numpy(goals[3])
for _ in range(5):
    p(s, g)
torch.cuda.synchronize()
marks = {}
orig_run, orig_fill = p.run_constrained_inference, planners._planner_outputs


def run(*a, **k):
    marks["t_run0"] = time.perf_counter()
    e0.record()
    out = orig_run(*a, **k)
    e1.record()
    marks["t_run1"] = time.perf_counter()
    return out


def fill(*a, **k):
    marks["t_fill0"] = time.perf_counter()
    out = orig_fill(*a, **k)
    marks["t_fill1"] = time.perf_counter()
    return out


p.run_constrained_inference, planners._planner_outputs = run, fill
rows = []
for _ in range(12):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = p(s, g)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    rows.append((t1 - t0, marks["t_run0"] - t0, marks["t_run1"] - marks["t_run0"], e0.elapsed_time(e1) * 1e-3, marks["t_fill0"] - marks["t_run1"],
                 marks["t_fill1"] - marks["t_fill0"], t1 - marks["t_fill1"]))
rows.sort()
r = rows[len(rows) // 2]
print(f"B={B} T={T} no constraints, median of {len(rows)}: call {1e3 * r[0]:.2f} ms = before the sampler {1e3 * r[1]:.3f} + sampler host enqueue {1e3 * r[2]:.3f} "
      f"(device span of the loop {1e3 * r[3]:.3f}) + timer sync / unnormalise {1e3 * r[4]:.3f} + post-processing incl. the transfer {1e3 * r[5]:.3f} + rest {1e3 * r[6]:.3f}")
