#!/usr/bin/env python
"""Wall time of the multi-agent search layer (mmd_amd.multi_agent_planners) on the GPU: per PrioritizedPlanning agent and per ECBS expansion
at 10 and 32 robots over real MPD planners (synthetic weights, EnvEmpty2D, 64 samples), split into low-level planner time and search-layer
time, and the search-layer pieces on their own (conflict search, candidate scan, constraint build, state copies).

    python tools/dbg/mapf_time.py [--T 25] [--ecbs-limit 20] [--out profiles/mapf_time.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from mmd_amd import multi_agent as ma, synth                 # noqa: E402
from mmd_amd.multi_agent_planners import CBS, PrioritizedPlanning, SearchState  # noqa: E402
from mmd_amd.planners import MPD                              # noqa: E402


def planners(n, T, B):
    starts, goals = synth.start_goal_circle(n, 0.85)
    sd = synth.synth_unet_state_dict(0)
    ps = [MPD(model_id="EnvEmpty2D-RobotPlanarDisk", planner_alg="mmd", start_state_pos=torch.from_numpy(starts[k]),
              goal_state_pos=torch.from_numpy(goals[k]), device="cuda", seed=100 + k, n_samples=B, model_state_dict=sd,
              model_args=dict(n_diffusion_steps=T), trained_models_dir="") for k in range(n)]
    return ps, [torch.from_numpy(v) for v in starts], [torch.from_numpy(v) for v in goals]


def timed(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def pieces(n, B=64):
    """Search-layer pieces on a synthetic state of n agents (straight lines + noise, 64 samples each, start times staggered by 5)."""
    starts, goals = synth.start_goal_circle(n, 0.85)
    lines = synth.straight_line_paths(starts, goals, 64)
    batches = []
    for k in range(n):
        b = np.repeat(lines[k:k + 1], B, 0) + 0.03 * synth.synth_noise(900 + k, (B, 64, 2))
        batches.append(torch.from_numpy(np.concatenate([b, np.zeros_like(b)], -1).astype(np.float32)).cuda())
    times = [5 * (k % 4) for k in range(n)]
    ix = [0] * n
    state = SearchState(list(ix), list(batches))
    lengths = [64] * n
    Tg = ma.global_horizon(lengths, times)
    free = torch.arange(B, device="cuda").view(-1, 1)
    table = ma.agent_table(batches, ix, times)

    def conflicts():
        ma.read_summary(ma.find_conflicts(ma.agent_table(batches, ix, times), n, Tg, ma.ORDERED)[0])

    def scan():
        ma.scan_candidates(ma.agent_table(batches, ix, times), n, Tg, 1, batches[1], free, ma.ORDERED, ma.SELECT_CBS).cpu()

    pc = ma.PathConstraints(batches, ix, 1, times, is_soft=True)

    def build():
        pc.build(2e-2)

    def copy():
        state.get_copy(share_paths=True)

    def table_upload():
        ma.agent_table(batches, ix, times)

    return {"conflict_search_ms": timed(conflicts), "candidate_scan_ms": timed(scan), "constraint_build_ms": timed(build),
            "state_copy_ms": timed(copy), "agent_table_upload_ms": timed(table_upload),
            "conflict_kernels_only_ms": timed(lambda: ma.find_conflicts(table, n, Tg, ma.ORDERED))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=25)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--ecbs-limit", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = {"device": torch.cuda.get_device_name(0), "T": a.T, "B": a.B}
    for n in (10, 32):
        r = {"pieces": pieces(n, a.B)}
        ps, sl, gl = planners(n, a.T, a.B)
        ps[0](sl[0], gl[0])                                       # (warm-up: model handle, textures)
        torch.cuda.synchronize()
        pp = PrioritizedPlanning(ps, sl, gl)
        t0 = time.perf_counter()
        _, _, status, n_conf = pp.plan(runtime_limit=600)
        wall = time.perf_counter() - t0
        r["pp"] = {"status": status.name, "n_conflicts": n_conf, "wall_s": wall, "per_agent_ms": wall / n * 1e3,
                   "low_level_per_agent_ms": pp.timing["low_level"] / n * 1e3, "search_per_agent_ms": pp.timing["search"] / n * 1e3}
        for batch in (True, False):
            ecbs = CBS(ps, sl, gl, is_ecbs=True, batch_expansions=batch)
            t0 = time.perf_counter()
            _, n_exp, status, n_conf = ecbs.plan(runtime_limit=a.ecbs_limit)
            wall = time.perf_counter() - t0
            root_calls = n
            e = max(n_exp, 1)
            r[f"ecbs_batched={batch}"] = {"status": status.name, "expansions": n_exp, "n_conflicts": n_conf, "wall_s": wall,
                                          "per_expansion_ms_incl_root": wall / e * 1e3,
                                          "low_level_s": ecbs.timing["low_level"], "search_s": ecbs.timing["search"],
                                          "search_per_expansion_ms": ecbs.timing["search"] / e * 1e3, "root_calls": root_calls}
        rows[f"n={n}"] = r
        print(json.dumps({f"n={n}": r}, indent=1), flush=True)
    txt = json.dumps(rows, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
