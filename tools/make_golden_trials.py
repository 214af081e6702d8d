#!/usr/bin/env python
"""Write tests/golden/g24_trial_stats.npz from the GENUINE reference functions (imported through tools/ref_bootstrap.py; build
container only).  Inputs come from tests/trial_cases.py (numpy PCG64 seeds); the file stores arrays only: the reference's outputs and,
for checking that the regenerated inputs are the recorded ones, the inputs.

    python tools/make_golden_trials.py

Per case of trial_cases.G24_CASES:
  <case>.paths [n, Tg, 4], <case>.tiles [m, 5] (agent, t0, offset_x, offset_y, rule)
  <case>.adherence [m]      each env class's compute_traj_data_adherence on the tile's 64 rows in the tile frame
  <case>.highways_sum [m]   (rule highways only, else 0) the reference's aggregate cross product: |sum| >= 1e-2 or NaN is asserted here
  <case>.path_length [n]    compute_path_length_from_pos;  <case>.mean_accel [n]  compute_average_acceleration_from_pos_vel
  <case>.pair_collisions    the pair loop of inference_multi_agent.py:288-294 at 2.0 * robot_planar_disk_radius
  <case>.trial [4] float64  (cases with tiles) data_adherence, path_length_per_agent, mean_path_acceleration_per_agent, success status
                            value after the collision rule, accumulated the way inference_multi_agent.py:295-342 accumulates them
and the formation helpers of mmd/common/multi_agent_utils.py:146-181 for N in {3, 10, 12}: circle.<N>.{start,goal} (radius 0.8),
small_circle.<N>.{start,goal} (radius 0.45), boundary.<N>.{start,goal}, column.<N> (x_pos = -0.6)."""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ref_bootstrap import bootstrap          # noqa: E402

bootstrap()
import torch                                  # noqa: E402

import trial_cases as TC                      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g24_trial_stats.npz")
TENSOR_ARGS = dict(device="cpu", dtype=torch.float32)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def reference_case(envs, paths, tiles):
    from mmd.config.mmd_params import MMDParams as params
    from mmd.common.experiments import TrialSuccessStatus
    from torch_robotics.trajectory.metrics import compute_path_length_from_pos, compute_average_acceleration_from_pos_vel
    paths_l = [torch.from_numpy(p.copy()) for p in paths]
    n = len(paths_l)
    out = {}
    # the pair loop
    collisions = 0
    for t in range(len(paths_l[0])):
        for i in range(n):
            for j in range(i + 1, n):
                if torch.norm(paths_l[i][t, :2] - paths_l[j][t, :2]) < 2.0 * params.robot_planar_disk_radius:
                    collisions += 1
    out["pair_collisions"] = np.int32(collisions)
    status = TrialSuccessStatus.FAIL_COLLISION_AGENTS if collisions > 0 else TrialSuccessStatus.SUCCESS
    # per tile
    adherence, sums = [], []
    for agent, t0, ox, oy, rule in tiles:
        local = paths_l[agent].clone()[t0:t0 + params.horizon, :2] - torch.tensor([ox, oy], **TENSOR_ARGS)
        env = envs[TC.RULE_ENV[rule]]
        adherence.append(float(_quiet(env.compute_traj_data_adherence, local)))
        s = 0.0
        if rule == TC.R.RULE_HIGHWAYS:
            v = local / torch.norm(local, dim=1, keepdim=True)
            s = float(torch.sum(v[:-1, 0] * v[1:, 1] - v[:-1, 1] * v[1:, 0]))
            assert np.isnan(s) or abs(s) >= 1e-2, ("highways case too close to zero", agent, t0, s)
        sums.append(s)
    out["adherence"] = np.array(adherence, np.float32)
    out["highways_sum"] = np.array(sums, np.float32)
    # per agent
    length = [compute_path_length_from_pos(p[:, :2].unsqueeze(0)).item() for p in paths_l]
    accel = [compute_average_acceleration_from_pos_vel(p[:, :2].unsqueeze(0), p[:, 2:].unsqueeze(0)).item() for p in paths_l]
    out["path_length"] = np.array(length, np.float32)
    out["mean_accel"] = np.array(accel, np.float32)
    if tiles:
        data_adherence = 0.0
        for a in range(n):
            own = [adherence[k] for k, t in enumerate(tiles) if t[0] == a]
            agent_adherence = 0.0
            for v in own:
                agent_adherence += v
            data_adherence += agent_adherence / len(own)
        data_adherence /= n
        pl = ac = 0.0
        for a in range(n):
            pl += length[a]
            ac += accel[a]
        out["trial"] = np.array([data_adherence, pl / n, ac / n, status.value], np.float64)
    return out


def formations():
    import mmd.common.multi_agent_utils as mu
    real = torch.tensor

    def cpu_tensor(*a, **k):                  # the helpers hard-code device='cuda'
        k["device"] = "cpu"
        return real(*a, **k)
    out = {}
    mu.torch.tensor = cpu_tensor
    try:
        for n in (3, 10, 12):
            for name, (s, g) in (("circle", mu.get_start_goal_pos_circle(n, radius=0.8)),
                                 ("small_circle", mu.get_start_goal_pos_circle(n, radius=0.45)),
                                 ("boundary", mu.get_start_goal_pos_boundary(n, dist=0.87))):
                out[f"{name}.{n}.start"], out[f"{name}.{n}.goal"] = torch.stack(s).numpy(), torch.stack(g).numpy()
            out[f"column.{n}"] = torch.stack(mu.get_state_pos_column(n, -0.6)).numpy()
    finally:
        mu.torch.tensor = real
    return out


def write_npz(path, arrays):
    """np.savez_compressed with a fixed member date and order: a re-run gives the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def main():
    import torch_robotics.environments as E
    envs = {name: _quiet(getattr(E, name), tensor_args=TENSOR_ARGS) for name in set(TC.RULE_ENV.values()) | {"EnvEmptyNoWait2D"}}
    out = {}
    for name, make in TC.G24_CASES.items():
        paths, tiles = make()
        out[f"{name}.paths"] = paths
        out[f"{name}.tiles"] = np.array(tiles, np.float64).reshape(-1, 5)
        for k, v in reference_case(envs, paths, tiles).items():
            out[f"{name}.{k}"] = v
        print(name, paths.shape, len(tiles), "tiles; collisions", int(out[f"{name}.pair_collisions"]), "adherence",
              np.round(out[f"{name}.adherence"], 3).tolist())
    # EnvEmptyNoWait2D shares the line rule: its own class on the line case
    paths, tiles = TC.G24_CASES["line"]()
    out["line.adherence_nowait"] = np.array([float(_quiet(envs["EnvEmptyNoWait2D"].compute_traj_data_adherence,
                                                          torch.from_numpy(paths[a, t0:t0 + 64, :2].copy()))) for a, t0, *_ in tiles], np.float32)
    out.update(formations())
    write_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
