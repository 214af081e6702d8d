"""The round's pick (mmd_amd/csrc/round_pick.hip: mmd_round_pick_paths) as a definition on the CPU, from code that shares nothing with the
HIP sources: the un-normalisation in numpy float32 (every operation rounded once), the free flag from the oracle's
get_trajs_collision_and_free on the robot's own GuideParams, the robot-robot counts from fp32_forms.torch_norm2 against the float32 margin
the kernel is passed, the cost key from the oracle's path length + smoothness in float64, and the rule from post_edge_cases.expected_pick.
Host only; tests/test_round_pick_cases_host.py and tests/test_gpu_round_pick_edges.py hold the kernels to it."""
import dataclasses

import numpy as np
import torch

import fp32_forms as F
import post_edge_cases as E
from oracle import mmd_oracle as O

H, D = 64, 4


def unnormalise(x, norm_min, norm_max):
    """float32 (clip(x, -1, 1) + 1) / 2 * (max - min) + min over the last axis' limits: the clip on every element, a NaN stays a NaN"""
    x = np.asarray(x, np.float32)
    lo, hi = np.asarray(norm_min, np.float32), np.asarray(norm_max, np.float32)
    c = np.where(np.isnan(x), x, np.minimum(np.maximum(x, np.float32(-1)), np.float32(1))).astype(np.float32)
    half = ((c + np.float32(1)) / np.float32(2)).astype(np.float32)
    return ((half * (hi - lo)).astype(np.float32) + lo).astype(np.float32)


def free_flags(trajs_u, gp, num_interpolation, margin, q_min, q_max):
    """bool [n]: the oracle's free samples of un-normalised float32 trajectories [n, H, 4] on one robot's GuideParams, the map and the
    workspace walls compared against `margin`"""
    gp = dataclasses.replace(gp, robot_radius=float(np.float32(margin)))
    q_min, q_max = (tuple(float(np.float32(v)) for v in q) for q in (q_min, q_max))
    _, _, _, free_idxs, _ = O.get_trajs_collision_and_free(torch.from_numpy(np.ascontiguousarray(trajs_u)), gp,
                                                           num_interpolation=num_interpolation, q_min=q_min, q_max=q_max)
    free = np.zeros(len(trajs_u), bool)
    free[free_idxs.reshape(-1).numpy()] = True
    return free


def collision_counts(pos_u, paths_all, self_idx, rr_margin):
    """int64 [n]: #{(t, j != self_idx): ||pos_u[b, t] - paths_all[j, t]|| < float32(rr_margin)} in the torch form of the norm.  (The oracle's
    count_collisions_with_others takes a radius and multiplies it by 2.1 in double; the kernel is passed the margin as a float32.)"""
    others = np.delete(np.asarray(paths_all, np.float32), self_idx, axis=0)                     # [N - 1, H, 2]
    d = F.pos_norm(np.asarray(pos_u, np.float32)[:, None], others[None])                        # [n, N - 1, H]
    return (d < np.float32(rr_margin)).sum(axis=(1, 2)).astype(np.int64)


def cost_keys(trajs_u):
    """float64 [n]: path length + smoothness of the float32 trajectories, in float64"""
    t = torch.from_numpy(np.ascontiguousarray(trajs_u)).double()
    return (O.compute_path_length(t) + O.compute_smoothness(t)).numpy()


def pick(x_norm, norm_min, norm_max, gps, num_interpolation, margin, q_min, q_max, paths_all=None, robot0=0, rr_margin=F.MARGIN):
    """x_norm float32 [R B, H, 4] normalised samples, gps: the R robots' GuideParams -> (free bool [R, B], key float64 [R, B] (the counts
    with paths_all, else the cost), idx int32 [R], n_free int32 [R], paths float32 [R, H, 2]: the picks' un-normalised positions)."""
    x_norm = np.asarray(x_norm, np.float32)
    R = len(gps)
    B = x_norm.shape[0] // R
    assert x_norm.shape == (R * B, H, D)
    u = unnormalise(x_norm, norm_min, norm_max)
    free = np.stack([free_flags(u[r * B:(r + 1) * B], gps[r], num_interpolation, margin, q_min, q_max) for r in range(R)])
    if paths_all is not None:
        key = np.stack([collision_counts(u[r * B:(r + 1) * B, :, :2], paths_all, robot0 + r, rr_margin) for r in range(R)])
        idx, n_free, _ = E.expected_pick(free.reshape(-1), B, R, counts=key.reshape(-1))
        key = key.astype(np.float64)
    else:
        key = cost_keys(u).reshape(R, B)
        idx, n_free, _ = E.expected_pick(free.reshape(-1), B, R, cost_a=key.reshape(-1))
    paths = u.reshape(R, B, H, D)[np.arange(R), idx][..., :2].copy()
    return free, key, idx, n_free, paths
