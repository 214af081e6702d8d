"""NumPy restatement of the statistics of a multi-agent solution (reference scripts/inference/inference_multi_agent.py:285-342): the
four data-adherence rules, the pair-collision count, path length and mean acceleration, and the trial-level bookkeeping.  It is what the
GPU tests compare mmd_solution_stats against at sizes golden g24 does not hold; g24 (tools/make_golden_trials.py, the genuine reference
functions) pins the restatement itself (tests/test_trials_host.py).

fp32 forms (established on the CPU against torch 2.10 on 2e5 random fp32 inputs each, zero mismatches, with fp32_forms.fma_f32):
  * torch.norm / torch.linalg.norm over two components is sqrt(fma(dy, dy, dx * dx)) in every shape the trial code uses: dim=-1 on
    [n, 2], dim=1 keepdim on [64, 2], and the full reduction of a 1-D tensor of 2 (the pair loop's and the conveyor's
    torch.norm(path[t] - q), the line rule's length).  The plain sqrt(dx * dx + dy * dy) mismatches on 8 % of inputs.
  * the line rule's torch.cross(g, p) z-component (g = last - first, p = point - first, z = 0) is fma(g_x, p_y, -(g_y * p_x)); the plain
    g_x p_y - g_y p_x mismatches on 27 %.  torch.norm of (0, 0, z) is exactly |z|.
  * the thresholds 0.1, 0.15, 0.2 and 2.0 * 0.05 are all below their fp32 roundings, so x < c gives the same answer for every fp32 x
    whether c is taken as the double or as its fp32 rounding.
  * the highways rule's products are separate torch ops (a * b, c * d, -), each rounded once, and its v / ||v|| is an IEEE division.
    Only its final torch.sum has an order that cannot be pinned: inputs keep |sum| >= 1e-2 (worst-case fp32 error of 63 terms bounded
    by 1: 63 * 63 * 2^-24 = 2.4e-4) or contain a NaN.
path_length and mean_accel are sums of non-negative fp32 terms that are exact by the first bullet; two summation orders of n such terms
differ by at most 2 (n - 1) 2^-24 relative, so comparisons use SUM_BOUND(Tg) = 2 Tg 2^-24 relative to the reference value."""
import numpy as np

import fp32_forms

H = 64
RULE_LINE, RULE_HIGHWAYS, RULE_CONVEYOR, RULE_DROP_REGION = 0, 1, 2, 3
ENV_RULE = {"EnvEmpty2D": RULE_LINE, "EnvEmptyNoWait2D": RULE_LINE, "EnvHighways2D": RULE_HIGHWAYS, "EnvConveyor2D": RULE_CONVEYOR,
            "EnvDropRegion2D": RULE_DROP_REGION}
COLLISION_DIST = np.float32(2.0 * 0.05)                       # inference_multi_agent.py:291
CONVEYOR_TOP = np.array([[0.6, 0.2], [0.0, 0.2], [-0.6, 0.2]], np.float32)            # env_conveyor_2d.py:170-171
CONVEYOR_BOTTOM = np.array([[-0.6, -0.2], [0.0, -0.2], [0.6, -0.2]], np.float32)
DROP_REGION_CENTERS = np.array([[0.4, 0.75], [0.4, 0.05], [0.4, -0.05], [0.4, -0.75], [-0.4, 0.75], [-0.4, 0.05], [-0.4, -0.05],
                                [-0.4, -0.75], [0.75, 0.4], [0.05, 0.4], [-0.05, 0.4], [-0.75, 0.4], [0.75, -0.4], [0.05, -0.4],
                                [-0.05, -0.4], [-0.75, -0.4]], np.float32)             # env_drop_region_2d.py:80-97


def SUM_BOUND(Tg):
    return 2.0 * Tg * 2.0 ** -24


def _norm_to(p, q):
    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)
    return fp32_forms.torch_norm2(d[..., 0], d[..., 1])


def adherence_line(p):
    """env_empty_2d.py:132-146 on p [64, 2] float32."""
    p = np.asarray(p, np.float32)
    g = p[-1] - p[0]
    length = fp32_forms.torch_norm2(g[0], g[1])
    q = p - p[0]
    z = fp32_forms.fma_f32(np.full(len(p), g[0], np.float32), q[:, 1], -(g[1] * q[:, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.abs(z) / np.float32(length)
        return float(np.float32((dev < np.float32(0.1)).sum()) / np.float32(len(p)))


def highways_sum(p):
    """The aggregate cross product of env_highways_2d.py:255-271 (summed in float64: the order of torch.sum is not pinned)."""
    p = np.asarray(p, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = p / fp32_forms.torch_norm2(p[:, 0], p[:, 1])[:, None]
        a, b = v[:-1, 0] * v[1:, 1], v[:-1, 1] * v[1:, 0]
        return float((a - b).astype(np.float64).sum())


def adherence_highways(p):
    return 1.0 if highways_sum(p) > 0 else 0.0


def _corridor(p, waypoints):
    prev = -1
    for q in waypoints:
        hit = np.nonzero(_norm_to(p, q) < np.float32(0.2))[0]
        hit = hit[hit > prev]
        if hit.size == 0:
            return False
        prev = int(hit[0])
    return True


def adherence_conveyor(p):
    """env_conveyor_2d.py:161-185: greedy in-order visits, at most one waypoint per corridor per time step."""
    return 1.0 if _corridor(p, CONVEYOR_TOP) or _corridor(p, CONVEYOR_BOTTOM) else 0.0


def adherence_drop_region(p):
    """env_drop_region_2d.py:183-196: 16 consecutive rows inside one disc, windows mask[i - 16 : i] for i in range(16, 64)."""
    for c in DROP_REGION_CENTERS:
        inside = _norm_to(p, c) < np.float32(0.15)
        for i in range(16, len(p)):
            if inside[i - 16:i].all():
                return 1.0
    return 0.0


RULES = {RULE_LINE: adherence_line, RULE_HIGHWAYS: adherence_highways, RULE_CONVEYOR: adherence_conveyor,
         RULE_DROP_REGION: adherence_drop_region}


def tile_points(paths, tile):
    """The tile's 64 positions in its own frame (inference_multi_agent.py:310-313); tile = (agent, t0, ox, oy, rule)."""
    agent, t0, ox, oy, _ = tile
    return np.asarray(paths, np.float32)[int(agent), int(t0):int(t0) + H, :2] - np.array([ox, oy], np.float32)


def pair_collisions(paths, dist=COLLISION_DIST):
    """inference_multi_agent.py:288-294: #{(t, i < j): ||p_i(t) - p_j(t)|| < dist} over all rows of the padded paths."""
    p = np.asarray(paths, np.float32)[..., :2]
    n, count = p.shape[0], 0
    for i in range(n - 1):
        count += int((fp32_forms.pos_norm(p[i][None], p[i + 1:]) < np.float32(dist)).sum())
    return count


def path_length(paths):
    """trajectory/metrics.py:13-16 per agent: fp32 terms, summed in float64 and rounded once."""
    p = np.asarray(paths, np.float32)
    d = p[:, 1:, :2] - p[:, :-1, :2]
    return fp32_forms.torch_norm2(d[..., 0], d[..., 1]).astype(np.float64).sum(-1).astype(np.float32)


def mean_accel(paths):
    """trajectory/metrics.py:52-65 per agent: the mean of the Tg - 1 terms ||v_{t+1} - v_t||."""
    p = np.asarray(paths, np.float32)
    d = p[:, 1:, 2:] - p[:, :-1, 2:]
    return (fp32_forms.torch_norm2(d[..., 0], d[..., 1]).astype(np.float64).sum(-1) / (p.shape[1] - 1)).astype(np.float32)


def solution_stats(paths, tiles, dist=COLLISION_DIST):
    """-> dict(pair_collisions int, path_length [n], mean_accel [n], adherence [n_tiles]) of paths [n, Tg, 4], tiles [(agent, t0, ox, oy, rule)]."""
    return dict(pair_collisions=pair_collisions(paths, dist), path_length=path_length(paths), mean_accel=mean_accel(paths),
                adherence=np.array([RULES[int(t[4])](tile_points(paths, t)) for t in tiles], np.float32))


def trial_means(n_agents, tiles, adherence, path_length_a, mean_accel_a):
    """The bookkeeping of inference_multi_agent.py:303-342: the mean over an agent's tiles, then over agents; Python-float sums of the
    per-agent fp32 values divided by N.  -> (data_adherence, path_length_per_agent, mean_path_acceleration_per_agent)."""
    data_adherence = 0.0
    for a in range(n_agents):
        own = [float(adherence[k]) for k, t in enumerate(tiles) if int(t[0]) == a]
        s = 0.0
        for v in own:
            s += v
        data_adherence += s / len(own)
    data_adherence /= n_agents
    pl = ac = 0.0
    for a in range(n_agents):
        pl += float(path_length_a[a])
        ac += float(mean_accel_a[a])
    return data_adherence, pl / n_agents, ac / n_agents
