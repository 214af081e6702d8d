"""Seeded inputs (numpy PCG64) for the solution statistics: the case families of golden g24 (tools/make_golden_trials.py records the
reference's outputs on them) and larger instances for the GPU tests.  A case is (paths [n, Tg, 4] float32 -- globally padded, global
frame -- and tiles: a list of (agent, t0, offset_x, offset_y, rule))."""
import numpy as np

import fp32_forms
import trial_stats_ref as R

H = 64
FAR = np.array([0.9, 0.9], np.float32)                     # farther than 0.2 / 0.15 from every waypoint / drop-region centre
TRANSFORMS3 = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, -2.0]], np.float32)          # tiles [0,0], [0,1], [1,1]: [col * 2, -row * 2]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def polyline(points, n=H):
    """n float32 points along the polyline through `points`, uniform in arc length."""
    pts = np.asarray(points, np.float64)
    seg = np.linalg.norm(np.diff(pts, axis=0), axis=1)
    s = np.concatenate([[0.0], np.cumsum(seg)])
    u = np.linspace(0.0, s[-1], n)
    return np.stack([np.interp(u, s, pts[:, 0]), np.interp(u, s, pts[:, 1])], 1).astype(np.float32)


def velocities(rng, n):
    """a smooth random velocity column pair [n, 2] float32 (the statistics read it for the acceleration only)."""
    k = np.arange(n)[:, None]
    return (rng.uniform(-1, 1, 2) * np.sin(k / 9.0 + rng.uniform(0, 6, 2)) + 0.05 * rng.standard_normal((n, 2))).astype(np.float32)


# ---- 64-row pieces in a tile's own frame, by rule ------------------------------------------------------------------------------------
def line_pieces(rng):
    out = []
    for sigma in (0.002, 0.02, 0.05, 0.1, 0.2, 0.4):                    # noisy straight lines
        a, b = rng.uniform(-0.9, 0.9, 2), rng.uniform(-0.9, 0.9, 2)
        out.append((polyline([a, b]).astype(np.float64) + sigma * np.linalg.norm(b - a) * rng.standard_normal((H, 2))).astype(np.float32))
    # points at d * (1 +- 4e-7) from the line on both sides: d = 0.1 * length, and d = 0.1 -- the rule compares the distance itself to 0.1
    # (env_empty_2d.py:144-146), so the second family sits on the decision
    for k in range(6):
        a, b = rng.uniform(-0.9, 0.9, 2).astype(np.float32), rng.uniform(-0.9, 0.9, 2).astype(np.float32)
        g = b.astype(np.float64) - a
        length = np.linalg.norm(g)
        normal = np.array([-g[1], g[0]]) / length
        s = rng.uniform(0, 1, H)[:, None]
        side = rng.choice([-1.0, 1.0], H)[:, None]
        d = (0.1 * length if k < 2 else 0.1) * (1 + rng.uniform(-4e-7, 4e-7, H))[:, None]
        p = (a + s * g + side * d * normal).astype(np.float32)
        p[0], p[-1] = a, b
        out.append(p)
    out.append(polyline([[-0.5, 0.25], [0.5, 0.25]]))                    # exactly straight: every cross product is 0
    out.append(polyline([[-0.7, -0.4], [0.6, 0.8]]))
    loop = polyline([[0.3, 0.3], [0.6, -0.2], [-0.4, -0.5], [0.3, 0.3]])  # first point == last point: length 0, NaN, score 0
    loop[-1] = loop[0]
    out.append(loop)
    out.append(np.tile(np.array([[0.25, -0.5]], np.float32), (H, 1)))    # standing still
    return out


def _arc(rng, theta0, dtheta):
    """position vectors whose angle follows theta0 + dtheta (an array of H increments from 0), radius wandering in 0.3 .. 0.8."""
    r = 0.55 + 0.2 * np.sin(np.linspace(0, rng.uniform(2, 6), H) + rng.uniform(0, 6)) + 0.01 * rng.standard_normal(H)
    th = theta0 + dtheta
    return np.stack([r * np.cos(th), r * np.sin(th)], 1).astype(np.float32)


def highways_pieces(rng):
    u = np.linspace(0, 1, H)
    out = []
    for sign in (1.0, -1.0):
        out.append(_arc(rng, rng.uniform(0, 6), sign * 2.5 * u))                                   # counter-clockwise / clockwise arcs
        out.append(_arc(rng, rng.uniform(0, 6), sign * 0.3 * u + 0.01 * rng.standard_normal(H)))
        out.append(_arc(rng, rng.uniform(0, 6), sign * (1.2 * np.sin(np.pi * u * 1.35))))           # S-shaped: out and most of the way back
        out.append(_arc(rng, rng.uniform(0, 6), sign * (0.8 * np.sin(2 * np.pi * u) + 0.4 * u)))
    origin = _arc(rng, 1.0, 2.0 * u)                                                                # a point exactly at the origin: NaN -> 0
    origin[20] = 0.0
    out.append(origin)
    return out


def _visits(rng, waypoints, rows, radius):
    """FAR everywhere except `rows`, which lie at radius * (1 +- 4e-7) (a scalar, or one per waypoint) from the given waypoints."""
    p = np.tile(FAR, (H, 1))
    p[list(rows)] = fp32_forms.near_points(rng, np.asarray(waypoints, np.float32), radius)
    return p


def conveyor_pieces(rng):
    top, bottom = R.CONVEYOR_TOP, R.CONVEYOR_BOTTOM
    out = [polyline([[0.85, 0.2], [-0.85, 0.2]]),                       # top corridor right to left: 1
           polyline([[-0.85, -0.2], [0.85, -0.2]]),                     # bottom corridor left to right: 1
           polyline([[-0.85, 0.2], [0.85, 0.2]]),                       # each in the wrong direction: 0
           polyline([[0.85, -0.2], [-0.85, -0.2]]),
           polyline([[0.6, 0.2], [-0.6, 0.2]]),                         # the first waypoint hit at t = 0
           polyline([[0.0, 0.2], [0.6, 0.2], [0.6, 0.7], [-0.6, 0.7], [-0.6, 0.2]]),      # waypoint 2 before waypoint 1, never again: 0
           polyline([[0.8, 0.25], [0.0, 0.15], [-0.3, -0.6], [-0.6, -0.2], [0.0, -0.25], [0.7, -0.15]])]
    for k in range(8):                                                  # points at 0.2 * (1 +- 4e-7) from the waypoints
        wp = top if k % 2 == 0 else bottom
        rows = sorted(rng.choice(np.arange(H), 3, replace=False))
        radius = np.full(3, 0.2)
        if k >= 2:                                                      # one visit on the decision, the other two well inside
            radius[np.arange(3) != k % 3] = 0.1
        out.append(_visits(rng, wp, rows, radius))
    same_row = _visits(rng, top, [5, 5, 40], 0.2)                       # (a row cannot serve two waypoints; the last assignment stays)
    out.append(same_row)
    return out


def _run(center, first, last, rng, radius=0.1):
    """FAR everywhere except rows first .. last, which lie within `radius` of `center`."""
    p = np.tile(FAR, (H, 1))
    n = last - first + 1
    phi, r = rng.uniform(0, 2 * np.pi, n), radius * np.sqrt(rng.uniform(0, 1, n))
    p[first:last + 1] = (np.asarray(center, np.float64) + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)).astype(np.float32)
    return p


def drop_region_pieces(rng):
    c = R.DROP_REGION_CENTERS
    out = [_run(c[0], 10, 25, rng),            # exactly 16 rows: 1
           _run(c[3], 10, 24, rng),            # exactly 15 rows: 0
           _run(c[8], 48, 63, rng),            # rows 48 .. 63: row 63 is never read, 15 count: 0
           _run(c[15], 47, 62, rng),           # rows 47 .. 62: 1
           _run(c[11], 0, 15, rng),            # the first window
           _run(c[5], 0, 63, rng)]
    split = _run(c[1], 20, 27, rng, 0.04)      # 8 rows at centre 1, then 8 at centre 2 (0.1 apart: within 0.04 of one is within 0.15 of
    split[28:36] = _run(c[2], 28, 35, rng, 0.04)[28:36]                  # the other): a run of 16 for both centres
    out.append(split)
    far_split = _run(c[0], 20, 27, rng)        # 8 rows at centre 0, then 8 at centre 4: no centre has 16
    far_split[28:36] = _run(c[4], 28, 35, rng)[28:36]
    out.append(far_split)
    for k in range(8):                         # 16 rows at 0.15 * (1 +- 4e-7) from a centre
        p = np.tile(FAR, (H, 1))
        first = int(rng.integers(0, 47))
        ck = c[int(rng.integers(0, 16))]
        p[first:first + 16] = _run(ck, first, first + 15, rng, 0.1)[first:first + 16]
        edge = rng.choice(np.arange(first, first + 16), 2 if k % 2 else 1, replace=False)
        p[edge] = fp32_forms.near_points(rng, np.tile(ck, (len(edge), 1)), 0.15)
        out.append(p)
    return out


PIECES = {R.RULE_LINE: line_pieces, R.RULE_HIGHWAYS: highways_pieces, R.RULE_CONVEYOR: conveyor_pieces,
          R.RULE_DROP_REGION: drop_region_pieces}


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def pad_paths(bodies, starts):
    """global_pad_paths (multi_agent_utils.py:120-143) on float32 bodies [L_k, 4]: the first row repeated before s_k, the last after."""
    Tg = max(len(b) + s for b, s in zip(bodies, starts))
    return np.stack([np.concatenate([np.repeat(b[:1], s, 0), b, np.repeat(b[-1:], Tg - len(b) - s, 0)]) for b, s in zip(bodies, starts)])


def _single_rule_case(rule, seed):
    rng = _rng(seed)
    pieces = PIECES[rule](rng)
    paths = np.stack([np.concatenate([p, velocities(rng, H)], 1) for p in pieces]).astype(np.float32)
    return paths, [(a, 0, 0.0, 0.0, rule) for a in range(len(pieces))]


def pairs_case(seed=2405, n=48):
    """margin_pairs at 2.0 * 0.05 as rows of 6 agents (agents 2k, 2k + 1 hold a pair; all other pairs of agents are wherever they fall), with
    stagger-padded heads and tails: repeated rows collide at every repeated t."""
    rng = _rng(seed)
    pa, pb = fp32_forms.margin_pairs(seed, n, margin=np.float32(2.0 * 0.05))
    rows = -(-len(pa) // 3)
    idx = np.arange(rows * 3) % len(pa)
    bodies = []
    for k in range(3):
        for side in (pa, pb):
            bodies.append(np.concatenate([side[idx[k::3]], velocities(rng, rows)], 1).astype(np.float32))
    starts = [0, 0, 3, 3, 7, 7]
    return pad_paths(bodies, starts), []


def multi_tile_case(seed=2406, n_agents=4, stagger=5):
    """n_agents x 3 tiles (transforms TRANSFORMS3), start times k * stagger, Tg = 192 + (n_agents - 1) * stagger; agent a's tile k follows rule
    (a + k) % 4 -- a different rule on every tile of an agent."""
    rng = _rng(seed)
    pools = {rule: PIECES[rule](rng) for rule in PIECES}
    bodies, tiles = [], []
    for a in range(n_agents):
        pos = []
        for k in range(3):
            rule = (a + k) % 4
            piece = pools[rule][int(rng.integers(0, len(pools[rule])))]
            pos.append(piece + TRANSFORMS3[k])
            tiles.append((a, a * stagger + k * H, float(TRANSFORMS3[k][0]), float(TRANSFORMS3[k][1]), rule))
        bodies.append(np.concatenate([np.concatenate(pos), velocities(rng, 3 * H)], 1).astype(np.float32))
    return pad_paths(bodies, [a * stagger for a in range(n_agents)]), tiles


G24_CASES = {
    "line": lambda: _single_rule_case(R.RULE_LINE, 2401),
    "highways": lambda: _single_rule_case(R.RULE_HIGHWAYS, 2402),
    "conveyor": lambda: _single_rule_case(R.RULE_CONVEYOR, 2403),
    "drop_region": lambda: _single_rule_case(R.RULE_DROP_REGION, 2404),
    "pairs": pairs_case,
    "multi_tile": multi_tile_case,
}
RULE_ENV = {R.RULE_LINE: "EnvEmpty2D", R.RULE_HIGHWAYS: "EnvHighways2D", R.RULE_CONVEYOR: "EnvConveyor2D",
            R.RULE_DROP_REGION: "EnvDropRegion2D"}


def scale_case(n_agents, stagger, seed):
    """n_agents x 3 tiles with staggered starts, every rule and piece kind mixed, plus margin pairs planted into rows of random agent pairs
    (never into a row of a highways tile: those inputs keep the sign of their sum decided)."""
    paths, tiles = multi_tile_case(seed, n_agents, stagger)
    rng = _rng(seed + 1)
    pa, pb = fp32_forms.margin_pairs(seed + 2, 4 * n_agents, margin=np.float32(2.0 * 0.05))
    Tg = paths.shape[1]
    keep = np.zeros((n_agents, Tg), bool)
    for agent, t0, _, _, rule in tiles:
        if rule == R.RULE_HIGHWAYS:
            keep[agent, t0:t0 + H] = True
    k = 0
    while k < len(pa):
        i, j = rng.choice(n_agents, 2, replace=False)
        t = int(rng.integers(0, Tg))
        if keep[i, t] or keep[j, t]:
            continue
        paths[i, t, :2], paths[j, t, :2] = pa[k], pb[k]
        k += 1
    return paths, tiles
