"""Seeded inputs that put the round's pick (mmd_amd/csrc/round_pick.hip) at its decision edges, as the NORMALISED samples the kernels take.
An edge in un-normalised space is approached from normalised space: for a target value u a ladder of float32 neighbours of the normalised
value, stepped in ulps of v + 1 (near v = 0 a step in ulps of v does not move (v + 1) / 2 * (max - min) + min at all), un-normalised on the
host by tests/round_pick_model.py, which then decides.  An expectation is always the model's verdict on the values the kernel will see,
never a verdict on the intended u.  Host only; tests/test_round_pick_cases_host.py asserts on the model alone that every family reaches its
edge, tests/test_gpu_round_pick_edges.py runs the kernels on the same cases."""
import dataclasses

import numpy as np
import torch

import cases
import fp32_forms as F
import post_edge_cases as E
import round_pick_model as M
from mmd_amd import synth
from oracle import mmd_oracle as O

H, D = 64, 4
STEPS = np.arange(-4, 5)                                   # a ladder's rungs, in ulps of v + 1
WIDE_STEPS = np.array([-8, -4, -2, -1, 0, 1, 2, 4, 8])     # where the edge may lie up to 8 ulps from the target (segment ends, a 2-D distance)
NORM_MIN, NORM_MAX = synth.NORM_MINS, synth.NORM_MAXS
WIDE_MIN = np.array([-1.25, -1.25, -1.5, -1.5], np.float32)      # +-1 (the joint limits) and +-1.03 (the walls at the robot radius) interior
WIDE_MAX = np.array([1.25, 1.25, 1.5, 1.5], np.float32)
EMPTY = "EnvEmpty2D"
SEGMENTS = (0, 31, 62)                                    # the segments (support points s, s + 1) an edge is embedded at
COST_GAP = 2 * (H + 2) * E.U24                            # the two smallest candidate keys differ by more than this times the larger


def far_paths(n):
    """float32 [n, H, 2]: paths no sample comes near (outside the workspace), every robot its own"""
    p = np.zeros((n, H, 2), np.float32)
    p[..., 0] = 3.0 + np.arange(n, dtype=np.float32)[:, None]
    p[..., 1] = 3.0
    return p


@dataclasses.dataclass
class Case:
    """One call of mmd_round_pick_paths: x float32 [R B, H, 4] normalised, robot r on map maps[r].  ladders int [L, K]: the samples of
    every ladder (None: no edge family); note: what a builder records of its design (family d: `planted`, the (path row, step) per
    sample, -1 where none; family f: the free flags, ties and counts it built)."""
    name: str
    x: np.ndarray
    maps: tuple
    norm_min: np.ndarray = NORM_MIN
    norm_max: np.ndarray = NORM_MAX
    ni: int = 5
    margin: float = 0.05
    q_min: tuple = (-1.0, -1.0)
    q_max: tuple = (1.0, 1.0)
    paths_all: np.ndarray = None
    robot0: int = 0
    rr_margin: float = float(F.MARGIN)
    extra: dict = None
    ladders: np.ndarray = None
    note: dict = dataclasses.field(default_factory=dict)

    @property
    def R(self):
        return len(self.maps)

    @property
    def B(self):
        return self.x.shape[0] // self.R

    @property
    def default_settings(self):
        """whether MultiRobotSampler._pick can express the case: its normaliser, five interpolants, the robot radius, the unit limits"""
        return (self.ni == 5 and np.float32(self.margin) == np.float32(0.05) and np.array_equal(self.norm_min, NORM_MIN) and
                np.array_equal(self.norm_max, NORM_MAX) and tuple(self.q_min) == (-1.0, -1.0) and tuple(self.q_max) == (1.0, 1.0) and
                np.float32(self.rr_margin) == F.MARGIN)


def guide_params(case):
    gps = [cases.guide_params(m) for m in case.maps]
    if case.extra is not None:
        for gp in gps:
            gp.extra_spheres = torch.from_numpy(np.asarray(case.extra["spheres"], np.float32))
            gp.extra_boxes = torch.from_numpy(np.asarray(case.extra["boxes"], np.float32))
    return gps


_MODEL = {}


def model(case):
    """round_pick_model.pick of the case (computed once per name) -> (free, key, idx, n_free, paths)"""
    if case.name not in _MODEL:
        _MODEL[case.name] = M.pick(case.x, case.norm_min, case.norm_max, guide_params(case), case.ni, case.margin, case.q_min, case.q_max,
                                   case.paths_all, case.robot0, case.rr_margin)
    return _MODEL[case.name]


# ---- ladders -----------------------------------------------------------------------------------------------------------------------
def nearest(u, lo, hi):
    """the float32 normalised value nearest to the un-normalised u"""
    return np.float32(2.0 * (np.float64(u) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) - 1.0)


def normalised(u, lo=NORM_MIN, hi=NORM_MAX):
    """float32 [..., 4]: the nearest normalised states of un-normalised ones"""
    return np.stack([nearest(np.asarray(u)[..., d], lo[d], hi[d]) for d in range(D)], -1).astype(np.float32)


def ladder(u, lo, hi, steps=STEPS):
    """float32 [len(steps)]: the normalised neighbours of nearest(u), `steps` ulps of v + 1 away -- or, where v + 1 is so small that its ulp
    is less than the ulp of u itself (u next to the normaliser's minimum), that many ulps of u in normalised units: a rung must move the
    un-normalised value"""
    v0 = nearest(u, lo, hi)
    s = max(np.float64(np.spacing(np.float32(v0 + np.float32(1.0)))),
            np.float64(np.spacing(np.abs(np.float32(u)))) * 2.0 / (np.float64(hi) - np.float64(lo)))
    return (np.float64(v0) + np.asarray(steps, np.float64) * s).astype(np.float32)


def _embedded(base_u, pts_u, axis, rung, at, lo, hi, steps=STEPS):
    """float32 [H, 4] normalised: the constant trajectory at base_u [2] with the points pts_u [m, 2] at support points at .. at + m - 1, their
    coordinate `axis` on rung `rung` of its ladder, the other one at its nearest normalised value; zero velocity"""
    x = np.zeros((H, D), np.float32)
    x[:, 0], x[:, 1] = nearest(base_u[0], lo[0], hi[0]), nearest(base_u[1], lo[1], hi[1])
    for m, p in enumerate(np.asarray(pts_u, np.float64).reshape(-1, 2)):
        o = 1 - axis
        x[at + m, axis] = ladder(p[axis], lo[axis], hi[axis], steps)[rung]
        x[at + m, o] = nearest(p[o], lo[o], hi[o])
    return x


def _ladder_case(name, targets, maps, **kw):
    """targets: [(base_u [2], pts_u [m, 2], axis, first support point)] -> the case with one ladder per target, under the counts rule
    against far paths (every count is 0: the pick is the first free sample, with no cost key near a tie)"""
    steps = kw.pop("steps", STEPS)
    lo, hi = kw.get("norm_min", NORM_MIN), kw.get("norm_max", NORM_MAX)
    x = np.stack([_embedded(b, p, ax, k, at, lo, hi, steps) for (b, p, ax, at) in targets for k in range(len(steps))])
    ladders = np.arange(len(x)).reshape(len(targets), len(steps))
    return Case(name, x, tuple(maps), paths_all=far_paths(len(maps) + 1), ladders=ladders, **kw)


def _free_side(gp, margin, p, axis, step):
    """p moved by `step` along `axis` to the side where the map is free at `margin`"""
    for s in (1.0, -1.0):
        q = np.asarray(p, np.float64).copy()
        q[axis] += s * step
        if not bool(O.compute_collision(torch.from_numpy(q.astype(np.float32)[None]), gp, margin)[0]):
            return q
    raise AssertionError(("no free side", p, axis))


# ---- a. map cell edges ---------------------------------------------------------------------------------------------------------------
def _map_edge_targets(ni, n_each=18, seed=3):
    gp = cases.guide_params(E.MAP)
    margin = gp.robot_radius
    pts, axis = E.cell_edge_points(gp, margin, seed)
    segs = E.cell_edge_segments(gp, margin, seed + 2, n=n_each)
    targets = []
    for n in range(n_each):                                            # a point: a segment of length zero (ni = 0: two support points)
        p, ax = pts[n, 2], int(axis[n])
        targets.append((_free_side(gp, margin, p, ax, E.CELL / 2), [p, p], ax, SEGMENTS[n % 3]))
    for n in range(n_each):                                            # a segment whose ends lie within 8 ulps of the edge
        ax = 0 if np.ptp(segs[n, :, 0]) > 0 else 1
        p = segs[n, 2 * (n % 8):2 * (n % 8) + 2, :2]
        mid = p[0].astype(np.float64)
        mid[ax] = float(E.edge(np.round((mid[ax] - E.LO) / E.CELL)))
        targets.append((_free_side(gp, margin, mid, ax, E.CELL / 2), p, ax, SEGMENTS[(n + 1) % 3]))
    if ni == 0:                                                        # the last support point alone
        for n in range(n_each, n_each + n_each // 2):
            p, ax = pts[n, 2], int(axis[n])
            targets.append((_free_side(gp, margin, p, ax, E.CELL / 2), [p], ax, H - 1))
    return targets


def map_edge_case(ni):
    """num_interpolation ni in {0, 1, 5, 16}: points and segments at cell edges of the map whose two cells decide differently, in an
    otherwise free trajectory (constant at the centre of the free cell) at segment 0, 31 or 62 -- ni = 0: also at support point 63 alone"""
    return _ladder_case(f"map_edge_ni{ni}", _map_edge_targets(ni), (E.MAP,), ni=ni, steps=WIDE_STEPS)


# ---- b. workspace walls --------------------------------------------------------------------------------------------------------------
def wall_case(ni):
    """the four walls at the robot radius (coordinate +-1.03: the wide normaliser, limits +-1.25 so that the wall alone decides)"""
    gp = cases.guide_params(E.MAP)
    pts = E.ws_boundary_points(gp, gp.robot_radius)[2::5]              # the crossing coordinate of each wall
    targets = []
    for w, p in enumerate(pts):
        ax = w // 2
        base = p.astype(np.float64)
        base[ax] -= 0.02 * np.sign(base[ax])
        for at in SEGMENTS:
            targets.append((base, [p, p], ax, at))
        if ni == 0:
            targets.append((base, [p], ax, H - 1))
    return _ladder_case(f"wall_ni{ni}", targets, (E.MAP,), ni=ni, norm_min=WIDE_MIN, norm_max=WIDE_MAX, q_min=(-1.25, -1.25),
                        q_max=(1.25, 1.25))


# ---- c. joint limits -----------------------------------------------------------------------------------------------------------------
def limit_case():
    """support points 0, 31 and 63 around each of the four joint limits +-1, interior to the wide normaliser; margin = -1: neither map nor
    wall decides.  Every ladder holds values on the limit (free: the bounds are included), inside and outside."""
    targets = []
    for ax in (0, 1):
        for sign in (1.0, -1.0):
            for at in (0, 31, H - 1):
                p = np.array([0.3, -0.2])
                p[ax] = sign
                targets.append((np.array([0.3, -0.2]), [p], ax, at))
    return _ladder_case("limits", targets, (E.MAP,), norm_min=WIDE_MIN, norm_max=WIDE_MAX, margin=-1.0)


# ---- d. robot-robot margin -----------------------------------------------------------------------------------------------------------
def margin_case(seed=11):
    """n_all = 7, robot0 = 2, 3 local robots.  F.margin_pairs planted as (a sample's point at step t, row j's point at step t), t in
    {0, 31, 63}: every (row, step) holds one pair's second point, every local robot but row j itself has a ladder around the first.
    Sample 1 of every robot is that robot's own row bit for bit (distance 0 at all 64 steps, never counted); sample 0 is the next local
    robot's row (64 hits from that row alone)."""
    n_all, robot0, R = 7, 2, 3
    steps_t = (0, 31, H - 1)
    pa, pb = F.margin_pairs(seed, 16)                                  # 16 random, 4 axis-aligned, 4 exactly at the margin, 4 coincident
    local = list(range(robot0, robot0 + R))
    slots = [(j, t) for j in range(n_all) if j not in local for t in steps_t] + [(j, t) for j in local for t in steps_t]
    pair_of = list(range(6)) + [16, 17] + [20, 21, 22, 23] + list(range(6, 13)) + [18, 19]      # the exact pairs on rows given as they are
    assert len(slots) == len(pair_of) == 21
    lo, hi = NORM_MIN, NORM_MAX
    paths = far_paths(n_all)
    own = np.zeros((R, H, D), np.float32)                             # every local robot's own sample, normalised
    for r in range(R):
        own[r, :, 0], own[r, :, 1] = nearest(0.9, lo[0], hi[0]), nearest(-0.9 + 0.3 * r, lo[1], hi[1])
    for (j, t), k in zip(slots, pair_of):
        if j in local:
            own[j - robot0, t, :2] = [nearest(pb[k, d], lo[d], hi[d]) for d in (0, 1)]
        else:
            paths[j, t] = pb[k]
    paths[robot0:robot0 + R] = M.unnormalise(own, lo, hi)[..., :2]
    x, ladders, planted = [], [], []
    for r in range(R):
        rows = [own[(r + 1) % R], own[r]]
        tags = [(-1, -1), (-1, -1)]
        ladders.append([])
        base = np.array([-0.9 + 0.3 * r, 0.95])
        for (j, t), k in zip(slots, pair_of):
            if j == robot0 + r:
                continue
            d = pa[k].astype(np.float64) - pb[k].astype(np.float64)
            target = paths[j, t].astype(np.float64) + d               # the pair's difference from the point the row really holds
            ax = 0 if abs(d[0]) >= abs(d[1]) else 1
            ladders[r].append(np.arange(len(WIDE_STEPS)) + len(rows))
            for rung in range(len(WIDE_STEPS)):
                rows.append(_embedded(base, [target], ax, rung, t, lo, hi, WIDE_STEPS))
                tags.append((j, t))
        x.append(np.stack(rows))
        planted.append(tags)
    B = len(x[0])
    assert all(len(v) == B for v in x)
    lad = np.concatenate([np.stack(ladders[r]) + r * B for r in range(R)])
    return Case("rr_margin", np.concatenate(x), (EMPTY,) * R, paths_all=paths, robot0=robot0, ladders=lad,
                note=dict(planted=np.asarray(planted).reshape(R * B, 2)))


def planted_distance(case):
    """float32 [R B]: the torch-form distance of every ladder sample's planted point to its row's point (NaN where nothing is planted)"""
    u = M.unnormalise(case.x, case.norm_min, case.norm_max)
    out = np.full(len(u), np.nan, np.float32)
    for n, (j, t) in enumerate(case.note["planted"]):
        if j >= 0:
            out[n] = F.pos_norm(u[n, t, :2], case.paths_all[j, t])
    return out


# ---- e. the phantom segment from the last support point to the origin ------------------------------------------------------------------
def phantom_cost_case():
    """two free samples under the cost rule: the first ends far from the origin and is the cheaper; with || last point - 0 || added to
    both keys it would be the dearer"""
    w = np.linspace(0, 1, H)[:, None]
    u = np.zeros((2, H, D))
    u[0, :, :2] = np.array([0.7, 0.8]) * (1 - w) + np.array([0.8, 0.8]) * w
    u[1, :, :2] = np.array([0.25, 0.0]) * (1 - w) + np.array([0.05, 0.0]) * w
    return Case("phantom_cost", normalised(u), (EMPTY,))


def phantom_map_case():
    """E.MAP under the cost rule: sample 0 stands still (key 0) at a free point whose straight line to the origin holds interpolated points
    inside an obstacle; sample 1 is a short free line"""
    gp = cases.guide_params(E.MAP)
    c = disc(gp)[0]
    w = np.linspace(0, 1, H)[:, None]
    u = np.zeros((2, H, D))
    u[0, :, :2] = c
    u[1, :, :2] = c * (1 - w) + (c + np.array([0.05, 0.0])) * w
    return Case("phantom_map", normalised(u), (E.MAP,))


# ---- f. pick sizes ---------------------------------------------------------------------------------------------------------------------
PICK_KINDS = ("counts", "cost", "ties", "nan")


def disc(gp):
    """(centre [2], radius, inside [2]): the largest disc of the map that is free at the robot radius (cell centres; 0.02 kept clear), and
    the deepest point inside an obstacle"""
    sdf = gp.sdf_grids[0][0].numpy()
    i, j = np.unravel_index(np.argmax(sdf), sdf.shape)
    a, b = np.unravel_index(np.argmin(sdf), sdf.shape)
    return (np.array([E.centre(i), E.centre(j)], np.float64), float(sdf[i, j]) - gp.robot_radius - 0.02,
            np.array([E.centre(a), E.centre(b)], np.float64))


def _in_disc(rng, c, rho, n):
    phi, r = rng.uniform(0, 2 * np.pi, n), rho * np.sqrt(rng.uniform(0, 1, n))
    return c + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)


def _pick_size_build(kind, B, R, share, attempt):
    rng = np.random.default_rng([PICK_KINDS.index(kind), B, R, int(10 * share), attempt])
    gp = cases.guide_params(E.MAP)
    c, rho, inside = disc(gp)
    n = R * B
    free = np.zeros((R, B), bool)
    for r in range(R):
        free[r, rng.permutation(B)[:B if share == 1.0 else int(np.ceil(share * B))]] = True
    w = np.linspace(0, 1, H)[None, :, None]
    u = np.zeros((n, H, D))
    a, b = _in_disc(rng, c, rho, n), _in_disc(rng, c, rho, n)
    u[..., :2] = a[:, None] * (1 - w) + b[:, None] * w
    u[..., 2:] = rng.normal(0, 0.05, (n, H, 2))
    paths, robot0, note = None, 0, {}
    some = share > 0
    if kind == "counts":
        # the row behind the local robots stands at the disc's centre; a sample stands on a ring around it but for its first `hits` steps
        robot0 = 1
        paths = far_paths(R + 2)
        paths[R + 1] = c.astype(np.float32)
        # the best count: robot 0 at 63 and 64 (either side of the scan's second trip) and 69, robot 1 beyond 63 only, robot 2 at 3 as well
        ties = [[i for i in t if i < B] for t in (((63, 64, 69), (64, 69), (3, 63, 64, 69)) if B > 64 else ((3, 5), (5, 6), (1, 3, 5)))]
        hits = rng.integers(2, 6, (R, B))
        for r in range(R):
            hits[r, ties[r]] = 1
        phi = rng.uniform(0, 2 * np.pi, n)
        u[..., :2] = (c + 0.2 * np.stack([np.cos(phi), np.sin(phi)], 1))[:, None]
        for k in range(n):
            u[k, 2:2 + hits.reshape(-1)[k], :2] = c
        if some:
            for r in range(R):
                free[r, ties[r]] = True
        note = dict(ties=ties[:R], hits=hits)
    elif kind == "ties":
        # the cheapest sample and its copies: robot 0 from index 3 on, the other robots from 64 on where there is one
        ties = []
        for r in range(R):
            first = 64 if r > 0 and B > 65 else min(3, B - 1)
            ties.append(sorted({first} | ({64, 128} & set(range(B)) if B > 64 else {B - 1}) | ({65} if first == 64 else set())))
            u[r * B + first, :, :2] = a[r * B + first] + np.array([1e-3, 0.0]) * w[0]
            u[r * B + first, :, 2:] = 0.0
            if some:
                free[r, ties[r]] = True
        note = dict(ties=ties)
    elif kind == "nan":
        nan_free = sorted({B - 1} | ({64} if B > 64 else set()))                # a NaN in the velocity only: free, with a NaN key
        if some:
            free[:, nan_free] = True
        if B > 1:
            free[:, 1] = False
        note = dict(nan_free=nan_free)
    u[~free.reshape(-1), 0:2, :2] = inside                                        # not free: the first segment inside an obstacle
    x = normalised(u)
    if kind == "ties":
        for r in range(R):
            for i in note["ties"][r][1:]:
                x[r * B + i] = x[r * B + note["ties"][r][0]]                      # bit for bit
    if kind == "nan":
        for r in range(R):
            for i in note["nan_free"]:
                x[r * B + i, 40, 3] = np.nan
            if B > 1:
                x[r * B + 1, 7, 0] = np.nan                                       # a NaN position: never free, a candidate only when none is
    note.update(free=free, share=share)
    return Case(f"pick_{kind}_B{B}_R{R}_s{int(10 * share)}", x, (E.MAP,) * R, paths_all=paths, robot0=robot0, note=note)


def cost_gap_ok(case):
    """the cost-rule gap of a case (None under the counts rule): per robot, every candidate whose key equals the smallest is the picked
    sample bit for bit, and the next larger key k1 exceeds the smallest k0 by more than COST_GAP k1.  A NaN pick needs no gap (a NaN key
    comes before every number, in the first index among NaNs)."""
    if case.paths_all is not None:
        return None
    free, key, idx, _, _ = model(case)
    B = case.B
    bits = case.x.view(np.int32)
    for r in range(case.R):
        cand = np.nonzero(free[r])[0] if free[r].any() else np.arange(B)
        k = key[r, cand]
        if np.isnan(k).any():
            continue
        k0 = k.min()
        if any(not np.array_equal(bits[r * B + i], bits[r * B + idx[r]]) for i in cand[k == k0]):
            return False
        rest = k[k > k0]
        if len(rest) and not rest.min() - k0 > COST_GAP * rest.min():
            return False
    return True


def pick_size_case(kind, B, R, share):
    """B in E.PICK_B, R in (1, 3), free share in (0, 0.1, 1) on E.MAP, the samples not free starting inside an obstacle.  counts: the best
    count shared by several samples, none of them sample 0, two of them either side of index 64; cost; ties: the cheapest sample repeated
    bit for bit (at 64 and 128 where B allows); nan: NaN keys among the free samples and, with none free, among all.  A build whose
    cost rule has no gap (cost_gap_ok) is rebuilt with the next seed."""
    for attempt in range(16):
        case = _pick_size_build(kind, B, R, share, attempt)
        if cost_gap_ok(case) is not False:
            return case
        _MODEL.pop(case.name, None)
    raise AssertionError(("no build with a cost gap", kind, B, R, share))


def pick_size_cases(kind):
    return [pick_size_case(kind, B, R, share) for B in E.PICK_B for R in E.PICK_R for share in E.PICK_SHARES]


# ---- two maps, extra objects -------------------------------------------------------------------------------------------------------------
def two_map_case():
    """3 robots on [E.MAP, EnvConveyor2D, E.MAP], the same samples for all three: ladders at E.MAP's cell edges and straight lines"""
    targets = _map_edge_targets(5, n_each=6, seed=13)
    rng = np.random.default_rng(17)
    lo, hi = NORM_MIN, NORM_MAX
    x = np.stack([_embedded(b, p, ax, k, at, lo, hi, WIDE_STEPS) for (b, p, ax, at) in targets for k in range(len(WIDE_STEPS))])
    ends = rng.uniform(-0.95, 0.95, (40, 2, 1, 2))
    w = np.linspace(0, 1, H)[None, :, None]
    lines = np.zeros((40, H, D), np.float32)
    lines[..., :2] = ends[:, 0] * (1 - w) + ends[:, 1] * w            # (normalised = un-normalised for the positions)
    x = np.concatenate([x, lines])
    return Case("two_maps", np.concatenate([x] * 3), (E.MAP, "EnvConveyor2D", E.MAP), paths_all=far_paths(4))


def extra_object_case():
    """EnvEmpty2D with the extra spheres and boxes of tests/test_gpu_margin.py: points either side of a sphere's margin, of a box's flat
    sides and of its rounded corners, at the robot radius; the fixed map is empty there"""
    from test_gpu_margin import _extra_objects
    spheres, boxes = _extra_objects()
    m = 0.05
    targets = []
    gp = guide_params(Case("", np.zeros((0, H, D), np.float32), (EMPTY,), extra=dict(spheres=spheres, boxes=boxes)))[0]

    def add(p, out, ax):
        p, out = np.asarray(p, np.float64), np.asarray(out, np.float64)
        base = p + 0.02 * out
        if not bool(O.compute_collision(torch.from_numpy(base.astype(np.float32)[None]), gp, m)[0]):      # (no other object in the way)
            targets.append((base, [p, p], ax, SEGMENTS[len(targets) % 3]))

    for cx, cy, r in spheres.astype(np.float64):
        for phi in np.deg2rad([0, 30, 90, 150, 180, 240, 270, 330]):
            d = np.array([np.cos(phi), np.sin(phi)])
            add(np.array([cx, cy]) + (r + m) * d, d, 0 if abs(d[0]) >= abs(d[1]) else 1)
    for cx, cy, sx, sy in boxes.astype(np.float64):
        half = np.array([sx, sy]) / 2
        rad = 0.15 * min(sx, sy)
        inner = half - rad
        for s in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            s = np.asarray(s, np.float64)
            add(np.array([cx, cy]) + s * np.array([half[0] + m, 0.5 * inner[1]]), [s[0], 0], 0)         # a flat side in x
            add(np.array([cx, cy]) + s * np.array([0.5 * inner[0], half[1] + m]), [0, s[1]], 1)         # a flat side in y
            for phi in np.deg2rad([30, 60]):
                d = np.array([np.cos(phi), np.sin(phi)])
                add(np.array([cx, cy]) + s * (inner + (rad + m) * d), s * d, 0 if d[0] >= d[1] else 1)
    return _ladder_case("extra_objects", targets, (EMPTY,), extra=dict(spheres=spheres, boxes=boxes))


# ---- what the host test asserts of a family of ladders ----------------------------------------------------------------------------------
def ladder_stats(verdict, ladders):
    """verdict bool [n] -> (share of the ladders on which both verdicts occur, share of True among the ladders' samples)"""
    v = np.asarray(verdict, bool)[ladders]
    both = v.any(1) & ~v.all(1)
    return float(both.mean()), float(v.mean())
