"""Seeded inputs that put the post-sampling kernels (mmd_amd/csrc/postprocess.hip) at their edges: points and segments a few ulps either
side of an SDF cell edge whose two cells decide differently, points at the workspace boundary and the joint limits, K-block trajectories
whose only offending point sits at a seam between two 64-point blocks, pick cases for mmd_select_best (ties, +inf, NaN), and inputs for the
metrics, the Savitzky-Golay operator, the waypoint variance and the un-normalisation.  Host only: numpy, torch and scipy on the oracle's GuideParams (`gp`); every
expectation comes from the oracle (in the tests) or from a float64 form written here.  tests/test_post_edges_host.py checks on the oracle alone that each
builder really holds both sides of its decision; tests/test_gpu_post_edges.py runs the kernels on them."""
import numpy as np
import torch

H, D = 64, 4
MAP = "EnvHighways2D"
LO, CELL = -1.0, 0.005                    # the 400 x 400 grid of cases.sdf_grid over [-1, 1]^2
ULPS = (-2, -1, 0, 1, 2)
U24 = 2.0 ** -24                          # unit roundoff of fp32


def ulps(x, k):
    """float32 x moved by k units in the last place (k an int or an int array, |k| small), towards +inf for k > 0."""
    x = np.asarray(x, np.float32).copy()
    k = np.broadcast_to(np.asarray(k, np.int64), x.shape)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    for s in range(1, int(np.abs(k).max(initial=0)) + 1):
        x = np.where(k >= s, np.nextafter(x, up), np.where(k <= -s, np.nextafter(x, down), x)).astype(np.float32)
    return x


def edge(i):
    """fp32 coordinate of the edge between cells i - 1 and i."""
    return np.float32(LO + np.asarray(i, np.float64) * CELL)


def centre(j):
    return np.float32(LO + (np.asarray(j, np.float64) + 0.5) * CELL)


def decisions(gp, margin):
    """bool [nx, ny]: the cell's sdf < margin, compared as the oracle compares."""
    return (gp.sdf_grids[0][0] < margin).numpy()


def flip_pairs(gp, margin):
    """Neighbouring cell pairs whose sdf < margin decisions differ -> (axis [P], lower cell index along the axis [P], index along the other
    axis [P], upper_free [P]): axis 0 = the pair (i, j) / (i + 1, j), axis 1 = (i, j) / (i, j + 1).  The edge at coordinate 0 is left out
    (its neighbours in fp32 are denormals)."""
    dec = decisions(gp, margin)
    out = []
    for axis in (0, 1):
        d = dec if axis == 0 else dec.T
        i, j = np.nonzero(d[:-1] != d[1:])
        keep = edge(i + 1) != 0
        i, j = i[keep], j[keep]
        out.append(np.stack([np.full_like(i, axis), i, j, d[i, j].astype(np.int64)], 1))       # lower cell collides <=> upper is free
    p = np.concatenate(out)
    return p[:, 0], p[:, 1], p[:, 2], p[:, 3].astype(bool)


def _place(axis, along, other):
    """[..., 2] points from the coordinate along `axis` and the other coordinate."""
    along, other = np.broadcast_arrays(np.asarray(along, np.float32), np.asarray(other, np.float32))
    a = np.asarray(axis).reshape(np.shape(axis) + (1,) * (along.ndim - np.ndim(axis)))
    return np.stack([np.where(a == 0, along, other), np.where(a == 0, other, along)], -1).astype(np.float32)


def cell_edge_points(gp, margin, seed):
    """-> (points float32 [P, 5, 2], axis [P]): for every flip pair (in a seeded order) the points on the shared edge at -2 .. +2 ulps, the
    other coordinate at the cell centre.  Where (p - lo) / dim * n rounds across the integer decides on which side each of them falls."""
    axis, i, j, _ = flip_pairs(gp, margin)
    order = np.random.default_rng(seed).permutation(len(axis))
    axis, i, j = axis[order], i[order], j[order]
    along = ulps(np.repeat(edge(i + 1)[:, None], len(ULPS), 1), np.asarray(ULPS)[None, :])
    return _place(axis, along, centre(j)[:, None]), axis


def cell_edge_segments(gp, margin, seed, n=400):
    """Trajectories float32 [n, 64, 4] along one flip pair's edge each, every support point within 8 ulps of the edge (the other coordinate at
    the cell centre).  First half: consecutive support points alternate below / above the edge by 1 .. 8 ulps, so the interpolants
    x_p a + x_{p+1} (1 - a) land on both sides.  Second half: every support point 0 .. 8 ulps on the FREE side (from kmin = 0 .. 4 ulps on),
    so the trajectory is free or not by where the index flips and by the rounding of the interpolation."""
    rng = np.random.default_rng(seed)
    axis, i, j, upper_free = flip_pairs(gp, margin)
    pick = rng.integers(0, len(axis), n)
    axis, i, j, upper_free = axis[pick], i[pick], j[pick], upper_free[pick]
    k = rng.integers(1, 9, (n, H)) * np.where((np.arange(H)[None, :] + rng.integers(0, 2, (n, 1))) % 2 == 0, -1, 1)
    kmin = rng.integers(0, 5, (n, 1))
    one_sided = (kmin + rng.integers(0, 9, (n, H)) % (9 - kmin)) * np.where(upper_free, 1, -1)[:, None]
    k = np.where(np.arange(n)[:, None] < n // 2, k, one_sided)
    along = ulps(np.repeat(edge(i + 1)[:, None], H, 1), k)
    trajs = np.zeros((n, H, D), np.float32)
    trajs[..., :2] = _place(axis, along, centre(j)[:, None])
    trajs[..., 2:] = rng.normal(0, 0.3, (n, H, 2))
    return trajs


def free_border_lane(gp, margin, width=12):
    """Index j along the other axis such that the `width` cells next to BOTH borders of each axis are free at `margin` in lane j of that
    axis -> (j for axis 0, i for axis 1)."""
    sdf = gp.sdf_grids[0][0].numpy()
    out = []
    for s in (sdf, sdf.T):
        worst = np.minimum(s[:width].min(0), s[-width:].min(0))
        j = int(np.argmax(worst))
        assert worst[j] > margin, "no lane with free cells at both borders"
        out.append(j)
    return out


def ws_boundary_points(gp, margin):
    """float32 [20, 2]: for each of the four workspace walls the points whose wall distance ws_max - p / p - ws_min is the nearest fp32 to
    `margin` from either side: the crossing coordinate at -2 .. +2 ulps; the other coordinate in a lane whose border cells are free at
    gp.margin, so that the wall alone decides."""
    lanes = free_border_lane(gp, gp.margin)
    m = np.float32(margin)
    pts = []
    for axis in (0, 1):
        hi = np.float32(gp.ws_max[axis]) - m
        lo = np.float32(gp.ws_min[axis]) + m
        for p0 in (hi, lo):
            pts.append(_place(np.full(len(ULPS), axis), ulps(np.full(len(ULPS), p0, np.float32), np.asarray(ULPS)), centre(lanes[axis])))
    return np.concatenate(pts)


def _border_base(gp, axis, sign):
    """A free point 2 cells inside the border `sign` (+1: q_max, -1: q_min) of `axis`, in a lane free at gp.margin."""
    lanes = free_border_lane(gp, gp.margin)
    return _place(np.asarray(axis), np.float32(sign * 0.99), centre(lanes[axis]))


def limit_trajs(gp):
    """-> (trajs float32 [36, 64, 4], free bool [36]): constant trajectories next to a joint limit with ONE support point (0, 31 or 63) put
    exactly on q_min / q_max (free: the bounds are included), 1 ulp inside (free) or 1 ulp outside (not free), in x and in y."""
    trajs, free = [], []
    for axis in (0, 1):
        for sign in (1, -1):
            base = _border_base(gp, axis, sign)
            for p in (0, 31, H - 1):
                for k in (-1, 0, 1):                                   # ulps OUTWARDS
                    t = np.zeros((H, D), np.float32)
                    t[:, :2] = base
                    t[p, axis] = ulps(np.float32(sign), k * sign)
                    trajs.append(t)
                    free.append(k <= 0)
    return np.stack(trajs), np.asarray(free)


def seam_trajs(K, gp):
    """-> (trajs float32 [n, 64 K, 4], free bool [n], segment int [n]) at the seams of the 64-point blocks; `segment` is the segment that
    holds the colliding interpolants, or -1.  In units of a cell, d = the distance from a flip pair's edge into its FREE cell:
      * 'interp' k = 1 .. K - 1: every point at d = 0.5 but p = 64 k - 2 at 0.9, p = 64 k - 1 at -0.05 (inside the colliding cell; a support
        point is not tested for occupancy) and p = 64 k at 0.03: for 1, 5 and 16 interpolants the segment 64 k - 1 -> 64 k (lane 63 of wave
        k - 1, whose neighbour is in the next block) holds colliding points and no other segment does; the free twin has p = 64 k - 1 at 0.5;
      * 'limit' p = 64 k (k = 0 .. K - 1) and p = L - 1: a constant trajectory next to q_max with that support point 1 ulp outside; the free
        twin has it on the limit."""
    L = K * H
    axis, i, j, upper_free = flip_pairs(gp, gp.robot_radius)
    pair = int(np.nonzero(axis == 0)[0][0])
    e, s, y = float(edge(i[pair] + 1)), (1.0 if upper_free[pair] else -1.0), centre(j[pair])
    at = lambda d: np.float32(e + s * d * CELL)                        # noqa: E731
    trajs, free, seg = [], [], []
    for k in range(1, K):
        for twin in (False, True):
            t = np.zeros((L, D), np.float32)
            t[:, 0], t[:, 1] = at(0.5), y
            t[H * k - 2, 0], t[H * k, 0] = at(0.9), at(0.03)
            if not twin:
                t[H * k - 1, 0] = at(-0.05)
            trajs.append(t); free.append(twin); seg.append(-1 if twin else H * k - 1)
    base = _border_base(gp, 0, 1)
    for p in [H * k for k in range(K)] + [L - 1]:
        for twin in (False, True):
            t = np.zeros((L, D), np.float32)
            t[:, :2] = base
            t[p, 0] = np.float32(1.0) if twin else ulps(np.float32(1.0), 1)
            trajs.append(t); free.append(twin); seg.append(-1)
    return np.stack(trajs), np.asarray(free), np.asarray(seg)


# ---- mmd_select_best ---------------------------------------------------------------------------------------------------------------
PICK_B = (1, 7, 64, 65, 129, 200)
PICK_R = (1, 3)
PICK_SHARES = (0.0, 0.1, 1.0)
PICK_KINDS = ("cost_a", "cost_a_plus_b", "counts", "ties", "inf", "all_inf", "nan", "nan_on_non_free")


def expected_pick(free, B, R, cost_a=None, cost_b=None, counts=None):
    """(idx [R], n_free [R], summary [R B + R]) by the host rule: the candidates are the robot's free samples, or all of them when none is
    free; torch.argmin over the candidates' keys (fp32 cost_a + cost_b; a NaN counts as the smallest, the first index wins among equals)
    mapped back to sample indices; in counts mode the first minimum (the strict '<' scan of cbs.py:452)."""
    idx, n_free = [], []
    for r in range(R):
        f = np.asarray(free[r * B:(r + 1) * B]).astype(bool)
        cand = np.nonzero(f)[0] if f.any() else np.arange(B)
        if counts is not None:
            c = np.asarray(counts[r * B:(r + 1) * B])[cand]
            best = 0
            for m in range(1, len(c)):
                if c[m] < c[best]:
                    best = m
        else:
            key = torch.as_tensor(cost_a[r * B:(r + 1) * B]).float()
            if cost_b is not None:
                key = key + torch.as_tensor(cost_b[r * B:(r + 1) * B]).float()
            best = int(torch.argmin(key[torch.from_numpy(cand)]))
        idx.append(int(cand[best]))
        n_free.append(int(f.sum()))
    summary = np.concatenate([np.asarray(free, np.float32) != 0, np.asarray(idx, np.float32)]).astype(np.float32)
    return np.asarray(idx, np.int32), np.asarray(n_free, np.int32), summary


def pick_cases(kind):
    """Every (B, R, free share) case of one key kind -> dicts(B, R, free uint8 [R B], cost_a, cost_b, counts, idx, n_free, summary)."""
    out = []
    for B in PICK_B:
        for R in PICK_R:
            for share in PICK_SHARES:
                rng = np.random.default_rng([PICK_KINDS.index(kind), B, R, int(10 * share)])
                n = R * B
                free = np.zeros(n, np.uint8)
                for r in range(R):
                    nf = B if share == 1.0 else int(np.ceil(share * B))
                    free[r * B + rng.permutation(B)[:nf]] = 1
                a = rng.uniform(0.5, 9.0, n).astype(np.float32)
                b, counts = None, None
                if kind == "cost_a_plus_b":
                    b = rng.uniform(0.5, 9.0, n).astype(np.float32)
                elif kind == "counts":
                    a, counts = None, rng.integers(0, 4, n).astype(np.int32)           # many equal counts: the first one wins
                elif kind == "ties":
                    a = rng.integers(2, 5, n).astype(np.float32)
                    for r in range(R):
                        if B > 64:                                     # the minimum at index 64 (lane 0's second key) tied with index 5
                            a[r * B + 64] = a[r * B + 5] = 1.0
                            free[r * B + 64] = free[r * B + 5] = free[r * B + 5] | free[r * B + 64]
                        if B > 128:                                    # and a third one across the stride
                            a[r * B + 128] = 1.0
                elif kind == "inf":
                    a[rng.random(n) < 0.6] = np.inf
                elif kind == "all_inf":
                    a[:] = np.inf
                elif kind == "nan":
                    a[rng.random(n) < 0.15] = np.nan
                    b = rng.uniform(0.5, 9.0, n).astype(np.float32) if B % 2 else None
                    for r in range(R):                                 # at least one NaN among each robot's candidates
                        f = free[r * B:(r + 1) * B]
                        cand = np.nonzero(f)[0] if f.any() else np.arange(B)
                        a[r * B + cand[rng.integers(0, len(cand))]] = np.nan
                elif kind == "nan_on_non_free":
                    a[free == 0] = np.where(rng.random(int((free == 0).sum())) < 0.5, np.nan, a[free == 0])
                    if (free == 0).any():
                        a[np.nonzero(free == 0)[0][0]] = np.nan
                idx, n_free, summary = expected_pick(free, B, R, a, b, counts)
                out.append(dict(B=B, R=R, share=share, free=free, cost_a=a, cost_b=b, counts=counts, idx=idx, n_free=n_free, summary=summary))
    return out


# ---- path length / smoothness ------------------------------------------------------------------------------------------------------
def metric_trajs(K, seed):
    """float32 [6, 64 K, 4]: three random trajectories, a walk of 1e-4 steps with ONE segment of 1e3 (at the block seam for K > 1), a
    constant trajectory (both metrics exactly 0) and a walk of steps that grow over six decades."""
    rng = np.random.default_rng(seed)
    L = K * H
    t = rng.uniform(-1, 1, (6, L, D))
    steps = rng.normal(0, 1e-4, (L, D))
    steps[H if K > 1 else 31] = 1e3                                    # the segment 63 -> 64 / 30 -> 31
    t[3] = np.cumsum(steps, 0)
    t[4] = rng.uniform(-1, 1, (1, D))
    t[5] = np.cumsum(rng.normal(0, 1, (L, D)) * np.logspace(-4, 2, L)[:, None], 0)
    return t.astype(np.float32)


def metric_reference(trajs):
    """float64 (path length [n], smoothness [n]) of float32 trajectories, and the derived bound per trajectory of each:
    (L + 2) 2^-24 sum ||diff||.  Each fp32 term sqrt(dx dx + dy dy) of exact fp32 differences carries at most 3 roundings' worth of
    relative error (the difference, product / sum, root), and any summation order of L - 1 terms adds at most L - 2 more."""
    x = np.asarray(trajs, np.float64)
    d = np.diff(x, axis=1)
    pl = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2).sum(1)
    sm = np.sqrt(d[..., 2] ** 2 + d[..., 3] ** 2).sum(1)
    c = (x.shape[1] + 2) * U24
    return pl, sm, c * pl, c * sm


# ---- Savitzky-Golay ----------------------------------------------------------------------------------------------------------------
SAVGOL_CONFIGS = ((64, 10, 2), (64, 5, 2), (64, 31, 3), (128, 10, 2), (192, 10, 2))       # (L, window, polynomial order)


def savgol_operator64(L, window, order):
    from scipy.signal import savgol_filter
    return savgol_filter(np.eye(L), window, order, axis=0)


def savgol_trajs(L, seed):
    """float32 [n, L, 4]: random trajectories; for L = 128 two more whose only non-zero support point is p = 63 / p = 64, at the seam."""
    rng = np.random.default_rng(seed)
    t = rng.normal(0, 0.5, (5, L, D)).astype(np.float32)
    if L == 2 * H:
        z = np.zeros((2, L, D), np.float32)
        z[0, H - 1] = (1.0, -0.75, 3.0, 0.3)
        z[1, H] = (-1.0, 0.6, 0.2, -2.0)
        t = np.concatenate([t, z])
    return t


def savgol_reference(trajs, window, order):
    """(scipy.signal.savgol_filter of the float64 copy, the bound per element (2 window + 3) 2^-24 sum_j |S_pj| |v_j|): the rounding of the
    fp32 operator (1) plus at most 2 window + 1 FMAs over the band, rounded up."""
    from scipy.signal import savgol_filter
    x = np.asarray(trajs, np.float64)
    S = np.abs(savgol_operator64(x.shape[1], window, order))
    return savgol_filter(x, window, order, axis=1), (2 * window + 3) * U24 * np.einsum("pj,njd->npd", S, np.abs(x))


# ---- waypoint variance -------------------------------------------------------------------------------------------------------------
VAR_B, VAR_L = (1, 2, 17, 100), (1, 64, 65)


def variance_trajs(B, L, seed, tight=False):
    """float32 [B, L, 4]; tight: near-identical trajectories, spread 1e-6 around 0.5."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (B, L, D))
    if tight:
        t[..., :2] = 0.5 + rng.uniform(-1e-6, 1e-6, (B, L, 2))
    return t.astype(np.float32)


def variance_reference(trajs):
    """float64 compute_variance_waypoints: sum over t of the unbiased variance of ALL B^2 entries of triu(cdist(p_t, p_t), 1)."""
    p = np.asarray(trajs, np.float64)[..., :2].transpose(1, 0, 2)                        # [L, B, 2]
    d = np.sqrt(((p[:, :, None] - p[:, None, :]) ** 2).sum(-1))
    d = np.triu(d, 1).reshape(p.shape[0], -1)
    if d.shape[1] < 2:
        return float("nan")
    return float(d.var(axis=1, ddof=1).sum())


# ---- un-normalisation --------------------------------------------------------------------------------------------------------------
UNNORM_MINS = np.array([-1.0, -1.1, -1.5, -1.7], np.float32)
UNNORM_MAXS = np.array([1.0, 0.9, 1.5, 1.3], np.float32)
WITHIN_EPS, ABOVE = 1.00005, 1.0002       # inside (1, 1 + 1e-4]: stays above the limit unless the tensor is clipped; beyond 1 + 1e-4


def _unnorm_base(shape, seed, n_tensors=1):
    """Values inside [-1, 1] and, in every tensor of the call, elements in (1, 1 + eps] that show whether that tensor was clipped."""
    x = torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32))
    per = shape[1] // n_tensors
    for c in range(n_tensors):
        x[1, c * per, 3, c % 4] = WITHIN_EPS
        x[-1, c * per + per - 1, 60, (c + 1) % 4] = -WITHIN_EPS
    return x


def unnorm_cases():
    """-> [(name, x float32 [steps, n, 64, 4], n_tensors)] for LimitsNormalizer.unnormalize; see each case's comment."""
    nan, inf = float("nan"), float("inf")
    out = []
    for comp in range(4):                                              # the NaN in each component of the float4
        x = _unnorm_base((9, 8, H, D), 200 + comp)
        x[4, 3, 17, comp] = nan
        out.append((f"nan_alone_{comp}", x, 1))                        # nothing out of range
        x = x.clone()
        x[7, 6, 40, (comp + 1) % 4] = ABOVE
        out.append((f"nan_and_above_{comp}", x, 1))                    # x.max() is NaN: NOT clipped, 1.0002 and the NaN stay
    x = _unnorm_base((9, 8, H, D), 210)
    x[0, 0, 0, 0], x[8, 7, 63, 3] = nan, -ABOVE
    out.append(("nan_first_and_below_last", x, 1))
    x = _unnorm_base((9, 16, H, D), 211, 4)
    x[2, 5, 9, 1], x[3, 10, 30, 2] = nan, ABOVE                        # tensor 1 holds the NaN, tensor 2 the 1.0002: only tensor 2 is clipped
    out.append(("nan_and_above_in_different_tensors", x, 4))
    x = x.clone()
    x[6, 11, 1, 0], x[5, 13, 2, 3] = nan, -ABOVE                       # now tensor 2 holds a NaN too and tensor 3 is out of range
    out.append(("nan_joins_the_clipped_tensor", x, 4))
    x = _unnorm_base((9, 8, H, D), 212)
    x[3, 3, 3, 0], x[5, 1, 7, 2] = inf, -inf
    out.append(("infinities", x, 1))                                   # clipped to the limits
    x = x.clone()
    x[8, 0, 0, 1] = nan
    out.append(("infinities_and_nan", x, 1))                           # not clipped: the infinities stay
    return out


def unnorm_chain_case(n_tensors):
    """[27, 320, 64, 4]: 552,960 points, more than the 2048 x 256 of one pass of the range kernel's grid; the ONLY element out of range lies
    in the last 20,000 points."""
    x = _unnorm_base((27, 320, H, D), 220, n_tensors)
    x[26, 319 - 100, 11, 2] = ABOVE                                    # point 552,960 - 101 * 64 + 11
    return x
