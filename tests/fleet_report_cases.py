"""Cases of the fleet run report (world_fleet.run_report / mmd_fleet_run_report), shared by the host and the GPU tests: one small texture,
the hand-built cases that put a decision at its edge, seeded random runs, and the report written out as loops over single points.

The world is 48 x 40 cells of 1/16 over (-1.5, -1.25) .. (1.5, 1.25): the pitch, the limits and every cell centre are exact in float32,
and a cell centre leaves half a cell of slack to the texel arithmetic."""
import numpy as np

import fp32_forms
from mmd_amd import environments as E
from mmd_amd import world_fleet as F
from mmd_amd.fleet_report import _order_key

f32 = np.float32
CELL = 0.0625
SHAPE = (48, 40)
LO, HI = (-1.5, -1.25), (1.5, 1.25)
WALL_X = 20                                   # a wall one cell thick: column 20, every row
INT_FIELDS = ("points_hit", "interp_hit", "first_hit", "bad_points", "outside", "arrival", "conflicts")
EXACT_FLOAT_FIELDS = ("clear_min", "max_step", "end_error")
RUN_FIELDS = ("conflict_count", "first_conflict", "robots_hit", "robots_in_conflict", "robots_arrived")

_CACHE = {}


def bitmap():
    occ = np.zeros(SHAPE, np.uint8)
    occ[WALL_X, :] = 1
    occ[30:36, 8:14] = 1                      # a block
    occ[5:8, 30] = 1                          # a short bar
    occ[40, 25] = 1                           # a single cell
    return occ


def texture():
    """float32 [48, 40, 4]: environments.occupancy_sdf_texture of the bitmap, computed once"""
    if "tex" not in _CACHE:
        _CACHE["tex"] = np.ascontiguousarray(E.occupancy_sdf_texture(bitmap(), CELL), dtype=f32)
    return _CACHE["tex"]


def centre(ix, iy):
    """the centre of cell (ix, iy): exact in float32"""
    return f32(LO[0] + (ix + 0.5) * CELL), f32(LO[1] + (iy + 0.5) * CELL)


def cells_of(points):
    ix, iy, _ = E._texel_indices(np.asarray(points, f32).reshape(-1, 2), LO, HI, SHAPE)
    return np.stack([ix, iy], 1)


def hop_case():
    """(paths [1, 4, 2], goals [1, 2]): waypoints at the centres of cells 16, 19, 22, 25 of row 10, three cells apart; the wall (column 20)
    lies between waypoints 1 and 2, and with n_interp = 2 the interior points of segment 1 are the centres of cells 20 and 21"""
    paths = np.asarray([[centre(16, 10), centre(19, 10), centre(22, 10), centre(25, 10)]], f32)
    return paths, paths[:, -1].copy()


def margin_edge_case():
    """(paths [1, 6, 2], goals, value, n_at): a path along column 19, whose cells touch the wall and all hold `value` = half a cell; n_at of
    its waypoints"""
    tex = texture()
    rows = [4, 7, 10, 13, 16, 19]
    paths = np.asarray([[centre(WALL_X - 1, r) for r in rows]], f32)
    value = tex[WALL_X - 1, rows[0], 0]
    assert all(tex[WALL_X - 1, r, 0] == value for r in rows) and value == f32(0.5 * CELL)
    return paths, paths[:, -1].copy(), value, len(rows)


def rr_edge_case():
    """(paths [2, 2, 2], goals, d): two robots d apart at column 0, d in torch.norm's float32 form by the margin tests' host model
    (fp32_forms.pos_norm), and far apart at column 1"""
    pa, pb = np.asarray([0.1, 0.2], f32), np.asarray([0.17, 0.26], f32)
    d = fp32_forms.pos_norm(pa, pb)
    paths = np.asarray([[pa, (0.5, 0.5)], [pb, (-0.5, -0.5)]], f32)
    return paths, paths[:, -1].copy(), f32(d)


def random_case(n, length, seed):
    """(paths float32 [n, length, 2], goals [n, 2]), seeded: random walks with steps of about 2.5 cells from random cells of the world;
    robots in groups of up to four that walk together a little less than the robot-robot margin apart (conflicts, some of them on and
    off along the way); a few percent of the points pushed onto occupied cells, outside the world (near and far) or set to NaN, +inf or
    -inf in one coordinate; a third of the robots end exactly on their goal and stay there for their last columns."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(LO), np.asarray(HI)
    paths = np.empty((n, length, 2), np.float64)
    for r0 in range(0, n, 4):
        walk = rng.uniform(lo * 0.9, hi * 0.9) + np.cumsum(rng.normal(0, 0.11, (length, 2)), 0)
        walk = lo + np.abs(np.mod(walk - lo, 2 * (hi - lo)) - (hi - lo))       # folded back into the world
        for r in range(r0, min(r0 + 4, n)):
            paths[r] = walk + rng.normal(0, 0.06, 2) + rng.normal(0, 0.015, (length, 2))
    paths = paths.astype(f32)
    occupied = np.argwhere(bitmap() != 0)
    kind = rng.uniform(size=(n, length))
    for r, t in np.argwhere(kind < 0.08):
        k = kind[r, t]
        if k < 0.04:
            paths[r, t] = centre(*occupied[rng.integers(len(occupied))])
        elif k < 0.055:
            paths[r, t] = paths[r, t] * f32(1.5) + f32(0.4)
        elif k < 0.065:
            paths[r, t] = (f32(rng.choice([-1e4, 3e6])), paths[r, t, 1])
        else:
            paths[r, t, rng.integers(2)] = f32(rng.choice([np.nan, np.inf, -np.inf]))
    goals = rng.uniform(lo, hi, (n, 2)).astype(f32)
    for r in range(0, n, 3):
        goals[r] = centre(int(rng.integers(SHAPE[0])), int(rng.integers(SHAPE[1])))
        paths[r, max(length - 1 - int(rng.integers(0, 5)), 0):] = goals[r]
        if length > 12:
            paths[r, length // 2] = goals[r]                                       # on the goal once before, and away again
    return paths, goals


def loop_report(paths, tex, lo, hi, goals, margin, rr_margin, n_interp, goal_tol):
    """run_report written out point by point and pair by pair, on the margin tests' host model of the norm (fp32_forms): a dict of its words.
    Slow: for small cases, to hold the vectorised definition to its own text."""
    paths, goals = np.asarray(paths, f32), np.asarray(goals, f32)
    n, length = paths.shape[:2]
    margin, rr_margin, goal_tol = f32(margin), f32(rr_margin), f32(goal_tol)
    lo32, hi32 = np.asarray(lo, f32), np.asarray(hi, f32)

    def value(p):
        ix, iy, _ = E._texel_indices(np.asarray(p, f32).reshape(1, 2), lo, hi, tex.shape[:2])
        return tex[ix[0], iy[0], 0]

    def finite(p):
        return bool(np.isfinite(p).all())

    def norm(a, b):
        with np.errstate(over="ignore", invalid="ignore"):
            return fp32_forms.pos_norm(a, b)

    out = {k: np.zeros(n, np.int64) for k in INT_FIELDS}
    out.update(clear_min=np.full(n, np.inf, f32), max_step=np.zeros(n, f32), end_error=np.zeros(n, f32), lengths=np.zeros((n, length - 1), f32))
    out["first_hit"][:] = -1
    for r in range(n):
        checked = []
        for t in range(length):
            a = paths[r, t]
            if not finite(a):
                out["bad_points"][r] += 1
                continue
            v = value(a)
            checked.append(v)
            seg_hit = bool(v < margin)
            out["points_hit"][r] += seg_hit
            out["outside"][r] += not (lo32[0] <= a[0] <= hi32[0] and lo32[1] <= a[1] <= hi32[1])
            if t + 1 < length and finite(paths[r, t + 1]):
                b = paths[r, t + 1]
                out["lengths"][r, t] = norm(b, a)
                for j in range(1, n_interp + 1):
                    with np.errstate(over="ignore", invalid="ignore"):
                        q = a + (b - a) * (f32(j) / f32(n_interp + 1))
                    if finite(q):
                        v = value(q)
                        checked.append(v)
                        out["interp_hit"][r] += bool(v < margin)
                        seg_hit |= bool(v < margin)
            if seg_hit and out["first_hit"][r] < 0:
                out["first_hit"][r] = t
        if checked:
            keys = _order_key(np.asarray(checked, f32).view(np.int32))
            out["clear_min"][r] = _order_key(np.asarray([keys.min()], np.int32)).view(f32)[0]
        out["max_step"][r] = out["lengths"][r].max()
        c = length
        while c > 0 and finite(paths[r, c - 1]) and norm(paths[r, c - 1], goals[r]) <= goal_tol:
            c -= 1
        out["arrival"][r] = c
        out["end_error"][r] = norm(paths[r, -1], goals[r]) if finite(paths[r, -1]) and finite(goals[r]) else np.nan
    columns, first = np.zeros(length, np.int64), (-1, -1, -1)
    for t in range(length):
        for i in range(n):
            for j in range(i + 1, n):
                if finite(paths[i, t]) and finite(paths[j, t]) and norm(paths[i, t], paths[j, t]) < rr_margin:
                    out["conflicts"][i] += 1
                    out["conflicts"][j] += 1
                    columns[t] += 1
                    if first[0] < 0:
                        first = (t, i, j)
    out.update(column_conflicts=columns, conflict_count=int(columns.sum()), first_conflict=first,
               robots_hit=int((out["points_hit"] + out["interp_hit"] > 0).sum()), robots_in_conflict=int((out["conflicts"] > 0).sum()),
               robots_arrived=int((out["arrival"] < length).sum()))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def assert_reports_equal(got, want, length, what=""):
    """every integer word, clear_min, max_step and end_error bit for bit; the per-run words; column_conflicts where both have them"""
    for k in INT_FIELDS:
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=f"{what} {k}")
        assert getattr(got, k).dtype == np.int32, k
    for k in EXACT_FLOAT_FIELDS:
        np.testing.assert_array_equal(bits(getattr(got, k)), bits(getattr(want, k)), err_msg=f"{what} {k}")
    for k in RUN_FIELDS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))
    if got.column_conflicts is not None and want.column_conflicts is not None:
        np.testing.assert_array_equal(got.column_conflicts, want.column_conflicts, err_msg=f"{what} column_conflicts")
