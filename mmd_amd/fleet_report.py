"""THE REPORT OF A RUN (run_report, opt-in; nothing in the fleet reads it but WorldFleet.report).  run_report IS the definition of what a whole run's paths [N, L, 2] are
worth against the map (waypoints and n_interp interior points of every segment), against each other (every pair at every column) and
against their goals; mmd_fleet_run_report (csrc/fleet_report.hip) computes the same integers and the same float32 bits into one buffer,
which device_run_report and WorldFleet.report read with one copy.  It samples; it proves nothing between its samples.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, environments
from .multi_agent import RR_MARGIN


# ---- the report of a run: the definition ---------------------------------------------------------------------------------------------------
REPORT_MAX_ROBOTS, REPORT_MAX_LENGTH, REPORT_MAX_INTERP = 4096, 65535, 63       # MMD_FLEET_REPORT_MAX_*
REPORT_HEADER = 8                                                              # MMD_FLEET_REPORT_HEADER: int32 words before the arrays
_INT_WORDS = ("points_hit", "interp_hit", "first_hit", "bad_points", "outside", "arrival")       # the report's arrays behind the conflicts,
_FLOAT_WORDS = ("clear_min", "length", "max_step", "end_error")                                  # in the buffer's order
_NAN_BITS, _INF_BITS = 0x7fc00000, 0x7f800000


class RunReport(NamedTuple):
    """What run_report, device_run_report and WorldFleet.report return: numpy on the host.  Per robot [N]:"""
    points_hit: np.ndarray      # int32: waypoints whose value is < margin
    interp_hit: np.ndarray      # int32: interior points whose value is < margin
    first_hit: np.ndarray       # int32: the least t whose waypoint, or an interior point of segment t, is hit; -1 if none
    bad_points: np.ndarray      # int32: waypoints with a coordinate that is not finite
    outside: np.ndarray         # int32: finite waypoints outside lo .. hi (they read the clamped border texel and still take part)
    arrival: np.ndarray         # int32: the least c with every column t >= c finite and within goal_tol of the goal; L if the last is not
    conflicts: np.ndarray       # int32: the (t, other robot) in collision
    clear_min: np.ndarray       # float32: the least value over all points checked (a NaN beyond the infinity of its sign); +inf if none
    length: np.ndarray          # float32: the sum of the segment lengths
    max_step: np.ndarray        # float32: the longest segment; 0 if there is none
    end_error: np.ndarray       # float32: ||p[L - 1] - goal||; NaN if that point or the goal is bad
    # per run
    conflict_count: int         # the pairs i < j in collision, summed over the columns: half the sum of `conflicts`
    first_conflict: tuple       # (t, i, j), the least t, then i, then j; (-1, -1, -1) if there is none
    robots_hit: int
    robots_in_conflict: int
    robots_arrived: int
    column_conflicts: np.ndarray = None         # int32 [L]: the pairs in collision per column; None unless asked for


def torch_norm2(dx, dy):
    """sqrt(fma(dy, dy, dx * dx)) in float32, csrc/collision_dev.h's torch_norm2 bit for bit: the product dx * dx rounded to float32, the
    fma's exact sum formed in float64 with its error term (TwoSum) and rounded to odd, so that the cast to float32 is the fma's one
    rounding (53 >= 2 * 24 + 2 bits); an infinite or NaN sum stays what it is."""
    dx, dy = np.atleast_1d(np.asarray(dx, np.float32)), np.atleast_1d(np.asarray(dy, np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        c, y = (dx * dx).astype(np.float64), dy.astype(np.float64)
        p = y * y
        s = np.ascontiguousarray(p + c)
        b = s - p
        e = (p - (s - b)) + (c - b)
        odd = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(odd, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return np.sqrt(s.astype(np.float32))


def _order_key(bits):
    """csrc/seed_dev.h's order_key on int32 bits: an int32 that orders like the float (a NaN beyond the infinity of its sign); its own inverse"""
    return bits ^ ((bits >> 31) & 0x7fffffff)


def _checked_report_args(what, n, length, tex_shape, lo, hi, margin, rr_margin, n_interp, goal_tol):
    """(margin, rr_margin, goal_tol as float32, n_interp as int) after the refusals that run_report and device_run_report share; goal_tol
    None: the texture's cell pitch, the larger axis's"""
    f = np.float32
    if len(tex_shape) != 3 or tex_shape[2] != 4:
        raise ValueError(f"{what}: a texture [nx, ny, 4], got {tuple(tex_shape)}")
    if not (1 <= n <= REPORT_MAX_ROBOTS and 2 <= length <= REPORT_MAX_LENGTH):
        raise ValueError(f"{what}: paths [N, L, 2] with N = {n} (1 .. {REPORT_MAX_ROBOTS}) and L = {length} (2 .. {REPORT_MAX_LENGTH})")
    lo, hi = np.asarray(lo, f).reshape(-1), np.asarray(hi, f).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        dim = np.abs(hi - lo)
    if lo.shape != (2,) or hi.shape != (2,) or not (np.isfinite(lo).all() and np.isfinite(dim).all() and (dim > 0).all()):
        raise ValueError(f"{what}: limits {lo.tolist()} .. {hi.tolist()} (two finite points, a non-zero extent per axis)")
    n_interp = int(n_interp)
    if goal_tol is None:
        goal_tol = max(dim[0] / f(tex_shape[0]), dim[1] / f(tex_shape[1]))
    with np.errstate(over="ignore"):
        margin, rr_margin, goal_tol = f(margin), f(rr_margin), f(goal_tol)
    if not (np.isfinite(margin) and np.isfinite(rr_margin) and np.isfinite(goal_tol) and goal_tol >= 0 and 0 <= n_interp <= REPORT_MAX_INTERP):
        raise ValueError(f"{what}: margin = {margin} and rr_margin = {rr_margin} (finite), goal_tol = {goal_tol} (finite, >= 0), "
                         f"n_interp = {n_interp} (0 .. {REPORT_MAX_INTERP})")
    return margin, rr_margin, goal_tol, n_interp


def segment_lengths(paths):
    """float32 [N, L - 1]: torch_norm2(p[t + 1] - p[t]) of paths [N, L, 2], 0 for a segment with a bad end: the terms of run_report's
    `length` and `max_step`"""
    p = np.asarray(paths, np.float32)
    fin = np.isfinite(p).all(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        d = p[:, 1:] - p[:, :-1]
    return np.where(fin[:, 1:] & fin[:, :-1], torch_norm2(d[..., 0].reshape(-1), d[..., 1].reshape(-1)).reshape(d.shape[:2]), np.float32(0))


def run_report(paths, tex, lo, hi, goals, margin, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
    """RunReport of paths float32 [N, L, 2] (global points; N in 1 .. 4096, L in 2 .. 65535) on any texture tex [nx, ny, 4] over lo .. hi,
    with goals float32 [N, 2]: THE DEFINITION of mmd_fleet_run_report's words.

    Every decision is float32, operation by operation.  A texel is environments._texel_indices' (mmd_sdf_grid_lookup's sequence), a value
    channel 0 of the texel, the norm torch_norm2.  A point with a coordinate that is not finite is BAD: it is counted in bad_points and
    takes part in nothing else, nor does a segment with a bad end.  Segment t runs from a = p[t] to b = p[t + 1]; its interior points are
    q_j = a + (b - a) * (float32(j) / float32(n_interp + 1)), j = 1 .. n_interp (n_interp in 0 .. 63): subtract, multiply, add, three
    roundings; an interior point that is not finite (the difference overflowed) is not checked and not counted.  A waypoint or interior
    point is HIT iff its value is < margin (strict; a NaN value is no hit); a pair of robots is in conflict at column t iff both points
    are finite and torch_norm2(p_i[t] - p_j[t]) < rr_margin; a robot stands on its goal at column t iff the point is finite and
    torch_norm2(p[t] - goal) <= goal_tol.  goal_tol=None: the texture's cell pitch (the larger axis's) -- the map resolves positions no
    finer, and a path's end is exact only on worlds whose arithmetic is.  `length` is the float64 sum of segment_lengths' float32 terms,
    rounded to float32; the device adds the same terms in float32 in a fixed order, so `length` alone is equal only within L * 2^-24.

    The paths are taken as given.  In a FleetResult column 64 e + 63 and column 64 (e + 1) are the same instant: the report sees a
    segment of length zero there, and a conflict at that instant counts in both columns.

    What this does NOT prove: a segment is sampled at n_interp points, not swept, so an obstacle thinner than the spacing of the samples
    can lie between two of them; and robot against robot is tested at the waypoints only, not between them."""
    f = np.float32
    p = np.ascontiguousarray(environments._host_array(paths), dtype=f)
    tex = np.ascontiguousarray(environments._host_array(tex), dtype=f)
    if p.ndim != 3 or p.shape[2] != 2:
        raise ValueError(f"run_report: paths [N, L, 2], got {p.shape}")
    n, length = p.shape[:2]
    margin, rr_margin, goal_tol, n_interp = _checked_report_args("run_report", n, length, tex.shape, lo, hi, margin, rr_margin, n_interp, goal_tol)
    g = np.ascontiguousarray(environments._host_array(goals), dtype=f)
    if g.shape != (n, 2):
        raise ValueError(f"run_report: goals [{n}, 2], got {g.shape}")
    lo32, hi32 = np.asarray(lo, f).reshape(2), np.asarray(hi, f).reshape(2)
    key_inf = np.int32(_INF_BITS)

    def values(points, shape):
        ix, iy, _ = environments._texel_indices(points.reshape(-1, 2), lo, hi, tex.shape[:2])
        return np.ascontiguousarray(tex[ix, iy, 0]).reshape(shape)

    def keys(v, taking):
        return np.where(taking, _order_key(v.view(np.int32)), key_inf)

    with np.errstate(over="ignore", invalid="ignore"):
        fin = np.isfinite(p).all(-1)                                             # [N, L]
        val = values(p, (n, length))
        hit = fin & (val < margin)
        outside = fin & ~((p >= lo32) & (p <= hi32)).all(-1)
        clear_key = keys(val, fin).min(1)
        seg = fin[:, :-1] & fin[:, 1:]
        d = p[:, 1:] - p[:, :-1]
        seg_hit, interp_hit = hit.copy(), np.zeros(n, np.int64)
        for j in range(1, n_interp + 1):
            q = p[:, :-1] + d * (f(j) / f(n_interp + 1))
            taking = seg & np.isfinite(q).all(-1)
            qv = values(q, (n, length - 1))
            q_hit = taking & (qv < margin)
            interp_hit += q_hit.sum(1)
            seg_hit[:, :-1] |= q_hit
            clear_key = np.minimum(clear_key, keys(qv, taking).min(1))
        lengths = segment_lengths(p)
        off_goal = ~(fin & (torch_norm2((p[..., 0] - g[:, None, 0]).reshape(-1), (p[..., 1] - g[:, None, 1]).reshape(-1)).reshape(n, length) <= goal_tol))
        last = p[:, -1] - g
        end_error = np.where(fin[:, -1] & np.isfinite(g).all(1), torch_norm2(last[:, 0], last[:, 1]), np.array(_NAN_BITS, np.int32).view(f))
        # robot against robot, a block of columns at a time
        conflicts, columns, first = np.zeros(n, np.int64), np.zeros(length, np.int64), (-1, -1, -1)
        upper = np.triu(np.ones((n, n), bool), 1)
        block = max(1, (1 << 21) // (n * n))
        for t0 in range(0, length if n > 1 else 0, block):
            pt = p[:, t0:t0 + block].transpose(1, 0, 2)                          # [B, N, 2]
            ft = fin[:, t0:t0 + block].T
            dd = pt[:, :, None, :] - pt[:, None, :, :]
            h = (torch_norm2(dd[..., 0].reshape(-1), dd[..., 1].reshape(-1)).reshape(dd.shape[:3]) < rr_margin) & ft[:, :, None] & ft[:, None, :]
            h &= ~np.eye(n, dtype=bool)
            conflicts += h.sum((0, 2))
            pairs = h & upper
            columns[t0:t0 + block] = pairs.sum((1, 2))
            if first[0] < 0 and pairs.any():
                first = tuple(int(v) + (t0 if k == 0 else 0) for k, v in enumerate(np.argwhere(pairs)[0]))
    points_hit = hit.sum(1)
    arrival = np.where(off_goal.any(1), length - off_goal[:, ::-1].argmax(1), 0)
    i32 = lambda a: np.asarray(a).astype(np.int32)                               # noqa: E731
    return RunReport(i32(points_hit), i32(interp_hit), i32(np.where(seg_hit.any(1), seg_hit.argmax(1), -1)), i32((~fin).sum(1)),
                     i32(outside.sum(1)), i32(arrival), i32(conflicts), _order_key(clear_key.astype(np.int32)).view(f),
                     lengths.astype(np.float64).sum(1).astype(f), lengths.max(1).astype(f), end_error.astype(f),
                     int(columns.sum()), first, int((points_hit + interp_hit > 0).sum()), int((conflicts > 0).sum()),
                     int((arrival < length).sum()), i32(columns) if column_conflicts else None)


# ---- the same on the device ----------------------------------------------------------------------------------------------------------------
def device_run_report_words(paths_dev, tex_dev, lo, hi, goals, margin, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
    """mmd_fleet_run_report's launch -> its one buffer, int32 [8 + 11 N (+ L)] on the paths' device, in include/mmd_amd.h's layout
    (report_from_words reads a copy of it).  paths_dev: contiguous float32 [N, L, 2] on a GPU; tex_dev: any texture [nx, ny, 4] on that
    device; goals [N, 2]: a tensor there, or anything on the host, which is uploaded.  Nothing is copied back."""
    what = "device_run_report"
    if not (isinstance(paths_dev, torch.Tensor) and paths_dev.dim() == 3 and paths_dev.shape[2] == 2):
        raise ValueError(f"{what}: paths [N, L, 2], got {tuple(getattr(paths_dev, 'shape', ()))}")
    paths_p = _lib.require_gpu(paths_dev, "paths")
    if not isinstance(tex_dev, torch.Tensor) or tex_dev.device != paths_dev.device:
        raise ValueError(f"{what}: the texture must be a tensor on the paths' device {paths_dev.device}")
    n, length = int(paths_dev.shape[0]), int(paths_dev.shape[1])
    margin, rr_margin, goal_tol, n_interp = _checked_report_args(what, n, length, tuple(tex_dev.shape), lo, hi, margin, rr_margin, n_interp, goal_tol)
    tex_p = _lib.require_gpu(tex_dev, "texture")
    goals_dev = torch.as_tensor(goals, dtype=torch.float32)
    if tuple(goals_dev.shape) != (n, 2):
        raise ValueError(f"{what}: goals [{n}, 2], got {tuple(goals_dev.shape)}")
    goals_dev = goals_dev.contiguous().to(paths_dev.device)
    words = torch.empty(REPORT_HEADER + (len(_INT_WORDS) + 1 + len(_FLOAT_WORDS)) * n + (length if column_conflicts else 0), dtype=torch.int32,
                        device=paths_dev.device)
    _lib.launch("mmd_fleet_run_report", paths_dev, paths_p, n, length, tex_p, int(tex_dev.shape[0]), int(tex_dev.shape[1]),
                (C.c_float * 2)(*map(float, np.asarray(lo, np.float32).reshape(2))), (C.c_float * 2)(*map(float, np.asarray(hi, np.float32).reshape(2))),
                C.c_void_p(goals_dev.data_ptr()), float(margin), float(rr_margin), n_interp, float(goal_tol), int(bool(column_conflicts)),
                C.c_void_p(words.data_ptr()))
    return words


def report_from_words(words, n, length, column_conflicts=False):
    """RunReport of mmd_fleet_run_report's buffer, as a numpy int32 copy on the host"""
    w = np.ascontiguousarray(words, dtype=np.int32)
    n_cols = length if column_conflicts else 0
    if w.shape != (REPORT_HEADER + (len(_INT_WORDS) + 1 + len(_FLOAT_WORDS)) * n + n_cols,):
        raise ValueError(f"report_from_words: {w.shape} words for N = {n}, L = {length}, column_conflicts = {bool(column_conflicts)}")
    count, key = (int(v) for v in w[:4].view(np.uint64))
    first = (-1, -1, -1) if key == 0xFFFFFFFFFFFFFFFF else (key >> 24, (key >> 12) & 0xFFF, key & 0xFFF)
    at = REPORT_HEADER + n + n_cols
    rows = w[at:].reshape(-1, n)
    ints, floats = rows[:len(_INT_WORDS)], rows[len(_INT_WORDS):].view(np.float32)
    return RunReport(*(r.copy() for r in ints), w[REPORT_HEADER:REPORT_HEADER + n].copy(), *(r.copy() for r in floats), count, first,
                     int(w[4]), int(w[5]), int(w[6]), w[REPORT_HEADER + n:at].copy() if column_conflicts else None)


def device_run_report(paths_dev, tex_dev, lo, hi, goals, margin, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
    """run_report() of paths on the device, by mmd_fleet_run_report (two kernels, one buffer) and ONE device -> host copy: every integer,
    clear_min, max_step and end_error bit for bit, `length` within L * 2^-24 (a float32 sum in the device's fixed order).  Any contiguous
    float32 paths [N, L, 2] and any texture [nx, ny, 4] on one GPU; the arguments and their refusals are run_report's."""
    words = device_run_report_words(paths_dev, tex_dev, lo, hi, goals, margin, rr_margin, n_interp, goal_tol, column_conflicts)
    return report_from_words(words.cpu().numpy(), int(paths_dev.shape[0]), int(paths_dev.shape[1]), column_conflicts)
