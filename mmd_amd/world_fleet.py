"""World fleets: N robots, each from anywhere to anywhere on a world map, planned together as a receding-horizon loop.

WorldRobotSampler plans many robots at once but wants every robot's start and goal in one window; world_routes takes one robot across
the world alone.  Here the two meet.  Every robot has the exact distance field of its goal over the whole world grid (built once, one
field per distinct goal cell).  An epoch reads every robot's next sub-goal and window off those fields in one launch
(mmd_grid_window_goals, device_window_goals), plans all robots together from their positions to their sub-goals with a
WorldRobotSampler on the windows, and moves the robots to the ends of the returned paths; the loop ends when every robot stands on
its goal.

Where each definition lives.  mmd_amd/fleet_subgoals.py holds the numpy definitions of an epoch's targets and the arguments for them: the
walk, the sub-goal and the window (window_goal; CONTAINMENT, PROGRESS), the walk's support cells and the seed (window_goal_samples,
window_seed), the sub-goals kept apart (subgoals_apart; SEPARATION, APART) and the standing robots that step aside (subgoals_aside;
STEPPING ASIDE, SAFETY).  mmd_amd/fleet_report.py holds the report of a run (run_report, device_run_report; opt-in, nothing here reads
it but WorldFleet.report).  This module holds the launches of the sub-goal kernels, the seeds and the epoch's frames, and the fleet
itself; every public name of the other two is importable from here as well.
"""
import ctypes as C
from collections import namedtuple
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, environments, map_textures, synth
from .fleet_report import (REPORT_HEADER, REPORT_MAX_INTERP, REPORT_MAX_LENGTH, REPORT_MAX_ROBOTS, RunReport, device_run_report,        # noqa: F401
                           device_run_report_words, report_from_words, run_report, segment_lengths, torch_norm2)
from .fleet_report import _order_key                                                    # noqa: F401  (these three private names were
from .fleet_subgoals import _walk, _walks                                               # noqa: F401   reached through this module: they stay reachable)
from .fleet_subgoals import (ASIDE_HELD, ASIDE_MOVED, ASIDE_RELEASED, ASIDE_YIELDS, SUBGOAL_SEPARATION, _checked_aside, _checked_sep,       # noqa: F401
                             _checked_walk_args, epoch_bound, subgoals_apart, subgoals_apart_samples, subgoals_apart_sweeps, subgoals_aside,
                             window_goal, window_goal_samples, window_goals, window_goals_samples, window_seed)
from .multi_agent import ROBOT_RADIUS, RR_MARGIN
from .world import OBSTACLE_MARGIN, WorldRobotSampler
from .world_routes import (ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, SEED_POINTS, UNREACHED, _int32_dev, _points, cell_centres,
                           device_distance_field, world_cells)

_STATUS_NAMES = {ROUTE_OK: "ok", ROUTE_UNREACHED: "unreached", ROUTE_STUCK: "stuck", ROUTE_OUTSIDE: "outside"}


# ---- the definitions' launches on the device ---------------------------------------------------------------------------------------------
def _checked_launch_args(what, dist_dev, reach, max_steps, window):
    """(reach, max_steps, window) as ints, after the checks of dist_dev and of the walk's arguments under the name `what`: the first
    refusals of every sub-goal launch, before anything is uploaded"""
    if dist_dev.dim() != 3 or dist_dev.dtype != torch.int32 or not dist_dev.is_cuda or not dist_dev.is_contiguous():
        raise ValueError(f"{what}: dist must be a contiguous int32 CUDA(HIP) tensor [n_fields, nx, ny]")
    return _checked_walk_args(what, tuple(dist_dev.shape[1:]), reach, max_steps, window)


# the eleven leading arguments of the three sub-goal entry points, in their order (mmd_grid_window_goals_aside takes some of them, by name)
_WalkArgs = namedtuple("_WalkArgs", "dist nx ny n_fields starts fields goals n reach max_steps window")


def _walk_launch_args(what, dist_dev, starts, fields, goals, reach, max_steps, window):
    """(_WalkArgs, the uploaded starts, fields and goals behind three of them: hold them until the launch); reach, max_steps and window are
    _checked_launch_args' """
    starts_dev = _int32_dev(starts, (-1, 2), dist_dev.device, f"{what}: starts")
    n = starts_dev.shape[0]
    fields_dev = _int32_dev(fields, (n,), dist_dev.device, f"{what}: fields")
    goals_dev = _int32_dev(goals, (int(dist_dev.shape[0]), 2), dist_dev.device, f"{what}: goals")
    lead = _WalkArgs(C.c_void_p(dist_dev.data_ptr()), int(dist_dev.shape[1]), int(dist_dev.shape[2]), int(dist_dev.shape[0]),
                     C.c_void_p(starts_dev.data_ptr()), C.c_void_p(fields_dev.data_ptr()), C.c_void_p(goals_dev.data_ptr()), n, reach, max_steps,
                     window)
    return lead, (starts_dev, fields_dev, goals_dev)


_WORDS = (("cells", 2), ("origins", 2), ("summary", 4), ("extra", 2), ("aside", 2))     # the parts of a sub-goal launch's words, [n, width] each
_WORD_STARTS = tuple(sum(width for _, width in _WORDS[:k]) for k in range(len(_WORDS) + 1))       # where part k starts, per query
_PLAIN, _APART, _ASIDE = 3, 4, 5                                                        # the parts that each entry point writes


@lru_cache(maxsize=256)                                      # (a fleet asks for the same few layouts in every epoch)
class _Words:
    """The layout of a sub-goal launch's int32 words for n queries: the first `rows` parts of _WORDS one behind the other, and with
    `with_changed` the one word `changed` behind them.  (The summary rows start 16 n bytes in: aligned as int4.)
    starts: where each part starts, and behind them the index of `changed`, which is the words of the parts; size: the buffer's words"""

    def __init__(self, n, rows, with_changed=False):
        self.n, self.rows, self.with_changed = n, rows, with_changed
        self.starts = [n * k for k in _WORD_STARTS[:rows + 1]]
        self.changed = self.starts[rows]
        self.size = self.changed + int(with_changed)
        self._bytes = [4 * k for k in self.starts[:rows + int(with_changed)]]
        self._parts = [(a, b, width) for a, b, (_, width) in zip(self.starts, self.starts[1:], _WORDS)]

    def pointers(self, words):
        """the address of every part of `words`, a tensor in this layout, and of `changed` where there is one: a launch's output arguments"""
        base = words.data_ptr()
        return [C.c_void_p(base + k) for k in self._bytes]

    def split(self, words):
        """the parts [n, width] as views of `words`, a tensor in this layout or its numpy copy"""
        return tuple(words[a:b].reshape(self.n, width) for a, b, width in self._parts)


def _split_words(words, rows=_PLAIN):
    """(cells [n, 2], origins [n, 2], summary [n, 4][, extra [n, 2][, aside [n, 2]]]): the first `rows` parts of a sub-goal launch's words,
    with or without `changed` behind them, as views; the launch that made the words knows its rows"""
    return _Words(words.shape[0] // _WORD_STARTS[rows], rows).split(words)


def _window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window, with_samples=False, what="device_window_goals"):
    """device_window_goals' launch -> (one int32 tensor [8 n] on the device: cells [n, 2], then origins [n, 2], then summary [n, 4]; None).
    with_samples: device_window_goal_samples' launch (mmd_grid_window_goal_samples) -> (that tensor, samples int32 [n, 64, 2])"""
    lead, _uploads = _walk_launch_args(what, dist_dev, starts, fields, goals, *_checked_launch_args(what, dist_dev, reach, max_steps, window))
    layout = _Words(lead.n, _PLAIN)
    words = torch.empty(layout.size, dtype=torch.int32, device=dist_dev.device)
    if not with_samples:
        _lib.launch("mmd_grid_window_goals", dist_dev, *lead, *layout.pointers(words))
        return words, None
    samples = torch.empty(lead.n, SEED_POINTS, 2, dtype=torch.int32, device=dist_dev.device)
    _lib.launch("mmd_grid_window_goal_samples", dist_dev, *lead, *layout.pointers(words), C.c_void_p(samples.data_ptr()))
    return words, samples


def device_window_goals(dist_dev, starts, fields, goals, reach, max_steps, window=400):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4]) on dist_dev's device: window_goals() for every query in one launch
    (mmd_grid_window_goals), word for word.  dist_dev: any int32 fields [n_fields, nx, ny] (device_distance_field's, or hand-built
    ones); goals [n_fields, 2]: the fields' goal cells.  The three results are views of one tensor."""
    return _split_words(_window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window)[0])


def device_window_goal_samples(dist_dev, starts, fields, goals, reach, max_steps, window=400):
    """(cells, origins, summary, samples int32 [n, 64, 2]) on dist_dev's device: window_goals_samples() for every query in one launch
    (mmd_grid_window_goal_samples), word for word.  The first three are device_window_goals' (views of one tensor); dist_dev: any int32
    fields, as there.  The samples of a query whose status is not ROUTE_OK are zero."""
    words, samples = _window_goals_words(dist_dev, starts, fields, goals, reach, max_steps, window, True, "device_window_goal_samples")
    return _split_words(words) + (samples,)


def device_window_seeds(tex_dev, lo, hi, samples, origins, summary, window, start_points, goal_points, clearance=OBSTACLE_MARGIN,
                        smooth_iters=64, dt=5.0 / 64):
    """(seeds float32 [n, 64, 4], clear_min float32 [n]) on tex_dev's device: window_seed() for every robot in one launch
    (mmd_window_seeds), bit for bit, from device_window_goal_samples' samples [n, 64, 2], origins [n, 2] and summary [n, 4] (or any
    contiguous int32 tensors of those shapes on the texture's device) on any texture [nx, ny, 4] over lo .. hi.  The seeds are global
    points, in trajs_final's format; every row of a robot whose status is not ROUTE_OK is zero, and so is its clear_min."""
    if tex_dev.dim() != 3 or tex_dev.shape[2] != 4:
        raise ValueError(f"device_window_seeds: a texture [nx, ny, 4], got {tuple(tex_dev.shape)}")
    tex_p = _lib.require_gpu(tex_dev, "texture")
    dev = tex_dev.device
    ok = lambda t, shape: (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and t.is_contiguous()      # noqa: E731
                           and tuple(t.shape[1:]) == shape)
    if not (ok(summary, (4,)) and summary.shape[0] >= 1 and ok(samples, (SEED_POINTS, 2)) and ok(origins, (2,))
            and samples.shape[0] == origins.shape[0] == summary.shape[0]):
        raise ValueError("device_window_seeds: samples [n, 64, 2], origins [n, 2] and summary [n, 4], contiguous int32 on the texture's "
                         "device, as device_window_goal_samples returns them")
    n = int(summary.shape[0])
    two_dt = float(np.float32(2.0 * float(dt)))
    if int(smooth_iters) < 0 or not (np.isfinite(two_dt) and two_dt > 0) or int(window) < 1:
        raise ValueError(f"device_window_seeds: smooth_iters = {smooth_iters} (>= 0), dt = {dt} (finite, > 0), window = {window} (>= 1)")
    pts = [torch.as_tensor(p, dtype=torch.float32).reshape(n, 2).contiguous().to(dev) for p in (start_points, goal_points)]
    seeds = torch.empty(n, SEED_POINTS, 4, dtype=torch.float32, device=dev)
    clear_min = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.launch("mmd_window_seeds", tex_dev, tex_p, int(tex_dev.shape[0]), int(tex_dev.shape[1]), (C.c_float * 2)(*map(float, lo)),
                (C.c_float * 2)(*map(float, hi)), float(clearance), C.c_void_p(samples.data_ptr()), C.c_void_p(origins.data_ptr()),
                C.c_void_p(summary.data_ptr()), n, int(window), C.c_void_p(pts[0].data_ptr()), C.c_void_p(pts[1].data_ptr()),
                int(smooth_iters), two_dt, C.c_void_p(seeds.data_ptr()), C.c_void_p(clear_min.data_ptr()))
    return seeds, clear_min


def device_epoch_frames(name, words, points, goal_points, norm_mins=synth.NORM_MINS, norm_maxs=synth.NORM_MAXS, line_a=None):
    """(offsets float32 [n, 2], sub-goal points [n, 2], hard conditions [n, 4] of row 0 and of row 63, straight lines [n, 64, 2]), views
    of one tensor on the words' device: everything a WorldRobotSampler's state takes from an epoch's targets on the world map `name`,
    in one launch (mmd_fleet_epoch_frames) and bit for bit what the host gives -- environments.world_map_window_offsets of the
    origins; world_routes.cell_centres of the cells, or goal_points[r] where summary[r, 3] == 1; the constructor's normalised
    (point - offset, 0, 0) of `points` and of the sub-goal points; synth.straight_line_paths(points, sub-goal points).
    words: int32 [8 n] on the device, a sub-goal launch's (cells, origins, summary) in _split_words' layout -- any words: nothing is
    indexed by them, and nothing is validated (WorldFleet has refused a robot whose status is not ROUTE_OK before this).  points:
    float32 on that device, [n, 2] in rows of any even stride (the last points paths[:, -1] of paths [n, 64, 2] are taken as they
    lie); goal_points float32 [n, 2], contiguous, on that device.  The constants the host definitions compute once are computed
    here by those same expressions; line_a: numpy.linspace(0, 1, 64, dtype=float32) on the device, uploaded here if not given."""
    if not (isinstance(words, torch.Tensor) and words.dtype == torch.int32 and words.is_cuda and words.dim() == 1 and words.is_contiguous()
            and words.shape[0] >= _WORD_STARTS[_PLAIN] and words.shape[0] % _WORD_STARTS[_PLAIN] == 0):
        raise ValueError("device_epoch_frames: words must be a contiguous int32 CUDA(HIP) tensor [8 n], n >= 1, as a sub-goal launch leaves it")
    n, dev = words.shape[0] // _WORD_STARTS[_PLAIN], words.device
    ok = lambda t: isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (n, 2)     # noqa: E731
    if not (ok(points) and points.stride(1) == 1 and points.stride(0) >= 2 and points.stride(0) % 2 == 0
            and points.data_ptr() % 8 == 0 and ok(goal_points) and goal_points.is_contiguous()):
        raise ValueError(f"device_epoch_frames: points (rows of an even stride) and goal_points (contiguous), float32 [{n}, 2] on {dev}")
    if line_a is None:
        line_a = torch.from_numpy(np.linspace(0.0, 1.0, SEED_POINTS, dtype=np.float32)).to(dev)
    lo, hi = (np.asarray(v, np.float32) for v in environments.world_map_limits(name))
    pitch = np.abs(hi - lo) / np.asarray(environments.world_map_occupancy(name).shape[:2], np.float32)        # cell_centres' pitch
    mins, maxs = np.asarray(norm_mins, np.float32), np.asarray(norm_maxs, np.float32)
    out = torch.empty(140 * n, dtype=torch.float32, device=dev)       # offsets 2 n, points 2 n, hard 4 n + 4 n, lines 128 n
    at = lambda k: C.c_void_p(out.data_ptr() + 4 * k)                 # noqa: E731
    _lib.launch("mmd_fleet_epoch_frames", words, *_Words(n, _PLAIN).pointers(words), C.c_void_p(points.data_ptr()), int(points.stride(0)),
                C.c_void_p(goal_points.data_ptr()), n,
                (C.c_double * 5)(environments.SDF_CELL_SIZE, *map(float, environments.world_map_origin(name)), *map(float, environments.LIMITS[0])),
                (C.c_float * 4)(*map(float, lo), *map(float, pitch)), (C.c_float * 4)(*map(float, mins)), (C.c_float * 4)(*map(float, maxs - mins)),
                C.c_void_p(line_a.data_ptr()), at(0), at(2 * n), at(4 * n), at(8 * n), at(12 * n))
    return (out[:2 * n].view(n, 2), out[2 * n:4 * n].view(n, 2), out[4 * n:8 * n].view(n, 4), out[8 * n:12 * n].view(n, 4),
            out[12 * n:].view(n, SEED_POINTS, 2))


def _to_fixed_point(launch, changed, sweeps, cap, what, n):
    """(the last host copy of the words, the sweeps run): launch(restart, n_sweeps) -> the words on the host, first a restart call of
    `sweeps` sweeps, then, while the word at `changed` is not zero, `sweeps` more, `cap` in all at most: the sweeps that always reach the
    fixed point and the one that reads changed == 0"""
    run = min(sweeps, cap)
    host = launch(1, run)
    while host[changed] != 0 and run < cap:
        more = min(sweeps, cap - run)
        host, run = launch(0, more), run + more
    if host[changed] != 0:
        raise RuntimeError(f"{what}: {int(host[changed])} robots still moved in sweep {run} of {n} robots: the workspace was disturbed")
    return host, run


# What _subgoals_apart_words leaves.  Its results: the words int32 [10 n + 1] on the device (cells [n, 2], origins [n, 2], summary [n, 4],
# extra [n, 2], changed [1]), their last copy on the host (numpy), samples int32 [n, 64, 2] on the device or None, the sweeps run.  And what
# the launch that continues from it needs (_subgoals_aside_words): the workspace at its fixed point, its size, the launch's leading
# arguments (_WalkArgs), the uploads behind three of them (kept alive), n.
_ApartState = namedtuple("_ApartState", "words host samples sweeps work work_bytes args uploads n")


def _subgoals_apart_words(dist_dev, starts, fields, goals, reach, max_steps, sep, window, sweeps, with_samples, what="device_subgoals_apart"):
    """device_subgoals_apart's launches -> _ApartState"""
    reach, max_steps, window = _checked_launch_args(what, dist_dev, reach, max_steps, window)
    sep, sweeps = _checked_sep(what, sep), int(sweeps)
    if max_steps > _lib.WINDOW_APART_MAX_STEPS or sweeps < 1:
        raise ValueError(f"{what}: max_steps = {max_steps} (at most {_lib.WINDOW_APART_MAX_STEPS}), sweeps = {sweeps} (at least 1)")
    lead, uploads = _walk_launch_args(what, dist_dev, starts, fields, goals, reach, max_steps, window)
    n, layout = lead.n, _Words(lead.n, _APART, True)
    work_bytes = int(_lib.load().mmd_grid_window_apart_work_bytes(n, max_steps))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dist_dev.device)
    words = torch.empty(layout.size, dtype=torch.int32, device=dist_dev.device)
    samples = torch.empty(n, SEED_POINTS, 2, dtype=torch.int32, device=dist_dev.device) if with_samples else None
    *parts, changed = layout.pointers(words)

    def launch(restart, n_sweeps):
        _lib.launch("mmd_grid_window_goals_apart", dist_dev, *lead, sep, restart, n_sweeps, C.c_void_p(work.data_ptr()), work_bytes, *parts,
                    C.c_void_p(samples.data_ptr()) if with_samples else None, changed)
        return words.cpu().numpy()
    host, run = _to_fixed_point(launch, layout.changed, sweeps, n + 1, what, n)      # n sweeps reach the fixed point, one more reads changed == 0
    return _ApartState(words, host, samples, run, work, work_bytes, lead, uploads, n)


def device_subgoals_apart(dist_dev, starts, fields, goals, reach, max_steps, sep, window=400, sweeps=4, with_samples=False):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4], extra int32 [n, 2][, samples int32 [n, 64, 2]], n_sweeps_run) on
    dist_dev's device: subgoals_apart() (with samples: subgoals_apart_samples()) for every query, word for word, by
    mmd_grid_window_goals_apart: a restart call with `sweeps` sweeps, then, while `changed` is not zero, `sweeps` more, at most n + 1 in
    all, the first call included (n reach the fixed point, the one after reads changed == 0).  No queries at all are refused, as
    device_window_goals refuses them.  Every call ends with one device -> host copy of all words, extra
    and changed, which live in one tensor: the common case costs one copy.  The first four results are views of that tensor."""
    state = _subgoals_apart_words(dist_dev, starts, fields, goals, reach, max_steps, sep, window, sweeps, with_samples)
    return _split_words(state.words, _APART) + ((state.samples,) if with_samples else ()) + (state.sweeps,)


def _subgoals_aside_words(dist_dev, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window, sweeps,
                          what="device_subgoals_aside"):
    """device_subgoals_aside's launches -> (one int32 tensor [12 n + 1] on the device: cells [n, 2], origins [n, 2], summary [n, 4],
    extra [n, 2], aside [n, 2], changed [1]; its last copy on the host, numpy; the sweeps of phase 1; the sweeps run here).  Phase 1 is
    _subgoals_apart_words' loop to its fixed point, whose workspace mmd_grid_window_goals_aside then reads."""
    reach, max_steps, window = _checked_launch_args(what, dist_dev, reach, max_steps, window)
    sep = _checked_sep(what, sep)
    aside_reach, aside_steps = _checked_aside(what, reach, aside_reach, aside_steps)
    phase1 = _subgoals_apart_words(dist_dev, starts, fields, goals, reach, max_steps, sep, window, sweeps, False, what)
    n, lead, layout = phase1.n, phase1.args, _Words(phase1.n, _ASIDE, True)
    work_bytes = int(_lib.load().mmd_grid_window_aside_work_bytes(n))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dist_dev.device)
    words = torch.empty(layout.size, dtype=torch.int32, device=dist_dev.device)

    before = (lead.dist, lead.nx, lead.ny, lead.n_fields, lead.fields, lead.n, lead.reach, lead.max_steps, lead.window, sep, aside_reach, aside_steps)
    behind = (C.c_void_p(phase1.work.data_ptr()), phase1.work_bytes, C.c_void_p(work.data_ptr()), work_bytes, *layout.pointers(words))

    def launch(restart, n_sweeps):
        _lib.launch("mmd_grid_window_goals_aside", dist_dev, *before, restart, n_sweeps, *behind)
        return words.cpu().numpy()
    # 2 n sweeps reach the fixed point, one more reads changed == 0
    host, run = _to_fixed_point(launch, layout.changed, int(sweeps), 2 * n + 1, what, n)
    return words, host, phase1.sweeps, run


def device_subgoals_aside(dist_dev, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window=400, sweeps=4):
    """(cells int32 [n, 2], origins int32 [n, 2], summary int32 [n, 4], extra int32 [n, 2], aside int32 [n, 2], n_sweeps_run) on dist_dev's
    device: subgoals_aside() for every query, word for word.  Phase 1 is device_subgoals_apart's loop; then
    mmd_grid_window_goals_aside on its workspace: a restart call with `sweeps` sweeps, then, while `changed` is not zero, `sweeps` more, at
    most 2 n + 1 in all (2 n reach the fixed point, the one after reads changed == 0); n_sweeps_run counts these, not phase 1's.  Every call
    of either entry point ends with one device -> host copy of all its words.  The five arrays are views of one tensor."""
    words, _, _, run = _subgoals_aside_words(dist_dev, starts, fields, goals, reach, max_steps, sep, aside_reach, aside_steps, window, sweeps)
    return _split_words(words, _ASIDE) + (run,)


# ---- the fleet -----------------------------------------------------------------------------------------------------------------------------
class EpochTargets(NamedTuple):
    """What one epoch plans towards (WorldFleet.epoch_targets): numpy on the host, and the launch's own tensors on the device."""
    cells: np.ndarray           # int32 [N, 2]: the sub-goal cells in the world
    origins: np.ndarray         # int32 [N, 2]: the windows' origin cells
    offsets: np.ndarray         # float32 [N, 2]: the windows' offsets (environments.world_map_window_offsets)
    points: np.ndarray          # float32 [N, 2]: the sub-goal points, global: the cell's centre, or the robot's exact goal once `arrived`
    summary: np.ndarray         # int32 [N, 4]: (steps, remaining, status, arrived)
    samples: torch.Tensor = None    # seed_epochs: int32 [N, 64, 2] on the device, the walks' support cells (never copied back); else None
    words: torch.Tensor = None      # int32 [8 N] on the device, (cells, origins, summary) as launched (_split_words); with separation a view
    extra: np.ndarray = None        # separation: int32 [N, 2] = (walked, clear) of subgoals_apart; else None
    sweeps: int = None              # separation: the sweeps device_subgoals_apart ran; else None
    aside: np.ndarray = None        # step_aside: int32 [N, 2] = (role bits, l) of subgoals_aside; else None


class FleetResult(NamedTuple):
    """What WorldFleet.run returns."""
    paths: torch.Tensor         # float32 [N, E * 64, 2] on the device, global: epoch e's paths are columns [64 e, 64 e + 64)
    arrived: np.ndarray         # bool [N]: the robot stands on its exact goal point
    # per epoch {"conflict_counts", "summary", "offsets"}: the PlanResult's counts, the epoch's targets; with seed_epochs also
    # "clear_min", float32 [N]: the least texel value over each robot's seed points; with separation also "held_back" (int [N]: walked - k),
    # "sweeps" and "stalled" (every k is 0 and some robot is off its goal: every later epoch would repeat this one); with step_aside also
    # "aside" (int32 [N, 2]: role bits, l), "moved_aside", "released" (int: how many robots) and "cycling" (these start cells occurred before)
    epochs: list


class WorldFleet:
    """N robots from global starts to global goals [N, 2] anywhere on the world map `name` (environments.register_world_map), planned
    together epoch by epoch; one process (rank 0 of 1).  The constructor builds, once, the distance field of every distinct goal cell
    over the whole world grid on the resident world texture (device_distance_field, region None): 4 * nx * ny bytes per distinct goal,
    16.8 MB on a 2048-side world.  ValueError names the robot whose start or goal lies outside the world or on a cell that is not
    routable at `clearance`, or whose goal cannot be reached from its start.

    reach, max_steps: window_goal's, in cells; reach <= 199 on the model's 400-cell window.  Further keyword arguments go to every
    epoch's WorldRobotSampler (n_samples, constraint_table, ...).  `positions` (float32 [N, 2], global) are the robots' current points.

    seed_epochs=True: an epoch starts from its walk instead of from noise.  epoch_targets then runs mmd_grid_window_goal_samples in
    place of mmd_grid_window_goals (the same three outputs, and the walks' 64 support cells, which stay on the device); step builds every
    robot's seed trajectory in one mmd_window_seeds launch on the resident world texture -- from the robot's position to its sub-goal
    point, smooth_iters iterations, at the fleet's clearance, inside the robot's window -- and calls the sampler's
    plan_rounds_seeded(trajs_from_global(seeds), paths_local=the seeds' positions, local_rounds=True, n_noising_steps,
    n_denoising_steps): round 0's constraint table is built on the seed paths, not on straight lines through walls, and every round of
    the epoch is a local re-plan.  Such a round runs n_denoising_steps + n_diffusion_steps_without_noise UNet forwards (3 + 1 = 4 with
    the defaults: run_local_inference's q_sample is one launch without a forward, then conditional_sample's loop) where a round from
    noise runs T + 1 (26 at the released T = 25).  An arrived robot has steps = 0: all 64 samples are its goal cell, so its seed
    runs from its goal point to its goal point inside that one cell (the cell's centre in between, drawn towards the goal point by the
    smoothing) with velocities of at most half a cell over 2 dt; that is "held still" as far as a seed goes, and the robot is still
    sampled between its two pinned ends.  With seed_epochs=False (the default) nothing of this runs.

    separation=None (the default): every robot's sub-goal is its walk's end, whatever the others do.  An int >= 1
    (SUBGOAL_SEPARATION = 23 keeps the pinned ends RR_MARGIN apart) keeps every epoch's sub-goals that many cells apart (fleet_subgoals'
    docstring, SEPARATION): the constructor refuses, naming both robots, two start cells or two goal cells closer than that, and
    max_steps above 4095; epoch_targets runs
    device_subgoals_apart (mmd_grid_window_goals_apart: a restart call of 4 sweeps and, while robots still moved, 4 more) in place of
    mmd_grid_window_goals, with seed_epochs with the samples of the shortened walks, so that mmd_window_seeds, unchanged, builds the seeds
    on them; EpochTargets gains `extra` (walked, clear) and `sweeps`, every epoch's dict "held_back" (walked - k per robot), "sweeps" and
    "stalled"; run(max_epochs=None) loops until every robot has arrived or an epoch is stalled (no robot moves, every k is 0: the
    state would repeat for good), which terminates although epoch_bound no longer holds; an explicit max_epochs still caps it.

    step_aside=False (the default): a robot that the separation holds back waits, and a fleet whose robots all wait is stalled.  True
    (needs separation=; refused with seed_epochs=True): a standing robot steps aside for the robots it holds back, into a cell of its
    box of radius aside_reach (at most min(reach, 63)) at most aside_steps (at most 4095) steps away, and the robots it held walk in the
    same epoch (fleet_subgoals' docstring, STEPPING ASIDE: every epoch's pinned ends stay `separation` apart, and a side cell lies in the
    robot's window).  epoch_targets runs device_subgoals_aside's launches in place of device_subgoals_apart's
    (mmd_grid_window_goals_apart to its fixed point, then mmd_grid_window_goals_aside on its workspace: a restart call of 4 sweeps and,
    while the state still moved, 4 more); EpochTargets gains `aside` (role bits, l), every epoch's dict "aside", "moved_aside" and
    "released" (how many robots) and "cycling" (the tuple of the robots' start cells occurred earlier in the run: epoch_targets is a
    function of the cells alone, so the run would repeat for good; run() returns after that epoch).  "stalled" keeps its expression: a
    robot that moved aside has summary[:, 0] = l >= 1, so an epoch with a side step is not stalled; "held_back" keeps its expression too
    and means nothing for a robot that moved aside.  run(max_epochs=None) is refused: no bound on the epochs is proven, so the caller
    states the cap.  persistent=True works as ever, bit for bit: the launch's first 8 N words keep their layout.

    persistent=False (the default): every epoch builds a WorldRobotSampler, a guide and a named window set of its own and releases the
    set afterwards.  persistent=True keeps ONE sampler (own_windows=True), one guide and
    one window set [N, 1, 400, 400, 4] (slice r is robot r's) for the whole run and moves them between epochs on the device
    (_moved_sampler): every result -- paths, conflict counts, summaries, offsets, clear_min -- is the default's bit for bit, with
    seed_epochs and separation as well; only the time and the memory traffic differ.  close() releases the set, and run()
    closes when it returns; a neighbor_slots= smaller than some epoch needs is refused by the sampler's own message, in that epoch.

    The three options share one epoch_targets, one step and one run; each is a branch where its launch, its sampler or its stop rule
    differs.  EpochTargets.words is the sub-goal launch's device words [8 N] under every option (they were None without seed_epochs
    while only the seeded epoch read them; the persistent step reads them as well).

    report(result_or_paths) judges a run afterwards (RunReport; fleet_report's docstring): obstacles at the waypoints and at sampled points
    inside the segments, robot against robot at every column of the whole run, arrival.  Opt-in: nothing above calls it.

    Out of scope here:
      - an arrived robot is sampled like any other, between two ends pinned to its goal point, not held still;
      - the fleet is not sharded over ranks;
      - repair= and replan=, which WorldRobotSampler refuses;
      - with separation= alone a stalled fleet is reported, not resolved; with step_aside=True no liveness is proven (a fleet may still
        stall or cycle), a cycling fleet is reported and not broken (the priorities are the robots' indices and never rotate), and
        seeded epochs are not built (a side step has no support cells); without separation two sub-goals may coincide.
    Whether a seeded epoch resolves conflicts as well as one from noise is not known."""

    def __init__(self, model, name, starts, goals, clearance=OBSTACLE_MARGIN, reach=180, max_steps=360, device="cuda", seed_epochs=False,
                 smooth_iters=64, n_noising_steps=3, n_denoising_steps=3, separation=None, persistent=False, step_aside=False,
                 aside_reach=48, aside_steps=96, **world_robot_sampler_kwargs):
        self.model, self.name, self.device = model, name, environments.resolved_device(device)
        self.persistent, self.step_aside = bool(persistent), bool(step_aside)
        if self.step_aside and separation is None:
            raise ValueError("WorldFleet: step_aside=True needs separation= (robots step aside for robots that the separation holds back)")
        if self.step_aside and seed_epochs:
            raise ValueError("WorldFleet: step_aside=True with seed_epochs=True is not built: a side step has no support cells yet")
        self._sampler = self._points_dev = self._points_host = self._goal_points_dev = self._line_a = self._report_goals_dev = None
        self.separation = None if separation is None else _checked_sep("WorldFleet: separation", separation)
        self.clearance = float(clearance)
        self.seed_epochs = bool(seed_epochs)
        self.smooth_iters, self.n_noising_steps, self.n_denoising_steps = int(smooth_iters), int(n_noising_steps), int(n_denoising_steps)
        if self.smooth_iters < 0 or self.n_noising_steps < 0 or self.n_denoising_steps < 1:
            raise ValueError(f"WorldFleet: smooth_iters = {smooth_iters} (>= 0), n_noising_steps = {n_noising_steps} (>= 0), "
                             f"n_denoising_steps = {n_denoising_steps} (>= 1)")
        self.sampler_kwargs = dict(world_robot_sampler_kwargs)
        for refused in ("rank", "world_size", "group", "env_id"):
            if refused in self.sampler_kwargs:
                raise ValueError(f"WorldFleet: {refused}= is not taken: a fleet runs in one process on the world map it was given")
        self.shape = tuple(environments.world_map_occupancy(name).shape)
        self.window = int(environments.grid_shape()[0])
        self.reach, self.max_steps, _ = _checked_walk_args("WorldFleet", self.shape, reach, max_steps, self.window)
        self.aside_reach, self.aside_steps = (_checked_aside("WorldFleet", self.reach, aside_reach, aside_steps) if self.step_aside
                                              else (aside_reach, aside_steps))
        self.limits = environments.world_map_limits(name)
        s_pts, self.goal_points = _points(starts), _points(goals)
        n = s_pts.shape[0]
        if n == 0 or self.goal_points.shape[0] != n:
            raise ValueError(f"WorldFleet: {n} starts and {self.goal_points.shape[0]} goals (equal and at least 1)")
        s_cells, g_cells = (self._cells(pts, what) for pts, what in ((s_pts, "start"), (self.goal_points, "goal")))
        if self.separation is not None:
            if self.max_steps > _lib.WINDOW_APART_MAX_STEPS:
                raise ValueError(f"WorldFleet: max_steps = {self.max_steps} with separation= (at most {_lib.WINDOW_APART_MAX_STEPS})")
            for what, cells in (("start", s_cells), ("goal", g_cells)):
                d = cells.astype(np.int64)[:, None, :] - cells.astype(np.int64)[None, :, :]
                close = np.argwhere(np.triu((d * d).sum(-1) < self.separation ** 2, 1))
                if close.size:
                    a, b = (int(v) for v in close[0])
                    raise ValueError(f"WorldFleet: the {what} cells of robots {a} and {b} on {name!r}, {cells[a].tolist()} and "
                                     f"{cells[b].tolist()}, are closer than separation = {self.separation} cells")
        self.field_goals, which = np.unique(g_cells, axis=0, return_inverse=True)
        self.fields = which.reshape(-1).astype(np.int32)
        tex = map_textures.device_world_texture(name, self.device)
        self.dist, _ = device_distance_field(tex, self.field_goals, self.clearance)
        # one gather and one copy: is every end routable, and how far is every start from its goal
        both = torch.from_numpy(np.concatenate([s_cells, g_cells]).astype(np.int64)).to(self.device)
        free = tex[both[:, 0], both[:, 1], 0] > np.float32(self.clearance)
        f_dev = torch.from_numpy(self.fields.astype(np.int64)).to(self.device)
        d0 = self.dist[f_dev, both[:n, 0], both[:n, 1]]
        free, d0 = free.cpu().numpy(), d0.cpu().numpy()
        for r in range(n):
            for what, ok, cell in (("start", free[r], s_cells[r]), ("goal", free[n + r], g_cells[r])):
                if not ok:
                    raise ValueError(f"WorldFleet: the {what} of robot {r} on {name!r}, cell {cell.tolist()}, is not routable at clearance "
                                     f"{self.clearance}")
            if d0[r] == UNREACHED:
                raise ValueError(f"WorldFleet: robot {r} on {name!r}: the goal cell {g_cells[r].tolist()} cannot be reached from the start "
                                 f"cell {s_cells[r].tolist()} at clearance {self.clearance}")
        self._fields_dev = f_dev.to(torch.int32)             # an epoch's launch uploads the robots' cells only
        self._goals_dev = torch.from_numpy(self.field_goals.astype(np.int32)).to(self.device)
        self.n_robots = n
        self.start_distances = d0.astype(np.int64)
        self.positions = s_pts.copy()
        self.last_clear_min = None

    def _cells(self, points, what):
        """world_cells of the robots' points, with its refusal (a point that is not finite or lies outside the world) naming the robot"""
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(~((points >= np.asarray(self.limits[0], np.float32)) & (points <= np.asarray(self.limits[1], np.float32))).all(1))
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"WorldFleet: the {what} of robot {k}, {points[k].tolist()}, lies outside the world map {self.name!r}, "
                             f"{self.limits[0]} .. {self.limits[1]}")
        return world_cells(self.name, points)

    def epoch_bound(self):
        """The epochs that bring every robot from its START onto its goal, at most (epoch_bound over the fields; at least 1: the epoch
        that moves a robot from its start point to its goal point inside one cell)"""
        return max(1, max(epoch_bound(d, self.reach, self.max_steps) for d in self.start_distances.tolist()))

    def _subgoal_words(self, c0):
        """(words on the device, their copy on the host, samples or None, sweeps or None, the rows of the words): the epoch's sub-goal
        launches from the robots' cells c0 under the fleet's options, each with its device -> host copies"""
        walk = (self.dist, c0, self._fields_dev, self._goals_dev, self.reach, self.max_steps)
        if self.separation is None:
            words, samples = _window_goals_words(*walk, self.window, self.seed_epochs)
            return words, words.cpu().numpy(), samples, None, _PLAIN
        if self.step_aside:
            words, host, sweeps, _ = _subgoals_aside_words(*walk, self.separation, self.aside_reach, self.aside_steps, self.window, 4, "WorldFleet")
            return words, host, None, sweeps, _ASIDE
        state = _subgoals_apart_words(*walk, self.separation, self.window, 4, self.seed_epochs, "WorldFleet")
        return state.words, state.host, state.samples, state.sweeps, _APART

    def epoch_targets(self, positions):
        """EpochTargets of the robots at the global points `positions` [N, 2]: one sub-goal launch -- mmd_grid_window_goals; with
        seed_epochs mmd_grid_window_goal_samples, the same words and the samples, which stay on the device; with separation
        device_subgoals_apart's launches (with seed_epochs: with the samples of the shortened walks), whose summary is
        (k, d0 - k, status, arrived) -- and one device -> host copy (with separation: one per call of the entry point).  A robot's cell
        is world_cells' texel of its point; its sub-goal point is the centre of the sub-goal cell by cell_centres' fp32 sequence, or,
        once the sub-goal cell is the goal's (`arrived`), the caller's exact goal point.  Refuses a robot whose status is not ROUTE_OK."""
        pts = _points(positions)
        if pts.shape[0] != self.n_robots:
            raise ValueError(f"WorldFleet.epoch_targets: {pts.shape[0]} positions for {self.n_robots} robots")
        c0 = self._cells(pts, "position")
        words, host, samples, sweeps, rows = self._subgoal_words(c0)
        cells, origins, summary, extra, aside = tuple(a.copy() for a in _split_words(host, rows)) + (None,) * (_ASIDE - rows)
        bad = np.flatnonzero(summary[:, 2] != ROUTE_OK)
        if bad.size:
            r = int(bad[0])
            raise RuntimeError(f"WorldFleet: robot {r} on {self.name!r} at cell {c0[r].tolist()}: sub-goal status "
                               f"{_STATUS_NAMES.get(int(summary[r, 2]), int(summary[r, 2]))}")
        points = np.ascontiguousarray(cell_centres(cells, self.limits[0], self.limits[1], self.shape), dtype=np.float32)
        arrived = summary[:, 3] == 1
        points[arrived] = self.goal_points[arrived]
        return EpochTargets(cells, origins, environments.world_map_window_offsets(self.name, origins), points, summary, samples,
                            words[:_WORD_STARTS[_PLAIN] * self.n_robots], extra, sweeps, aside)

    def _moved_sampler(self, targets):
        """persistent=True: (the fleet's one sampler, moved to the epoch's targets; the robots' points and their sub-goal points [N, 2]
        on the device; the straight lines between them [N, 64, 2]).  One mmd_fleet_epoch_frames launch on the launch's words, the
        robots' points and their goal points, all on the device, and the sampler moved to what it wrote
        (WorldRobotSampler._move_on_device: one mmd_sdf_grid_windows_moved launch, which cuts only the slices whose origin changed).
        The first epoch builds the sampler with own_windows=True first; its windows then do not move.  No sampler, guide or facade is
        built, no texture allocated, no window named, no hard condition, offset or line uploaded.  The robots' points of the next
        epoch are the device slice paths_local[:, -1]; the host copy feeds world_cells and its refusals, as ever."""
        if self._goal_points_dev is None:
            self._goal_points_dev = torch.from_numpy(self.goal_points).to(self.device)
            self._line_a = torch.from_numpy(np.linspace(0.0, 1.0, SEED_POINTS, dtype=np.float32)).to(self.device)
        if self._points_host is not self.positions:          # the first epoch, or positions set by the caller: the only upload of points
            self._points_dev = torch.from_numpy(np.ascontiguousarray(self.positions, dtype=np.float32).reshape(-1, 2)).to(self.device)
        if self._sampler is None:
            self._sampler = WorldRobotSampler(self.model, self.positions, targets.points, targets.offsets, env_id=self.name,
                                              device=self.device, own_windows=True, **self.sampler_kwargs)
        kw = {k: self.sampler_kwargs[k] for k in ("norm_mins", "norm_maxs") if k in self.sampler_kwargs}
        offsets_dev, points_dev, hard_first, hard_last, lines = device_epoch_frames(self.name, targets.words, self._points_dev,
                                                                                   self._goal_points_dev, line_a=self._line_a, **kw)
        self._sampler._move_on_device((self.positions, targets.points), targets.offsets, targets.origins, offsets_dev, hard_first, hard_last,
                                      _split_words(targets.words)[1])
        return self._sampler, self._points_dev, points_dev, lines

    def step(self, seed, max_rounds=8):
        """One epoch: the targets of the current positions; the epoch's sampler from the positions to the sub-goal points -- a fresh
        WorldRobotSampler on named windows, whose map set is released afterwards (map_textures.release_sdf_textures), or, with
        persistent=True, the fleet's one sampler moved in place (_moved_sampler; nothing is released), the same epoch bit for bit --;
        its plan -- plan(max_rounds, seed) on the fresh sampler, plan_rounds from the straight lines the frames launch wrote on the moved
        one, and with seed_epochs plan_rounds_seeded from the epoch's seeds on either (the class's docstring); the seeds' ends are the
        points as they come: host arrays, which device_window_seeds uploads, or the moved sampler's device tensors --; and the robots
        moved to the last points of the returned paths, as they are.  -> (PlanResult, EpochTargets); with seed_epochs `last_clear_min`
        (float32 [N]) holds the seeds' least texel values, from the copy that brings the new positions back."""
        targets = self.epoch_targets(self.positions)
        if self.persistent:
            sampler, starts, goals, lines = self._moved_sampler(targets)
        else:
            starts, goals = self.positions, targets.points
            sampler = WorldRobotSampler(self.model, starts, goals, targets.offsets, env_id=self.name, device=self.device, **self.sampler_kwargs)
        try:
            if self.seed_epochs:
                _, origins_dev, summary_dev = _split_words(targets.words)
                seeds, clear_min = device_window_seeds(map_textures.device_world_texture(self.name, self.device), self.limits[0], self.limits[1],
                                                       targets.samples, origins_dev, summary_dev, self.window, starts, goals, self.clearance,
                                                       self.smooth_iters)
                res = sampler.plan_rounds_seeded(sampler.trajs_from_global(seeds), paths_local=seeds[..., :2].contiguous(),
                                                 local_rounds=True, n_noising_steps=self.n_noising_steps,
                                                 n_denoising_steps=self.n_denoising_steps, max_rounds=max_rounds, seed=seed)
            elif self.persistent:
                res = sampler.plan_rounds(paths_local=lines, max_rounds=max_rounds, seed=seed)
            else:
                res = sampler.plan(max_rounds=max_rounds, seed=seed)
        finally:
            if not self.persistent:
                map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), self.device)
        ends = res.paths_local[:, -1, :]
        if self.seed_epochs:
            back = torch.cat([ends, clear_min[:, None]], dim=1).cpu().numpy()            # one copy: the ends and clear_min
            self.positions, self.last_clear_min = np.ascontiguousarray(back[:, :2], dtype=np.float32), back[:, 2].copy()
        else:
            self.positions = np.ascontiguousarray(ends.cpu().numpy(), dtype=np.float32)
        if self.persistent:
            self._points_dev, self._points_host = ends, self.positions
        return res, targets

    def report(self, result_or_paths, margin=ROBOT_RADIUS, rr_margin=RR_MARGIN, n_interp=3, goal_tol=None, column_conflicts=False):
        """RunReport (device_run_report: two kernels, one copy) of a FleetResult's paths, or of any global paths [N, L, 2] of this fleet's
        robots, on the resident world texture (map_textures.device_world_texture), over the fleet's limits and against its exact goal
        points.  Reads nothing of the sampler: it works after run() has closed it, and changes nothing in the fleet.  margin: the
        least value a point may read without being hit, by default the robot's radius (a value is the distance to the nearest occupied
        cell's edge); goal_tol=None: the world's cell pitch."""
        paths = result_or_paths.paths if isinstance(result_or_paths, FleetResult) else result_or_paths
        paths = torch.as_tensor(paths, dtype=torch.float32).to(self.device).contiguous()
        if paths.dim() != 3 or paths.shape[0] != self.n_robots:
            raise ValueError(f"WorldFleet.report: paths [{self.n_robots}, L, 2], got {tuple(paths.shape)}")
        if self._report_goals_dev is None:
            self._report_goals_dev = torch.from_numpy(self.goal_points).to(self.device)
        return device_run_report(paths, map_textures.device_world_texture(self.name, self.device), self.limits[0], self.limits[1],
                                 self._report_goals_dev, margin, rr_margin, n_interp, goal_tol, column_conflicts)

    def close(self):
        """persistent=True: release the sampler's window set (update_world_map no longer reaches it) and drop the sampler; the next
        step builds another.  Nothing otherwise.  run() closes when it returns, also on an exception."""
        sampler, self._sampler = self._sampler, None
        self._points_dev = self._points_host = None
        if sampler is not None:
            sampler.release_windows()

    def _epoch_record(self, res, targets, stalled, cycling):
        """an epoch's dict in FleetResult.epochs: the keys of every run, then each option's own"""
        record = {"conflict_counts": list(res.conflict_counts), "summary": targets.summary, "offsets": targets.offsets}
        if self.separation is not None:
            record.update(held_back=targets.extra[:, 0] - targets.summary[:, 0], sweeps=targets.sweeps, stalled=stalled)
        if self.step_aside:
            record.update(aside=targets.aside, moved_aside=int(((targets.aside[:, 0] & ASIDE_MOVED) != 0).sum()),
                          released=int(((targets.aside[:, 0] & ASIDE_RELEASED) != 0).sum()), cycling=cycling)
        if self.seed_epochs:
            record["clear_min"] = self.last_clear_min
        return record

    def run(self, max_epochs=None, max_rounds=8, seed=0):
        """Epochs (epoch e with seed + e) until every robot has arrived, at most max_epochs of them (None: epoch_bound(), which suffices
        from the starts).  A robot that has arrived keeps taking part, from its goal point to its goal point, so that the others stay
        constrained by it.  With separation: until every robot has arrived or an epoch is stalled (fleet_subgoals' docstring: one of the two
        comes), at most max_epochs of them if that is given.  -> FleetResult"""
        apart = self.separation is not None
        if max_epochs is None:
            if self.step_aside:
                raise ValueError("WorldFleet.run: step_aside=True needs max_epochs (no bound on the epochs is proven: the caller states the cap)")
            max_epochs = None if apart else self.epoch_bound()
        elif int(max_epochs) < 1:
            raise ValueError(f"WorldFleet.run: max_epochs = {max_epochs} (at least 1)")
        paths, epochs, seen = [], [], set()
        try:
            while True:
                cycling = False
                if self.step_aside:                          # the targets are a function of the robots' cells alone: a repeat repeats for good
                    at = world_cells(self.name, self.positions).tobytes()
                    cycling, _ = at in seen, seen.add(at)
                res, targets = self.step(seed + len(epochs), max_rounds)
                arrived = targets.summary[:, 3] == 1         # the epoch's sub-goal was the goal point: the robot now stands on it
                paths.append(res.paths_local)
                stalled = bool(apart and (targets.summary[:, 0] == 0).all() and not arrived.all())  # no robot moves, one that arrives now included
                epochs.append(self._epoch_record(res, targets, stalled, cycling))
                if arrived.all() or stalled or cycling or (max_epochs is not None and len(epochs) >= int(max_epochs)):
                    return FleetResult(torch.cat(paths, dim=1), arrived, epochs)
        finally:
            self.close()
