"""PyTorch-ROCm custom ops over the C ABI (include/mmd_amd.h): `torch.ops.mmd_amd.{unet_forward, guide_steps,
p_sample_loop, ddim_sample, solution_stats, bin_constraints_from_paths, count_collisions_binned, path_conflicts, round_select,
round_constraints_init, round_soft_from_paths, conflict_constraints_append,
framed_constraints_from_paths, fleet_run_report}`.  They take tensors instead of raw pointers, run on torch's CURRENT HIP stream
without any host synchronisation (so they can be captured into a hipGraph with torch.cuda.graph) and register fake
(meta) implementations so that torch.compile / FakeTensor tracing sees their output shapes.  The C header stays the ABI
of record: every op is a thin wrapper over the same entry point the host mirror classes call through ctypes.

Models and guides are opaque device-side objects (an mmd_unet_t handle + schedule tables; the guide's descriptor with its
resident SDF texture and constraint tables).  Ops receive them as integer tokens from `register(obj)`; the registry
holds weak references, so a token dies with its object.
"""
import ctypes as C
import itertools
import weakref
from typing import Tuple

import torch

from . import _lib

_REGISTRY = weakref.WeakValueDictionary()
_NEXT_TOKEN = itertools.count(1)


def register(obj) -> int:
    """Token for a GaussianDiffusionModel / TemporalUnet / GuideManagerTrajectoriesWithVelocity to pass to the ops.
    Tokens come from a process-wide counter and are stored on the object (registering twice returns the same token), so
    a token is never reused: after its object is gone the ops raise "expired token" instead of resolving to whatever
    CPython later allocated at the same address."""
    tok = getattr(obj, "_mmd_amd_op_token", None)
    if tok is None:
        tok = next(_NEXT_TOKEN)
        obj._mmd_amd_op_token = tok
    _REGISTRY[tok] = obj
    return tok


def _get(token, what):
    obj = _REGISTRY.get(int(token))
    if obj is None:
        raise RuntimeError(f"mmd_amd op: unknown or expired {what} token {token}")
    return obj


def _check_traj(x, name="x", rows="n_traj", width=4):
    """x [rows, 64, width]: trajectories [n_traj, 64, 4] or, for _check_traj(paths, "paths", "n_all", 2), best paths [n_all, 64, 2]"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.ndim == 3 and x.shape[1] == 64
            and x.shape[2] == width):
        raise RuntimeError(f"mmd_amd op: {name} must be a contiguous float32 CUDA(HIP) tensor [{rows}, 64, {width}]")


# ---- unet_forward --------------------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::unet_forward", mutates_args=(), device_types="cuda")
def unet_forward(x: torch.Tensor, t: int, n_timesteps: int, unet: int) -> torch.Tensor:
    """eps = TemporalUnet(x, t) (temporal_unet.py:121); `unet` = register(TemporalUnet), table sized n_timesteps."""
    _check_traj(x)
    model = _get(unet, "unet")
    out = torch.empty_like(x)
    ws = model.workspace(x.shape[0], x.device)
    _lib.launch("mmd_unet_forward", x, model.handle(n_timesteps, x.device), x.data_ptr(), int(t), out.data_ptr(), x.shape[0],
                                            ws.data_ptr(), ws.numel())
    return out


@unet_forward.register_fake
def _(x, t, n_timesteps, unet):
    return torch.empty_like(x)


# ---- guide_steps ---------------------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::guide_steps", mutates_args=("x",), device_types="cuda")
def guide_steps(x: torch.Tensor, hard: torch.Tensor, hard_rows: int, n_steps: int, guide: int) -> None:
    """In place: n_steps x { x += guide(x); apply_hard_conditioning } (sample_functions.py:89-107); hard [n_robots, n_rows, 4] + the 64-bit row
    mask as a SIGNED int64 (_lib.signed64(_lib.HARD_ROWS_START_GOAL) for the start / goal pair)."""
    _check_traj(x)
    g = _get(guide, "guide")
    d = g.desc()
    _lib.launch("mmd_guide_steps", x, C.byref(d), x.data_ptr(), _lib.require_gpu(hard, "hard"), int(hard_rows) & 0xFFFFFFFFFFFFFFFF,
                                           g.n_robots, x.shape[0] // g.n_robots, int(n_steps), None)


# ---- p_sample_loop -------------------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::p_sample_loop", mutates_args=("x",), device_types="cuda")
def p_sample_loop(x: torch.Tensor, hard: torch.Tensor, hard_rows: int, model: int, guide: int, n_robots: int,
                  n_steps: int, n_steps_without_noise: int, init_noise: bool, step_noise: torch.Tensor | None, seed: int,
                  n_guide_steps: int, t_start_guide: int, noise_std_extra: float, traj_index_base: int,
                  return_chain: bool) -> torch.Tensor:
    """GaussianDiffusionModel.p_sample_loop (diffusion_model_base.py:162-211) on x [n_traj,64,4] in place (x_T or the warm
    start on entry unless init_noise; the final sample on exit).  model = register(GaussianDiffusionModel); guide =
    register(guide) or 0.  Returns the chain [n_steps + n_steps_without_noise + 1, n_traj, 64, 4] (empty if not
    return_chain)."""
    _check_traj(x)
    m = _get(model, "model")
    g = _get(guide, "guide") if guide else None
    n_total = n_steps + n_steps_without_noise
    s = m._sampler_desc(n_guide_steps, t_start_guide, None, hard_rows, 0, traj_index_base)
    s.noise_std_extra, s.noise_std_extra_by_t = float(noise_std_extra), None
    gd = g.desc() if g is not None else None
    chain = (torch.empty((n_total + 1,) + tuple(x.shape), dtype=torch.float32, device=x.device) if return_chain
             else torch.empty(0, dtype=torch.float32, device=x.device))
    if step_noise is not None and tuple(step_noise.shape) != (n_total,) + tuple(x.shape):
        raise RuntimeError("mmd_amd::p_sample_loop: step_noise must be [n_steps_total, n_traj, 64, 4]")
    ws = m.model.workspace(x.shape[0], x.device, sampler=True)
    _lib.launch("mmd_p_sample_loop", x, m.model.handle(m.n_diffusion_steps, x.device), C.byref(s), C.byref(gd) if gd is not None else None, x.data_ptr(),
        _lib.require_gpu(hard, "hard"), int(n_robots), x.shape[0] // int(n_robots), int(n_steps), int(n_steps_without_noise),
        int(bool(init_noise)), _lib.require_gpu(step_noise, "step_noise") if step_noise is not None else None,
        C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), chain.data_ptr() if return_chain else None, ws.data_ptr(), ws.numel())
    return chain


@p_sample_loop.register_fake
def _(x, hard, hard_rows, model, guide, n_robots, n_steps, n_steps_without_noise, init_noise, step_noise, seed,
      n_guide_steps, t_start_guide, noise_std_extra, traj_index_base, return_chain):
    n_total = n_steps + n_steps_without_noise
    return x.new_empty((n_total + 1,) + tuple(x.shape)) if return_chain else x.new_empty(0)


# ---- ddim_sample ---------------------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::ddim_sample", mutates_args=("x",), device_types="cuda")
def ddim_sample(x: torch.Tensor, hard: torch.Tensor, hard_rows: int, model: int, guide: int, n_robots: int,
                n_diffusion_steps: int, init_noise: bool, seed: int, t_start_guide: int, traj_index_base: int,
                return_chain: bool) -> torch.Tensor:
    """GaussianDiffusionModel.ddim_sample (diffusion_model_base.py:213-290, eta = 0) on x in place; chain [n_times, ...]."""
    import numpy as np
    _check_traj(x)
    m = _get(model, "model")
    g = _get(guide, "guide") if guide else None
    s = m._sampler_desc(1, t_start_guide, None, hard_rows, 0, traj_index_base)
    times = np.asarray(m.ddim_times(n_diffusion_steps), dtype=np.int32)
    acp = np.ascontiguousarray(m._tables["alphas_cumprod"], dtype=np.float32)
    gd = g.desc() if g is not None else None
    chain = (torch.empty((len(times),) + tuple(x.shape), dtype=torch.float32, device=x.device) if return_chain
             else torch.empty(0, dtype=torch.float32, device=x.device))
    ws = m.model.workspace(x.shape[0], x.device, sampler=True)
    _lib.launch("mmd_ddim_sample", x, m.model.handle(m.n_diffusion_steps, x.device), C.byref(s), acp.ctypes.data, times.ctypes.data, len(times),
        C.byref(gd) if gd is not None else None, x.data_ptr(), _lib.require_gpu(hard, "hard"), int(n_robots),
        x.shape[0] // int(n_robots), int(bool(init_noise)), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
        chain.data_ptr() if return_chain else None, ws.data_ptr(), ws.numel())
    return chain


@ddim_sample.register_fake
def _(x, hard, hard_rows, model, guide, n_robots, n_diffusion_steps, init_noise, seed, t_start_guide, traj_index_base,
      return_chain):
    n_times = n_diffusion_steps // 5 + 2
    return x.new_empty((n_times,) + tuple(x.shape)) if return_chain else x.new_empty(0)


# ---- solution_stats ------------------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::solution_stats", mutates_args=(), device_types="cuda")
def solution_stats(paths: torch.Tensor, tiles: torch.Tensor, collision_dist: float) -> torch.Tensor:
    """The statistics of a multi-agent solution (inference_multi_agent.py:285-342; mmd_solution_stats): paths [n_agents, Tg, 4] globally
    padded, tiles a HOST float64 tensor [n_tiles, 5] of (agent, t0, offset_x, offset_y, rule) -> float32 [1 + 2 n_agents + n_tiles]: the
    pair-collision count (an int32 in word 0), path length and mean acceleration per agent, adherence per tile."""
    from . import trials
    if not (paths.is_cuda and paths.dtype == torch.float32 and paths.is_contiguous() and paths.ndim == 3 and paths.shape[2] == 4):
        raise RuntimeError("mmd_amd op: paths must be a contiguous float32 CUDA(HIP) tensor [n_agents, Tg, 4]")
    if tiles.is_cuda or tiles.ndim != 2 or tiles.shape[1] != 5:
        raise RuntimeError("mmd_amd op: tiles must be a host tensor [n_tiles, 5]")
    return trials.solution_stats_dev(paths, [tuple(row) for row in tiles.tolist()], collision_dist)


@solution_stats.register_fake
def _(paths, tiles, collision_dist):
    return paths.new_empty(1 + 2 * paths.shape[0] + tiles.shape[0])


# ---- bin_constraints_from_paths ------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::bin_constraints_from_paths", mutates_args=(), device_types="cuda")
def bin_constraints_from_paths(paths: torch.Tensor, radius: float, lo_x: float, lo_y: float, hi_x: float, hi_y: float, nx: int,
                               ny: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The cell-binned inter-robot constraint table of the best paths [n_all, 64, 2] (mmd_bin_constraints_from_paths; include/mmd_amd.h:
    mmd_cons_bins): (cell_off int32 [64, nx ny + 1], entries float32 [64, 9 n_all, 4] of (qx, qy, bit pattern of the robot id, 0))."""
    from . import constraints
    _check_traj(paths, "paths", "n_all", 2)
    return constraints.bin_constraints_table(paths, radius, ((lo_x, lo_y), (hi_x, hi_y)), (nx, ny))


@bin_constraints_from_paths.register_fake
def _(paths, radius, lo_x, lo_y, hi_x, hi_y, nx, ny):
    return (paths.new_empty((64, nx * ny + 1), dtype=torch.int32), paths.new_empty((64, 9 * paths.shape[0], 4)))


# ---- count_collisions_binned / path_conflicts / round_select ----------------------------------------------------------------------
def _collision_table(paths, robot0, n_local):
    from . import constraints
    _check_traj(paths, "paths", "n_all", 2)
    return constraints.binned_collision_table(paths, robot0, n_local)


@torch.library.custom_op("mmd_amd::count_collisions_binned", mutates_args=(), device_types="cuda")
def count_collisions_binned(trajs: torch.Tensor, paths: torch.Tensor, robot0: int, n_local: int, margin: float) -> torch.Tensor:
    """The 'least_collisions' counts int32 [n_local, B] of the local robots' un-normalised samples trajs [n_local * B, 64, 4] against the
    best paths [n_all, 64, 2], on a cell table of the paths built here (mmd_bin_paths + mmd_count_collisions_binned): the integers of
    mmd_count_collisions."""
    from . import multi_agent
    _check_traj(trajs, "trajs")
    return multi_agent.count_collisions_binned(trajs, _collision_table(paths, robot0, n_local), n_local, margin)


@count_collisions_binned.register_fake
def _(trajs, paths, robot0, n_local, margin):
    return trajs.new_empty((n_local, trajs.shape[0] // n_local), dtype=torch.int32)


@torch.library.custom_op("mmd_amd::path_conflicts", mutates_args=(), device_types="cuda")
def path_conflicts(paths: torch.Tensor, margin: float, list_cap: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The conflict report of the best paths [n_all, 64, 2] (mmd_bin_paths + mmd_path_conflicts_binned): (summary int32 [16]: word 0 the
    count, words 4 .. 15 the first mmd_conflict record; robot_counts int32 [n_all]; list int32 [list_cap, 12], the first records)."""
    from . import multi_agent
    summ, robots, lst = multi_agent.path_conflicts(paths, margin, list_cap, _collision_table(paths, 0, paths.shape[0]))
    return summ, robots, lst if lst is not None else paths.new_empty((0, 12), dtype=torch.int32)


@path_conflicts.register_fake
def _(paths, margin, list_cap):
    return (paths.new_empty(16, dtype=torch.int32), paths.new_empty(paths.shape[0], dtype=torch.int32),
            paths.new_empty((list_cap, 12), dtype=torch.int32))


@torch.library.custom_op("mmd_amd::round_select", mutates_args=(), device_types="cuda")
def round_select(paths: torch.Tensor, robot_counts: torch.Tensor, robot0: int, n_local: int, margin: float, mode: int,
                 iters: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The robots a round re-plans, from the best paths [n_all, 64, 2] and path_conflicts' robot_counts of them (mmd_bin_paths +
    mmd_round_select; mode 0 = every robot in conflict, 1 = an independent set by `iters` iterations): (selected int32 [n_all], 0 / 1;
    perm int32 [n_all], the selected ids then the others; header int32 [4] = selected, of them below robot0, of them in
    [robot0, robot0 + n_local), left undecided)."""
    from . import multi_agent
    names = {v: k for k, v in multi_agent.REPLAN_MODES.items()}
    if mode not in names:
        raise RuntimeError(f"mmd_amd op: round_select mode must be one of {sorted(names)}, got {mode}")
    _check_words(robot_counts, "robot_counts", (paths.shape[0],))
    sel = multi_agent.select_replan(paths, _collision_table(paths, robot0, n_local), robot_counts, names[mode], iters, n_local, margin)
    return sel.selected, sel.perm, sel.header


@round_select.register_fake
def _(paths, robot_counts, robot0, n_local, margin, mode, iters):
    n = paths.shape[0]
    return paths.new_empty(n, dtype=torch.int32), paths.new_empty(n, dtype=torch.int32), paths.new_empty(4, dtype=torch.int32)


# ---- the round table: round_constraints_init / round_soft_from_paths / conflict_constraints_append -------------------------------
def _check_round(ell, n_all, n_local, hard_slots):
    S = int(hard_slots) + int(n_all) - 1
    if not (ell.is_cuda and ell.dtype == torch.float32 and ell.is_contiguous() and tuple(ell.shape) == (int(n_local) * S, 64, 4)):
        raise RuntimeError(f"mmd_amd op: ell must be a contiguous float32 CUDA(HIP) tensor [{int(n_local) * S}, 64, 4]")


def _check_words(t, name, shape):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise RuntimeError(f"mmd_amd op: {name} must be a contiguous int32 CUDA(HIP) tensor {list(shape)}")


@torch.library.custom_op("mmd_amd::round_constraints_init", mutates_args=(), device_types="cuda")
def round_constraints_init(like: torch.Tensor, n_all: int, n_local: int, hard_slots: int, weight_hard: float,
                           weight_soft: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """A fresh round table on the device of `like` (mmd_round_constraints_init): (ell float32 [n_local S, 64, 4] with S = hard_slots +
    n_all - 1 -- the hard blocks inactive, the soft blocks unwritten --, grp_slot_off int32 [2 n_local + 1], grp_weight float32
    [2 n_local], robot_grp_off int32 [n_local + 1], fill int32 [n_local, 64] = 0, dropped int32 [n_local] = 0)."""
    from .constraints import group_tensors
    S = int(hard_slots) + int(n_all) - 1
    ell, gso, gw, rgo = group_tensors(max(n_local, 0) * max(S, 0), 2 * n_local, n_local, like.device)
    fill = like.new_empty((n_local, 64), dtype=torch.int32)
    dropped = like.new_empty(n_local, dtype=torch.int32)
    _lib.launch("mmd_round_constraints_init", like, int(n_all), int(n_local), 64, int(hard_slots), float(weight_hard), float(weight_soft),
                ell.data_ptr(), gso.data_ptr(), gw.data_ptr(), rgo.data_ptr(), fill.data_ptr(), dropped.data_ptr())
    return ell, gso, gw, rgo, fill, dropped


@round_constraints_init.register_fake
def _(like, n_all, n_local, hard_slots, weight_hard, weight_soft):
    S = hard_slots + n_all - 1
    return (like.new_empty((n_local * S, 64, 4), dtype=torch.float32), like.new_empty(2 * n_local + 1, dtype=torch.int32),
            like.new_empty(2 * n_local, dtype=torch.float32), like.new_empty(n_local + 1, dtype=torch.int32),
            like.new_empty((n_local, 64), dtype=torch.int32), like.new_empty(n_local, dtype=torch.int32))


@torch.library.custom_op("mmd_amd::round_soft_from_paths", mutates_args=("ell",), device_types="cuda")
def round_soft_from_paths(ell: torch.Tensor, paths: torch.Tensor, robot0: int, n_local: int, hard_slots: int, radius: float) -> None:
    """In place: the soft blocks of the round table `ell` from the best paths [n_all, 64, 2] (mmd_round_soft_from_paths)."""
    _check_traj(paths, "paths", "n_all", 2)
    _check_round(ell, paths.shape[0], n_local, hard_slots)
    _lib.launch("mmd_round_soft_from_paths", ell, paths.data_ptr(), paths.shape[0], int(robot0), int(n_local), 64, int(hard_slots),
                float(radius), ell.data_ptr())


@torch.library.custom_op("mmd_amd::conflict_constraints_append", mutates_args=("ell", "fill", "dropped"), device_types="cuda")
def conflict_constraints_append(ell: torch.Tensor, fill: torch.Tensor, dropped: torch.Tensor, paths: torch.Tensor, robot0: int,
                                n_local: int, hard_slots: int, t_pad: int, margin: float, radius: float) -> None:
    """In place: the hard points of the conflicts of the best paths [n_all, 64, 2] appended to the round table (mmd_bin_paths +
    mmd_conflict_constraints_append; the collision cell table of the paths is built here)."""
    table = _collision_table(paths, robot0, n_local)
    _check_round(ell, paths.shape[0], n_local, hard_slots)
    _check_words(fill, "fill", (n_local, 64))
    _check_words(dropped, "dropped", (n_local,))
    _lib.launch("mmd_conflict_constraints_append", ell, paths.data_ptr(), C.byref(table.struct), int(n_local), 64, int(hard_slots),
                int(t_pad), float(margin), float(radius), ell.data_ptr(), fill.data_ptr(), dropped.data_ptr())


# ---- framed_constraints_from_paths ---------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::framed_constraints_from_paths", mutates_args=(), device_types="cuda")
def framed_constraints_from_paths(paths: torch.Tensor, offsets: torch.Tensor, robot0: int, n_local: int, slots: int, radius: float,
                                  weight: float, lo_x: float, lo_y: float, hi_x: float,
                                  hi_y: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The framed all-pairs table of the GLOBAL best paths [n_all, 64, 2] of robots at offsets [n_all, 2] (mmd_framed_constraints_from_paths),
    culled with the window (lo, hi) of a robot's local frame: (ell float32 [n_local slots, 64, 4], grp_slot_off int32 [n_local + 1],
    grp_weight float32 [n_local], robot_grp_off int32 [n_local + 1], used int32 [n_local], dropped int32 [n_local])."""
    from . import constraints
    _check_traj(paths, "paths", "n_all", 2)
    if not (offsets.is_cuda and offsets.dtype == torch.float32 and offsets.is_contiguous() and tuple(offsets.shape) == (paths.shape[0], 2)):
        raise RuntimeError(f"mmd_amd op: offsets must be a contiguous float32 CUDA(HIP) tensor [{paths.shape[0]}, 2]")
    return constraints.framed_constraints_table(paths, offsets, int(robot0), int(n_local), int(slots), radius, weight, ((lo_x, lo_y), (hi_x, hi_y)))


@framed_constraints_from_paths.register_fake
def _(paths, offsets, robot0, n_local, slots, radius, weight, lo_x, lo_y, hi_x, hi_y):
    return (paths.new_empty((n_local * slots, 64, 4)), paths.new_empty(n_local + 1, dtype=torch.int32), paths.new_empty(n_local),
            paths.new_empty(n_local + 1, dtype=torch.int32), paths.new_empty(n_local, dtype=torch.int32),
            paths.new_empty(n_local, dtype=torch.int32))


# ---- fleet_run_report ------------------------------------------------------------------------------------------------
@torch.library.custom_op("mmd_amd::fleet_run_report", mutates_args=(), device_types="cuda")
def fleet_run_report(paths: torch.Tensor, tex: torch.Tensor, goals: torch.Tensor, lo_x: float, lo_y: float, hi_x: float, hi_y: float,
                     margin: float, rr_margin: float, n_interp: int, goal_tol: float, column_conflicts: bool) -> torch.Tensor:
    """The report of a whole run's global paths [N, L, 2] on the texture tex [nx, ny, 4] over (lo, hi), against goals [N, 2]
    (mmd_fleet_run_report): its one buffer, int32 [8 + 11 N (+ L with column_conflicts)] in include/mmd_amd.h's layout, which
    world_fleet.report_from_words reads from a host copy.  No synchronisation and no copy here."""
    from . import world_fleet
    if not (goals.is_cuda and goals.dtype == torch.float32 and goals.device == paths.device):
        raise RuntimeError("mmd_amd op: goals must be a float32 CUDA(HIP) tensor on the paths' device")
    try:
        return world_fleet.device_run_report_words(paths, tex, (lo_x, lo_y), (hi_x, hi_y), goals, margin, rr_margin, n_interp, goal_tol,
                                                   column_conflicts)
    except ValueError as e:
        raise RuntimeError(f"mmd_amd op: {e}") from e


@fleet_run_report.register_fake
def _(paths, tex, goals, lo_x, lo_y, hi_x, hi_y, margin, rr_margin, n_interp, goal_tol, column_conflicts):
    return paths.new_empty(8 + 11 * paths.shape[0] + (paths.shape[1] if column_conflicts else 0), dtype=torch.int32)
