"""Constraint types (mirror of reference mmd/common/constraints.py:46-85 and the CostConstraint holder,
deps/motion_planning_baselines/mp_baselines/planners/costs/cost_functions.py:275-295) and their packing into the
time-bucketed ELL table the guide kernel reads (include/mmd_amd.h: mmd_guide_desc.cons_ell_dev)."""
import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .multi_agent import RR_MARGIN

VERTEX_CONSTRAINT_RADIUS = 0.05 * 2.4        # mmd/config/mmd_params.py:52
H = 64


class MultiPointConstraint:
    """Same fields and accessors as the reference class (mmd/common/constraints.py:46-85)."""

    def __init__(self, q_l: List[torch.Tensor], t_range_l: List[Tuple[int, int]], radius_l: List[float] = None,
                 is_soft: bool = False):
        self.q_l = q_l
        self.t_range_l = t_range_l
        self.radius_l = [VERTEX_CONSTRAINT_RADIUS] * len(q_l) if radius_l is None else radius_l
        self.is_soft = is_soft

    def get_q_l(self):
        return self.q_l

    def get_t_range_l(self):
        return self.t_range_l

    def get_radius_l(self):
        return self.radius_l

    def get_is_soft(self):
        return self.is_soft

    def get_copy(self):
        return MultiPointConstraint(list(self.q_l), list(self.t_range_l), list(self.radius_l), self.is_soft)


def _points_xy(q_l) -> np.ndarray:
    """[n, 2] float32 host array of the (x, y) of every constraint point.  CBS hands over hundreds of tiny tensors per call
    (cbs.py:468-508), usually device tensors: they are stacked where they live and cross to the host in ONE copy (one by one, each
    `.cpu()` is a device synchronisation: 2 ms of a 5 ms planner call at 568 points)."""
    if torch.is_tensor(q_l):
        q = q_l
    else:
        q_l = list(q_l)
        if not q_l:            # (the reference's torch.stack(q_l) at cost_functions.py:293 fails the same way)
            raise RuntimeError("CostConstraint: stack expects a non-empty list of constraint points")
        try:                                        # (per-element Python work is what costs: one stack, no per-point calls)
            q = torch.stack(q_l)
        except (TypeError, RuntimeError):           # not all tensors, or mixed shapes / devices: the element-wise path
            return np.stack([np.asarray(torch.as_tensor(q).detach().cpu(), dtype=np.float32).reshape(-1)[:2]
                             for q in q_l]).astype(np.float32).reshape(-1, 2)
    q = q.detach().reshape(q.shape[0], -1)
    return np.ascontiguousarray(q[:, :2].to("cpu", torch.float32).numpy()).reshape(-1, 2)


def _ranges(traj_range_l) -> np.ndarray:
    """[n, 2] float32 (the reference keeps them as a float tensor too, cost_functions.py:294).  A list of (t0, t1) pairs goes through
    np.fromiter: 2.5 x faster than np.asarray on a list of tuples, and CBS hands over hundreds per call."""
    if isinstance(traj_range_l, (list, tuple)) and traj_range_l and all(type(t) is tuple and len(t) == 2 for t in traj_range_l):
        try:
            from itertools import chain
            return np.fromiter(chain.from_iterable(traj_range_l), dtype=np.float32, count=2 * len(traj_range_l)).reshape(-1, 2)
        except (TypeError, ValueError):
            pass
    return np.asarray(traj_range_l, dtype=np.float32).reshape(-1, 2)


class CostConstraint:
    """Parameter holder with the reference constructor signature (cost_functions.py:282-295).  One instance = one
    guide cost term = one ELL group (own gradient clip and weight)."""

    def __init__(self, robot=None, n_support_points=H, q_l=None, traj_range_l=None, radius_l=None, is_soft=False,
                 **kwargs):
        self.n_support_points = n_support_points
        self.qs = _points_xy(q_l)
        self.traj_ranges = _ranges(traj_range_l)
        self.radii = np.asarray(radius_l, dtype=np.float32).reshape(-1)
        self.is_soft = is_soft


class PathConstraintGroup(CostConstraint):
    """The group a multi_agent.PathConstraints puts on its agent, in a pack: the host pack reserves its slots (n_slots points, each active at
    t = 0 only, fill exactly n_slots slots) and mmd_path_constraints then writes the whole block on the device (build_path_groups)."""

    def __init__(self, spec, n_slots):
        self.spec, self.n_slots = spec, int(n_slots)
        self.n_support_points = H
        self.qs = np.zeros((self.n_slots, 2), dtype=np.float32)
        self.traj_ranges = np.tile(np.array([[0.0, 1.0]], dtype=np.float32), (self.n_slots, 1))
        self.radii = np.full(self.n_slots, spec.radius, dtype=np.float32)
        self.is_soft = spec.is_soft


def path_constraint_group(spec):
    """PathConstraintGroup of a multi_agent.PathConstraints, or None when the reference would add no group (no point at all)."""
    has_points, n_slots = spec.extent()
    return PathConstraintGroup(spec, n_slots) if has_points else None


def build_path_groups(per_robot_groups, cons, host_offsets):
    """Write every PathConstraintGroup's block into the packed table `cons` (pack_constraints' output) at its slots."""
    flat = [g for groups in per_robot_groups for g, _ in groups]
    for k, g in enumerate(flat):
        if isinstance(g, PathConstraintGroup) and g.n_slots > 0:
            off = int(host_offsets[k])
            g.spec.build(0.0, ell_out=cons[0][off:off + g.n_slots], n_slots=g.n_slots)


def pack_constraints(per_robot_groups: Sequence[Sequence[Tuple[CostConstraint, float]]], device, return_max_slots=False,
                     host_offsets=None):
    """per_robot_groups[r] = [(CostConstraint, weight), ...].  Returns device tensors
    (ell [n_slots,H,4] f32, grp_slot_off [G+1] i32, grp_weight [G] f32, robot_grp_off [R+1] i32) or None if empty.
    `host_offsets` (a list): receives grp_slot_off on the host."""
    lib = _lib.load()
    flat = [gw for groups in per_robot_groups for gw in groups]
    if not flat:
        return (None, 0) if return_max_slots else None
    G = len(flat)
    n_pts = (C.c_int32 * G)(*[g.qs.shape[0] for g, _ in flat])
    keep = []

    def ptr_array(arrs):
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in arrs]
        keep.append(arrs)
        return (C.c_void_p * G)(*[a.ctypes.data for a in arrs])

    q = ptr_array([g.qs for g, _ in flat])
    tr = ptr_array([g.traj_ranges for g, _ in flat])
    rad = ptr_array([g.radii for g, _ in flat])
    slots = (C.c_int32 * G)()
    _lib.check(lib.mmd_pack_constraints(G, n_pts, q, tr, rad, H, None, 0, slots))
    total = int(sum(slots))
    R = len(per_robot_groups)
    # ONE host buffer and ONE upload for the four tables (each pageable host -> device copy is a blocking call of its own, ~12 us,
    # in front of a planner call's first kernel): [ell | grp_slot_off | grp_weight | robot_grp_off], all 4-byte words
    n_ell = max(total, 1) * H * 4
    buf = np.zeros(n_ell + (G + 1) + G + (R + 1), dtype=np.float32)
    ell = buf[:n_ell].reshape(max(total, 1), H, 4)
    ell[..., 2] = -1.0
    _lib.check(lib.mmd_pack_constraints(G, n_pts, q, tr, rad, H, ell.ctypes.data, max(total, 1), slots))
    words = buf.view(np.int32)
    grp_slot_off = words[n_ell:n_ell + G + 1]
    grp_slot_off[1:] = np.cumsum(np.array(list(slots), dtype=np.int64))
    if host_offsets is not None:
        host_offsets.extend(int(v) for v in grp_slot_off)
    buf[n_ell + G + 1:n_ell + 2 * G + 1] = [w for _, w in flat]
    robot_grp_off = words[n_ell + 2 * G + 1:]
    robot_grp_off[1:] = np.cumsum([len(g) for g in per_robot_groups])
    dev = torch.from_numpy(buf).to(device)
    dev_words = dev.view(torch.int32)
    out = (dev[:n_ell].view(max(total, 1), H, 4), dev_words[n_ell:n_ell + G + 1], dev[n_ell + G + 1:n_ell + 2 * G + 1],
           dev_words[n_ell + 2 * G + 1:])
    if return_max_slots:                         # the most slots any one robot owns (sizes the guide kernel's on-chip table)
        per_robot = grp_slot_off[robot_grp_off[1:]] - grp_slot_off[robot_grp_off[:-1]]
        return out, int(per_robot.max())
    return out


def group_tensors(n_slots, n_groups, n_robots, device):
    """(ell [n_slots, H, 4] float32, grp_slot_off [n_groups + 1] int32, grp_weight [n_groups] float32, robot_grp_off [n_robots + 1] int32),
    unwritten, on `device`: the four tensors of an ELL table that a device builder (csrc/cons_tables.hip, mmd_path_constraints) fills."""
    return (torch.empty((n_slots, H, 4), dtype=torch.float32, device=device), torch.empty(n_groups + 1, dtype=torch.int32, device=device),
            torch.empty(n_groups, dtype=torch.float32, device=device), torch.empty(n_robots + 1, dtype=torch.int32, device=device))


def _check_paths(paths, who, n_all=None):
    """Raise unless paths is [N, H, 2] (N = n_all where given)"""
    if paths.dim() != 3 or tuple(paths.shape[1:]) != (H, 2) or (n_all is not None and paths.shape[0] != n_all):
        raise ValueError(f"{who}: paths [{'N' if n_all is None else n_all}, {H}, 2], got {tuple(paths.shape)}")


def _check_robot_range(who, n_all, robot0, n_local):
    """Raise unless [robot0, robot0 + n_local) is a non-empty range of n_all >= 2 robots (check_robot_range, csrc/cons_table_dev.h)"""
    if not (n_all >= 2 and n_local >= 1 and robot0 >= 0 and robot0 + n_local <= n_all):
        raise ValueError(f"{who}: bad robot range")


def soft_constraints_from_paths(paths: torch.Tensor, robot0: int, n_local: int, radius=VERTEX_CONSTRAINT_RADIUS,
                                weight=2e-2):
    """Device-side all-pairs soft constraints (replaces cbs.py:468-508 for equal start times).  paths [N,H,2]
    un-normalised best-path positions of ALL robots on this device; returns the 4 constraint tensors for local
    robots [robot0, robot0+n_local)."""
    lib = _lib.load()
    n_all = paths.shape[0]
    ell, gso, gw, rgo = group_tensors(n_local * (n_all - 1), n_local, n_local, paths.device)
    _lib.launch("mmd_soft_constraints_from_paths", paths, _lib.require_gpu(paths, "paths"), n_all, robot0, n_local, H,
                                                   float(radius), float(weight), ell.data_ptr(), gso.data_ptr(),
                                                   gw.data_ptr(), rgo.data_ptr())
    return ell, gso, gw, rgo, float(radius)


FRAME_WINDOW_SLACK = 1.0625      # a robot's window is the position limits widened by (1 + 1/16) x the radius (csrc/cons_tables.hip)


def framed_window(limits, radius):
    """(lo [2], hi [2]) float32: `limits` = (lo, hi) widened by 1.0625 x radius per side, computed in fp32 -- the window
    framed_constraints_from_paths culls with when none is given."""
    w = np.float32(FRAME_WINDOW_SLACK) * np.float32(radius)
    return (np.asarray(limits[0], dtype=np.float32) - w).astype(np.float32), (np.asarray(limits[1], dtype=np.float32) + w).astype(np.float32)


def framed_constraints_table(paths, offsets, robot0, n_local, slots, radius, weight, window):
    """mmd_framed_constraints_from_paths on checked tensors -> (ell, grp_slot_off, grp_weight, robot_grp_off, used, dropped).  One launch
    on the current stream, no host synchronisation."""
    n_all, dev = paths.shape[0], paths.device
    ell, gso, gw, rgo = group_tensors(n_local * slots, n_local, n_local, dev)
    used = torch.empty(n_local, dtype=torch.int32, device=dev)
    dropped = torch.empty(n_local, dtype=torch.int32, device=dev)
    lo, hi = (C.c_float * 2)(*[float(v) for v in window[0]]), (C.c_float * 2)(*[float(v) for v in window[1]])
    _lib.launch("mmd_framed_constraints_from_paths", paths, _lib.require_gpu(paths, "paths"), _lib.require_gpu(offsets, "offsets"), n_all,
                int(robot0), int(n_local), H, int(slots), float(radius), float(weight), lo, hi, ell.data_ptr(), gso.data_ptr(),
                gw.data_ptr(), rgo.data_ptr(), used.data_ptr(), dropped.data_ptr())
    return ell, gso, gw, rgo, used, dropped


def framed_constraints_from_paths(paths: torch.Tensor, offsets: torch.Tensor, robot0: int, n_local: int, slots: int,
                                  radius=VERTEX_CONSTRAINT_RADIUS, weight=2e-2, window=None):
    """The inter-robot soft constraints of robots that each plan in the model's own tile frame, at offsets [N, 2] in a global frame (global
    = local + offset): paths [N, H, 2] GLOBAL best-path positions of all robots on this device.  Local robot r's block holds, per time
    step t >= 1, the other robots' points paths[j][t] - offsets[r] that fall into `window` = (lo, hi) of r's local frame (default:
    environments.LIMITS widened by 1.0625 x radius, in fp32), packed in ascending id into `slots` slots: the table's size follows the
    local density, not N, and the guided step's result is that of the unculled all-pairs table (a point outside the window can never
    come within `radius` of a clipped trajectory).  -> (ell, grp_slot_off, grp_weight, robot_grp_off, radius) as set_packed_constraints
    takes them, then used int32 [n_local] (the most slots a robot filled at one time step) and dropped int32 [n_local] (included points
    that found the block full; 0 at slots = framed_slot_bound while every path stays in its own window), both on the device."""
    _check_paths(paths, "framed_constraints_from_paths")
    n_all = paths.shape[0]
    if tuple(offsets.shape) != (n_all, 2):
        raise ValueError(f"framed_constraints_from_paths: offsets [{n_all}, 2], got {tuple(offsets.shape)}")
    _check_robot_range("framed_constraints_from_paths", n_all, robot0, n_local)
    if not 1 <= int(slots) <= n_all - 1:
        raise ValueError(f"framed_constraints_from_paths: slots must be in [1, {n_all - 1}], got {slots}")
    if window is None:
        from .environments import LIMITS
        window = framed_window(LIMITS, radius)
    out = framed_constraints_table(paths, offsets, robot0, n_local, slots, radius, weight, window)
    return out[:4] + (float(radius),) + out[4:]


def framed_slot_bound(offsets, robot0, n_local, limits=None, radius=VERTEX_CONSTRAINT_RADIUS):
    """The static slot bound of framed_constraints_from_paths, on the host from the offsets [N, 2] alone: per local robot the number of
    OTHER robots whose window box offset_j + limits intersects this robot's widened window offset_r + (limits -/+ 1.0625 x radius); the
    maximum over the local robots, clamped to [1, N - 1].  While every path stays inside its own window box, no included point is ever
    dropped at this many slots.  The boxes are closed and compared with a few fp32 ulp of the coordinates' size to spare, so the rounding
    of the device's fp32 subtraction cannot include a robot this count left out."""
    if limits is None:
        from .environments import LIMITS
        limits = LIMITS
    off = np.asarray(torch.as_tensor(offsets).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 2)
    n = off.shape[0]
    _check_robot_range("framed_slot_bound", n, robot0, n_local)
    wlo, whi = (np.asarray(v, dtype=np.float64) for v in framed_window(limits, radius))
    lo, hi = np.asarray(limits[0], dtype=np.float64), np.asarray(limits[1], dtype=np.float64)
    eps = 4.0 * float(np.finfo(np.float32).eps) * (np.abs(off).max() + max(np.abs(wlo).max(), np.abs(whi).max()))
    box_lo, box_hi = off + lo, off + hi
    worst = 0
    rows = max(1, SLOT_BOUND_CHUNK_PAIRS // n)          # the local robots, a chunk of rows at a time: [rows, n, 2] comparisons, never n^2
    for r0 in range(robot0, robot0 + n_local, rows):
        own = off[r0:min(r0 + rows, robot0 + n_local)]
        own_lo, own_hi = own + wlo - eps, own + whi + eps
        hit = ((box_hi[None, :, 0] >= own_lo[:, None, 0]) & (box_lo[None, :, 0] <= own_hi[:, None, 0])          # per axis: [rows, n] each
               & (box_hi[None, :, 1] >= own_lo[:, None, 1]) & (box_lo[None, :, 1] <= own_hi[:, None, 1]))
        worst = max(worst, int(np.count_nonzero(hit, axis=1).max()) - 1)      # (robot r's own box always intersects)
    return min(max(worst, 1), n - 1)


SLOT_BOUND_CHUNK_PAIRS = 1 << 20  # framed_slot_bound: robot pairs compared at once (4 MB of comparisons a chunk)


BIN_CELL_SLACK = 1.0625          # a cell side is at least (1 + 1/16) x the radius (csrc/guide.hip: COVER; the build is csrc/cons_tables.hip)
BIN_MAX_CELLS = 32               # per axis, of the default grid


def bin_grid(limits, radius):
    """(nx, ny) of the default cell grid of a cell-binned constraint table over `limits` = (lo [2], hi [2]): the finest grid, up to 32
    cells per axis, whose cells are at least (1 + 1/16) x radius wide -- 15 x 15 on the [-1, 1]^2 maps at the vertex-constraint radius
    0.12.  Raises if even one cell per axis would be too small."""
    lo, hi = limits
    if not radius > 0:
        raise ValueError(f"bin_grid: radius must be positive, got {radius}")
    n = []
    for k in range(2):
        extent = float(hi[k]) - float(lo[k])
        cells = min(BIN_MAX_CELLS, int(np.floor(extent / (BIN_CELL_SLACK * float(radius)))))
        if cells < 1:
            raise ValueError(f"bin_grid: axis {k} of extent {extent} cannot hold a cell of {BIN_CELL_SLACK} x radius = "
                             f"{BIN_CELL_SLACK * float(radius)}")
        n.append(cells)
    return tuple(n)


def check_bin_grid(limits, radius, grid):
    """Raise unless every cell of the nx x ny `grid` over `limits` is at least (1 + 1/16) x radius wide (the library's own rule)."""
    lo, hi = limits
    for k in range(2):
        if int(grid[k]) < 1 or (float(hi[k]) - float(lo[k])) / int(grid[k]) < BIN_CELL_SLACK * float(radius):
            raise ValueError(f"cell grid {tuple(grid)}: cells of axis {k} are smaller than {BIN_CELL_SLACK} x radius")


class BinnedConstraints:
    """A cell-binned inter-robot constraint table on the device (include/mmd_amd.h: mmd_cons_bins): owns the two device tensors and the
    filled struct that GuideManagerTrajectoriesWithVelocity.set_binned_constraints hands to the guided step."""

    def __init__(self, cell_off, entries, limits, grid, n_all, robot0, n_local, radius, weight, first_step=1):
        self.cell_off, self.entries = cell_off, entries
        # 1: a constraint table (no entries at time step 0; the guided step's bits are promised on it), 0: a collision table, which also
        # lists time step 0 (multi_agent.count_collisions_binned / path_conflicts).  The C struct does not carry it.
        self.first_step = int(first_step)
        self.grid, self.n_all, self.robot0, self.n_local = tuple(grid), int(n_all), int(robot0), int(n_local)
        self.radius, self.weight = float(radius), float(weight)
        b = _lib.ConsBins()
        lo, hi = limits
        for k in range(2):
            b.lo[k] = float(lo[k])
            # the fp32 quotient mmd_bin_constraints_from_paths built the table with
            b.inv_cell[k] = float(np.float32(self.grid[k]) / (np.float32(hi[k]) - np.float32(lo[k])))
        b.nx, b.ny, b.n_all, b.robot0 = self.grid[0], self.grid[1], self.n_all, self.robot0
        b.radius, b.weight = self.radius, self.weight
        b.cell_off_dev, b.entries_dev = cell_off.data_ptr(), entries.data_ptr()
        self.struct = b

    def lists(self):
        """Host copy for tests and tools: (offsets [H, nx * ny + 1] int32, entries [H, 9 * n_all, 4] float32, ids [H, 9 * n_all] int32)."""
        ent = self.entries.cpu().numpy()
        return self.cell_off.cpu().numpy(), ent, np.ascontiguousarray(ent[..., 2]).view(np.int32)


def bin_constraints_table(paths: torch.Tensor, radius, limits, grid, first_step=1):
    """mmd_bin_constraints_from_paths (first_step = 1) / mmd_bin_paths: the (cell_off [H, nx * ny + 1] int32, entries [H, 9 * n_all, 4]
    float32) device tensors of the cell table of `paths` [N, H, 2]; time steps below first_step (0 or 1) get empty lists.  One launch on
    the current stream, no host synchronisation."""
    lib = _lib.load()
    n_all, (nx, ny) = paths.shape[0], (int(grid[0]), int(grid[1]))
    cell_off = torch.empty((H, nx * ny + 1), dtype=torch.int32, device=paths.device)
    entries = torch.empty((H, 9 * n_all, 4), dtype=torch.float32, device=paths.device)
    ob, eb = C.c_size_t(), C.c_size_t()
    lib.mmd_cons_bins_bytes(n_all, nx, ny, C.byref(ob), C.byref(eb))
    assert ob.value == cell_off.numel() * 4 and eb.value == entries.numel() * 4
    lo, hi = (C.c_float * 2)(*[float(v) for v in limits[0]]), (C.c_float * 2)(*[float(v) for v in limits[1]])
    if int(first_step) == 1:
        _lib.launch("mmd_bin_constraints_from_paths", paths, _lib.require_gpu(paths, "paths"), n_all, H, float(radius), lo, hi, nx, ny,
                    cell_off.data_ptr(), entries.data_ptr())
    else:
        _lib.launch("mmd_bin_paths", paths, _lib.require_gpu(paths, "paths"), n_all, H, float(radius), lo, hi, nx, ny, int(first_step),
                    cell_off.data_ptr(), entries.data_ptr())
    return cell_off, entries


def binned_constraints_from_paths(paths: torch.Tensor, robot0: int, n_local: int, radius=VERTEX_CONSTRAINT_RADIUS, weight=2e-2,
                                  limits=None, grid=None, first_step=1):
    """The soft constraints of soft_constraints_from_paths as a cell table: per time step and map cell the robots near that cell
    instead of N - 1 slots per robot, O(N) instead of O(N^2) work and memory per round, and the same bits out of the guided step.
    paths [N, H, 2] un-normalised best-path positions of ALL robots on this device; the table serves the local robots
    [robot0, robot0 + n_local).  limits = (lo, hi) of the map (default: environments.LIMITS), grid = (nx, ny) (default: bin_grid).
    first_step = 0 also lists time step 0: a collision table (binned_collision_table), which the guide refuses."""
    if limits is None:
        from .environments import LIMITS
        limits = LIMITS
    n_all = paths.shape[0]
    _check_paths(paths, "binned_constraints_from_paths")
    _check_robot_range("binned_constraints_from_paths", n_all, robot0, n_local)
    grid = bin_grid(limits, radius) if grid is None else tuple(int(v) for v in grid)
    check_bin_grid(limits, radius, grid)
    if int(first_step) not in (0, 1):
        raise ValueError(f"binned_constraints_from_paths: first_step must be 0 or 1, got {first_step}")
    cell_off, entries = bin_constraints_table(paths, radius, limits, grid, first_step)
    return BinnedConstraints(cell_off, entries, limits, grid, n_all, robot0, n_local, radius, weight, first_step)


def binned_collision_table(paths: torch.Tensor, robot0: int = 0, n_local: int = None, reach=VERTEX_CONSTRAINT_RADIUS, limits=None,
                           grid=None):
    """The cell table of the best paths [N, H, 2] for the collision kernels (multi_agent.count_collisions_binned / path_conflicts): every
    time step listed, t = 0 included, since collisions count there.  reach: the largest collision margin the table can serve; the default,
    the constraint radius (0.12 >= the 0.105 robot-robot margin), reuses the constraint table's 15 x 15 grid.  n_local defaults to all
    robots from robot0 on.  The weight field is not read by those kernels."""
    n_local = paths.shape[0] - int(robot0) if n_local is None else n_local
    return binned_constraints_from_paths(paths, robot0, n_local, radius=reach, weight=0.0, limits=limits, grid=grid, first_step=0)


class RoundConstraints:
    """The round table of a many-robot round on the device (include/mmd_amd.h: mmd_round_constraints_init): per local robot a hard group
    of up to `hard_slots` points per time step -- the midpoints of the conflicts seen so far, as CBS gives both agents of a conflict a
    hard constraint (convert_conflicts_to_constraints, mmd/common/conflict_conversion.py:41-55) -- in front of the soft all-pairs group
    of soft_constraints_from_paths.  Owns the tensors; `fill` int32 [n_local, H] (hard slots in use per time step) and `dropped` int32
    [n_local] (points that found the hard block full) stay on the device.  Every call is launches on the current stream, no host
    synchronisation.  reset() -> set_soft(paths) / append_conflicts(paths, table) per round -> tensors() for
    GuideManagerTrajectoriesWithVelocity.set_packed_constraints."""

    def __init__(self, n_all, robot0, n_local, hard_slots=32, radius=VERTEX_CONSTRAINT_RADIUS, w_hard=2e-1, w_soft=2e-2,
                 hard_radius=None, device="cuda"):
        self.n_all, self.robot0, self.n_local, self.hard_slots = int(n_all), int(robot0), int(n_local), int(hard_slots)
        _check_robot_range("RoundConstraints", self.n_all, self.robot0, self.n_local)
        if self.hard_slots < 1:
            raise ValueError(f"RoundConstraints: hard_slots must be at least 1, got {hard_slots}")
        self.radius = float(radius)
        self.hard_radius = self.radius if hard_radius is None else float(hard_radius)
        self.w_hard, self.w_soft = float(w_hard), float(w_soft)
        self.slots_per_robot = self.hard_slots + self.n_all - 1
        dev = torch.device(device)
        self.ell, self.gso, self.gw, self.rgo = group_tensors(self.n_local * self.slots_per_robot, 2 * self.n_local, self.n_local, dev)
        self.fill = torch.empty((self.n_local, H), dtype=torch.int32, device=dev)
        self.dropped = torch.empty(self.n_local, dtype=torch.int32, device=dev)
        self.reset()

    def reset(self):
        """Offsets and weights, an empty hard block for every robot, fill and dropped zeroed.  The soft blocks are set_soft's."""
        _lib.launch("mmd_round_constraints_init", self.ell, self.n_all, self.n_local, H, self.hard_slots, self.w_hard, self.w_soft,
                    self.ell.data_ptr(), self.gso.data_ptr(), self.gw.data_ptr(), self.rgo.data_ptr(), self.fill.data_ptr(),
                    self.dropped.data_ptr())

    def _paths(self, paths_all, what):
        _check_paths(paths_all, f"RoundConstraints.{what}", self.n_all)
        return _lib.require_gpu(paths_all.contiguous(), "paths_all")

    def set_soft(self, paths_all):
        """The soft blocks from the best paths [N, H, 2] of all robots: soft_constraints_from_paths' rows of the local robots."""
        _lib.launch("mmd_round_soft_from_paths", self.ell, self._paths(paths_all, "set_soft"), self.n_all, self.robot0, self.n_local, H,
                    self.hard_slots, self.radius, self.ell.data_ptr())

    def append_conflicts(self, paths_all, collision_table, margin=RR_MARGIN, t_pad=2):
        """Append the hard points of the conflicts of paths_all [N, H, 2], read off their collision cell table
        (binned_collision_table(paths_all, robot0, n_local)): every record (tc, a, b, mid) of multi_agent.path_conflicts gives a and b the
        point mid with range (tc - t_pad, tc + t_pad), in report order behind the earlier calls' points."""
        tb = collision_table
        if getattr(tb, "first_step", None) != 0:
            raise ValueError("RoundConstraints.append_conflicts: a collision table lists time step 0 (binned_collision_table)")
        if (tb.n_all, tb.robot0) != (self.n_all, self.robot0) or tb.n_local < self.n_local:
            raise ValueError(f"RoundConstraints.append_conflicts: a table of robots [{tb.robot0}, {tb.robot0 + tb.n_local}) of {tb.n_all}")
        _lib.launch("mmd_conflict_constraints_append", self.ell, self._paths(paths_all, "append_conflicts"), C.byref(tb.struct),
                    self.n_local, H, self.hard_slots, int(t_pad), float(margin), self.hard_radius, self.ell.data_ptr(),
                    self.fill.data_ptr(), self.dropped.data_ptr())

    def tensors(self):
        """(ell, grp_slot_off, grp_weight, robot_grp_off, uniform_radius) for set_packed_constraints.  uniform_radius: the one radius of
        every active point when the hard and the soft radius are equal (the reference: both vertex_constraint_radius), else 0.0, the
        guided step's general path."""
        return self.ell, self.gso, self.gw, self.rgo, self.radius if self.hard_radius == self.radius else 0.0
