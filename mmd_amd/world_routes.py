"""World routes: from a start to a goal anywhere on a world map, the sequence of robot windows between them.

A world map (environments.register_world_map) is larger than the model's tile; MPDEnsemble carries a robot across tiles, given the tile
skeleton.  Here the skeleton is found: a geodesic distance field of the world texture's routable cells per goal, a descent from the
start that lists the lattice tiles the cell path crosses, and the glue that makes the list an MPDEnsemble (route_planner).  Tile-to-tile
connectivity depends on the fine obstacles (a wall with a door), so the search runs on the cell grid.

The numpy functions routable_cells, grid_distance_field and descend ARE the definition; mmd_grid_distance_field and mmd_grid_descend
(include/mmd_amd.h, csrc/grid_route.hip) compute the same integers on the device, and the tests hold them to equality.

  routable[ix, iy] = tex[ix, iy, 0] > clearance (a strict float32 compare: a NaN texel is not routable), inside `region`
  dist[f, ix, iy]  = steps of the shortest 4-connected path over routable cells from goals[f]; UNREACHED elsewhere
The field is 4-connected with unit cost on purpose: a step crosses at most one lattice line, so consecutive tiles of a route share an
edge, which is what MPDEnsemble's cross conditioning (the end of tile k pinned to the start of tile k + 1) needs.

The cell path itself becomes the planner's prior (world_routes_seeded, route_experience): descend_samples keeps 64 support cells per tile
visit and seed_trajectory turns them into a smoothed chain of points with velocities, in trajs_final's format.  These two numpy functions
are the definition as well; mmd_grid_descend_samples and mmd_route_seeds (csrc/route_seeds.hip) compute the same integers and the same
float32 bits."""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, environments
from .environments import LIMITS, SDF_CELL_SIZE
from .world import OBSTACLE_MARGIN

UNREACHED = _lib.GRID_DIST_UNREACHED
ROUTE_OK, ROUTE_UNREACHED, ROUTE_STUCK, ROUTE_TOO_MANY_TILES, ROUTE_OUTSIDE = 0, 1, 2, 3, 4       # the status codes of a descent
_NEIGHBOURS = ((1, 0), (-1, 0), (0, 1), (0, -1))             # +x, -x, +y, -y: the candidate order of the descent


# ---- the definitions, on the host ----------------------------------------------------------------------------------------------------
def _region(region, shape):
    r = (0, 0, shape[0], shape[1]) if region is None else tuple(int(v) for v in region)
    if len(r) != 4 or not (0 <= r[0] <= r[2] <= shape[0] and 0 <= r[1] <= r[3] <= shape[1]):
        raise ValueError(f"region = (i_lo, j_lo, i_hi, j_hi) with lo <= hi inside the grid of {shape[0]} x {shape[1]} cells, got {region!r}")
    return r


def routable_cells(tex, clearance=OBSTACLE_MARGIN, region=None):
    """bool [nx, ny]: tex[ix, iy, 0] > float32(clearance) inside region = (i_lo, j_lo, i_hi, j_hi), upper bounds exclusive (None: the whole
    grid).  tex: float32 [nx, ny, 4], any map's SDF texture."""
    tex = np.asarray(tex)
    if tex.ndim != 3 or tex.dtype != np.float32:
        raise ValueError(f"routable_cells: a float32 texture [nx, ny, 4], got {tex.dtype} {tex.shape}")
    r = _region(region, tex.shape[:2])
    out = np.zeros(tex.shape[:2], bool)
    with np.errstate(invalid="ignore"):
        out[r[0]:r[2], r[1]:r[3]] = tex[r[0]:r[2], r[1]:r[3], 0] > np.float32(clearance)
    return out


def grid_distance_field(routable, goals):
    """int32 [n_fields, nx, ny]: per goal (ix, iy) a level-synchronous breadth-first search over the routable cells, 4-connected; UNREACHED
    where a cell is not routable or not reached.  A goal that is not routable or lies outside the grid: UNREACHED everywhere."""
    routable = np.asarray(routable, bool)
    nx, ny = routable.shape
    goals = np.asarray(goals, np.int64).reshape(-1, 2)
    free = routable.reshape(-1)
    out = np.full((goals.shape[0], nx * ny), UNREACHED, np.int32)
    for f, (gx, gy) in enumerate(goals.tolist()):
        if not (0 <= gx < nx and 0 <= gy < ny and routable[gx, gy]):
            continue
        dist = out[f]
        frontier = np.array([gx * ny + gy], np.int64)
        dist[frontier] = 0
        level = 0
        while frontier.size:
            level += 1
            ix, iy = frontier // ny, frontier % ny
            nxt = np.concatenate([frontier[ix + 1 < nx] + ny, frontier[ix > 0] - ny, frontier[iy + 1 < ny] + 1, frontier[iy > 0] - 1])
            nxt = np.unique(nxt[free[nxt] & (dist[nxt] == UNREACHED)])
            dist[nxt] = level
            frontier = nxt
    return out.reshape(-1, nx, ny)


def descend(dist, start, tile, lattice_origin=(0, 0), max_tiles=16):
    """(tiles int32 [min(n_tiles, max_tiles), 2], steps, n_tiles, status): the walk down one field dist [nx, ny] from the cell `start`.
    While d = dist[c] > 0: the candidates are the neighbours of c in the order +x, -x, +y, -y that lie inside the grid and hold exactly
    d - 1; the first candidate in the lattice tile of c is taken, else the first candidate.  Lattice tile (a, b) covers the cells
    [o + a * tile, o + (a + 1) * tile) per axis, o = lattice_origin.  The list starts with the start's tile and gets a tile each time the
    walk enters one other than the last listed; repeats are kept.  status: ROUTE_OK (steps = dist[start]); ROUTE_UNREACHED (steps = -1,
    no tile); ROUTE_STUCK (no candidate: the field was not converged; steps and tiles are what the walk covered); ROUTE_TOO_MANY_TILES
    (n_tiles is the true count, the first max_tiles are returned); ROUTE_OUTSIDE (the start is not a cell of the grid; steps = -1)."""
    dist = np.asarray(dist)
    nx, ny = dist.shape
    tile, max_tiles = int(tile), int(max_tiles)
    if tile < 1 or max_tiles < 1:
        raise ValueError(f"descend: tile = {tile}, max_tiles = {max_tiles} (both at least 1)")
    o = (int(lattice_origin[0]), int(lattice_origin[1]))
    ix, iy = int(start[0]), int(start[1])
    none = np.zeros((0, 2), np.int32)
    if not (0 <= ix < nx and 0 <= iy < ny):
        return none, -1, 0, ROUTE_OUTSIDE
    d = int(dist[ix, iy])
    if d == UNREACHED:
        return none, -1, 0, ROUTE_UNREACHED
    here = ((ix - o[0]) // tile, (iy - o[1]) // tile)
    tiles, n_tiles, steps, status = [here], 1, 0, ROUTE_OK
    while d > 0:
        cand = [(ix + dx, iy + dy) for dx, dy in _NEIGHBOURS
                if 0 <= ix + dx < nx and 0 <= iy + dy < ny and int(dist[ix + dx, iy + dy]) == d - 1]
        if not cand:
            status = ROUTE_STUCK
            break
        same = [c for c in cand if ((c[0] - o[0]) // tile, (c[1] - o[1]) // tile) == here]
        ix, iy = same[0] if same else cand[0]
        d -= 1
        steps += 1
        if not same:
            here = ((ix - o[0]) // tile, (iy - o[1]) // tile)
            if n_tiles < max_tiles:
                tiles.append(here)
            n_tiles += 1
    if status == ROUTE_OK and n_tiles > max_tiles:
        status = ROUTE_TOO_MANY_TILES
    return np.asarray(tiles, np.int32).reshape(-1, 2), steps, n_tiles, status


SEED_POINTS = _lib.ROUTE_SEED_POINTS                         # support points per tile visit: the tile model's horizon


def sample_offsets(m):
    """int64 [64]: the path cells of a visit of m cells that its support points fall on, off(j) = (j * (m - 1) + 31) // 63: exact integers,
    monotone in j, off(0) = 0 and off(63) = m - 1; every cell of the visit is hit while m <= 64."""
    return (np.arange(SEED_POINTS, dtype=np.int64) * (int(m) - 1) + 31) // 63


def descend_samples(dist, start, tile, lattice_origin=(0, 0), max_tiles=16):
    """(tiles, steps, n_tiles, status, visit_cells int32 [K], cells int32 [K, 64, 2]): descend() with the support cells of the cell path.
    The walk is descend's, rule for rule, and the first four results are descend's.  The cell path is c_0 (the start) .. c_steps (the
    goal); visit k, the k-th listed tile, owns the path indices [f_k, f_k + m_k), m_k >= 1: visit_cells[k] = m_k, and support point j of
    visit k is the cell c[f_k + sample_offsets(m_k)[j]].  With a status other than ROUTE_OK there are no samples: K = 0."""
    tiles, steps, n_tiles, status = descend(dist, start, tile, lattice_origin, max_tiles)
    none = np.zeros(0, np.int32), np.zeros((0, SEED_POINTS, 2), np.int32)
    if status != ROUTE_OK:
        return (tiles, steps, n_tiles, status) + none
    dist = np.asarray(dist)
    nx, ny = dist.shape
    tile, o = int(tile), (int(lattice_origin[0]), int(lattice_origin[1]))
    tile_of = lambda c: ((c[0] - o[0]) // tile, (c[1] - o[1]) // tile)                          # noqa: E731
    path, first = [(int(start[0]), int(start[1]))], [0]                      # the cell path, and f_k per visit
    for d in range(int(dist[path[0]]), 0, -1):
        ix, iy = path[-1]
        cand = [(ix + dx, iy + dy) for dx, dy in _NEIGHBOURS if 0 <= ix + dx < nx and 0 <= iy + dy < ny and int(dist[ix + dx, iy + dy]) == d - 1]
        same = [c for c in cand if tile_of(c) == tile_of(path[-1])]
        if not same:
            first.append(len(path))
        path.append(same[0] if same else cand[0])
    assert len(path) == steps + 1 and len(first) == n_tiles
    visit_cells = np.diff(np.asarray(first + [len(path)], np.int64)).astype(np.int32)
    path = np.asarray(path, np.int32)
    cells = np.stack([path[f + sample_offsets(m)] for f, m in zip(first, visit_cells)])
    return tiles, steps, n_tiles, status, visit_cells, cells


def _f32(a):
    return np.asarray(a, np.float32)


def cell_centres(cells, lo, hi, shape):
    """float32 [..., 2]: the centres of the cells [..., 2] of a grid of `shape` over lo .. hi, by THE fp32 sequence of the seed: per axis
    lo + (float32(cell) + 0.5) * pitch, pitch = |hi - lo| / float32(n): a convert, an add, a multiply, an add, one rounding each.  The
    texel of a centre (_texels) is its cell."""
    lo, hi = _f32(lo), _f32(hi)
    pitch = np.abs(hi - lo) / _f32(shape[:2])
    return lo + (np.asarray(cells).astype(np.float32) + np.float32(0.5)) * pitch


def _texels(points, lo, hi, shape):
    """(ix, iy) int64 of float32 points [n, 2]: mmd_sdf_grid_lookup's sequence, environments._texel_indices for every finite point; the
    clamp is fmax then fmin, which drop a NaN (index 0), as the device's do."""
    lo, hi = _f32(lo), _f32(hi)
    dim = np.abs(hi - lo)
    with np.errstate(over="ignore", invalid="ignore"):
        idx = [np.fmin(np.fmax(np.floor((points[:, k] - lo[k]) / dim[k] * np.float32(shape[k])), np.float32(0)),
                       np.float32(shape[k] - 1)).astype(np.int64) for k in range(2)]
    return idx[0], idx[1]


def _bits_order(values):
    """int32 keys that order like the float32 values' bits: -0 below +0, a NaN beyond the infinity of its sign"""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.int32)
    return bits ^ ((bits >> 31) & np.int32(0x7fffffff))


def seed_trajectory(tex, lo, hi, cells, tiles, tile, lattice_origin, start_point, goal_point, clearance=OBSTACLE_MARGIN, smooth_iters=64,
                    dt=5.0 / 64):
    """(seed float32 [K * 64, 4], clear_min float32): the seed trajectory of a route, in trajs_final's format, from descend_samples' cells
    [K, 64, 2] and tiles [K, 2] on the texture tex [nx, ny, 4] over lo .. hi.  Every operation is float32 with one rounding.
      p[64 k + j] = cell_centres(cells[k, j]); p[0] = start_point and p[-1] = goal_point, the caller's exact points, which stay fixed.
      smooth_iters Jacobi iterations over the whole chain, every interior i from the iteration before (so no order matters):
        c = 0.5 * (p[i - 1] + p[i + 1]); (ix, iy) = the texel of c; p'[i] = c iff tex[ix, iy, 0] > float32(clearance) (strict; a NaN
        rejects) and (ix, iy) is a cell of lattice tile tiles[i // 64]; else p'[i] = p[i].
      v[i] = (p[i + 1] - p[i - 1]) / float32(2 * dt) for interior i, 0 at both ends; seed[i] = (p.x, p.y, v.x, v.y).
      clear_min = the least texel value over the final points (least in the order of the values' bits, _bits_order).
    What the seed promises: every support point of every iteration whose cell was routable keeps the clearance and lies in its own
    tile's window, which is what lets MPDEnsemble split the seed into tile frames.  It does NOT promise the clearance of the segments
    between support points: a visit with a long in-tile path has widely spaced samples, and the planner's own collision split judges
    them.  K = 0: an empty seed and clear_min 0."""
    tex = np.asarray(tex)
    if tex.ndim != 3 or tex.dtype != np.float32:
        raise ValueError(f"seed_trajectory: a float32 texture [nx, ny, 4], got {tex.dtype} {tex.shape}")
    cells = np.asarray(cells, np.int32).reshape(-1, SEED_POINTS, 2)
    tiles = np.asarray(tiles, np.int64).reshape(-1, 2)
    two_dt = np.float32(2.0 * float(dt))
    if int(smooth_iters) < 0 or not (np.isfinite(two_dt) and two_dt > 0) or int(tile) < 1 or len(tiles) != len(cells):
        raise ValueError(f"seed_trajectory: smooth_iters = {smooth_iters} (>= 0), dt = {dt} (finite, > 0), tile = {tile} (>= 1), "
                         f"{len(tiles)} tiles for {len(cells)} visits")
    if len(cells) == 0:
        return np.zeros((0, 4), np.float32), np.float32(0)
    shape = tex.shape[:2]
    p = np.ascontiguousarray(cell_centres(cells.reshape(-1, 2), lo, hi, shape), dtype=np.float32)
    p[0], p[-1] = _f32(start_point).reshape(2), _f32(goal_point).reshape(2)
    first = np.repeat(tiles * int(tile) + np.asarray(lattice_origin, np.int64), SEED_POINTS, axis=0)[1:-1]    # the first cell of i's tile
    clearance = np.float32(clearance)
    for _ in range(int(smooth_iters)):
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.float32(0.5) * (p[:-2] + p[2:])
            ix, iy = _texels(c, lo, hi, shape)
            ok = tex[ix, iy, 0] > clearance
        ok &= (ix >= first[:, 0]) & (ix < first[:, 0] + int(tile)) & (iy >= first[:, 1]) & (iy < first[:, 1] + int(tile))
        p[1:-1] = np.where(ok[:, None], c, p[1:-1])
    seed = np.zeros((len(p), 4), np.float32)
    seed[:, :2] = p
    with np.errstate(over="ignore", invalid="ignore"):
        seed[1:-1, 2:] = (p[2:] - p[:-2]) / two_dt
    ix, iy = _texels(p, lo, hi, shape)
    values = tex[ix, iy, 0]
    return seed, values[np.argmin(_bits_order(values))]


# ---- the same on the device ------------------------------------------------------------------------------------------------------------
def _int32_dev(a, shape, device, what):
    t = torch.as_tensor(a).to(dtype=torch.int32).reshape(shape).contiguous()
    if t.dim() and t.shape[0] == 0:
        raise ValueError(f"{what}: nothing given")
    return t.to(device)


def device_distance_field(tex_dev, goals, clearance=OBSTACLE_MARGIN, region=None, sweeps_per_call=8, max_sweeps=None):
    """(dist, sweeps): int32 [n_fields, nx, ny] on tex_dev's device, grid_distance_field(routable_cells(tex, clearance, region), goals) to
    the integer, and the number of sweeps run.  All fields go through one launch sequence: mmd_grid_distance_field is called with
    sweeps_per_call sweeps per call until its per-field count of changed blocks reads all zero, one read of 4 * n_fields bytes per call.
    max_sweeps=None: the number of routable cells + 2, which always suffices (a sweep that does not end the search settles a cell);
    RuntimeError if the fields have not converged by then."""
    nx, ny = int(tex_dev.shape[0]), int(tex_dev.shape[1])
    if tex_dev.dim() != 3 or tex_dev.shape[2] != 4:
        raise ValueError(f"device_distance_field: a texture [nx, ny, 4], got {tuple(tex_dev.shape)}")
    tex_p = _lib.require_gpu(tex_dev, "texture")
    r = _region(region, (nx, ny))
    goals_dev = _int32_dev(goals, (-1, 2), tex_dev.device, "device_distance_field: goals")
    n = goals_dev.shape[0]
    if int(sweeps_per_call) < 1:
        raise ValueError(f"device_distance_field: sweeps_per_call = {sweeps_per_call} (at least 1)")
    if max_sweeps is None:
        max_sweeps = int((tex_dev[r[0]:r[2], r[1]:r[3], 0] > np.float32(clearance)).sum().item()) + 2
    lib = _lib.load()
    work_bytes = lib.mmd_grid_distance_work_bytes(nx, ny, n)
    if work_bytes == 0:
        raise ValueError(f"device_distance_field: {n} fields of {nx} x {ny} cells are refused (include/mmd_amd.h: mmd_grid_distance_field)")
    dist = torch.empty(n, nx, ny, dtype=torch.int32, device=tex_dev.device)
    work = torch.empty(work_bytes // 4, dtype=torch.int32, device=tex_dev.device)
    changed = torch.empty(n, dtype=torch.int32, device=tex_dev.device)
    region_c = (C.c_int32 * 4)(*r)
    sweeps, restart = 0, 1
    while True:
        k = min(int(sweeps_per_call), max_sweeps - sweeps)
        if k <= 0:
            raise RuntimeError(f"device_distance_field: {n} fields of {nx} x {ny} cells not converged after {sweeps} sweeps (max_sweeps = {max_sweeps})")
        _lib.launch("mmd_grid_distance_field", tex_dev, tex_p, nx, ny, float(clearance), region_c, C.c_void_p(goals_dev.data_ptr()), n, restart,
                    k, C.c_void_p(dist.data_ptr()), C.c_void_p(work.data_ptr()), work_bytes, C.c_void_p(changed.data_ptr()))
        sweeps, restart = sweeps + k, 0
        if not changed.cpu().any():
            return dist, sweeps


def device_descend(dist_dev, starts, fields, tile, lattice_origin=(0, 0), max_tiles=16):
    """(tiles int32 [n, max_tiles, 2], summary int32 [n, 4] = (steps, n_tiles, status, 0)) on dist_dev's device: descend() for query q from
    starts[q] in field dist_dev[fields[q]], all queries in one launch.  Rows of tiles behind a query's n_tiles are zero."""
    if dist_dev.dim() != 3 or dist_dev.dtype != torch.int32 or not dist_dev.is_cuda or not dist_dev.is_contiguous():
        raise ValueError("device_descend: dist must be a contiguous int32 CUDA(HIP) tensor [n_fields, nx, ny]")
    starts_dev = _int32_dev(starts, (-1, 2), dist_dev.device, "device_descend: starts")
    n = starts_dev.shape[0]
    fields_dev = _int32_dev(fields, (n,), dist_dev.device, "device_descend: fields")
    tiles = torch.zeros(n, int(max_tiles), 2, dtype=torch.int32, device=dist_dev.device)
    summary = torch.zeros(n, 4, dtype=torch.int32, device=dist_dev.device)
    _lib.launch("mmd_grid_descend", dist_dev, C.c_void_p(dist_dev.data_ptr()), int(dist_dev.shape[1]), int(dist_dev.shape[2]),
                int(dist_dev.shape[0]), C.c_void_p(starts_dev.data_ptr()), C.c_void_p(fields_dev.data_ptr()), n, int(tile),
                (C.c_int32 * 2)(int(lattice_origin[0]), int(lattice_origin[1])), int(max_tiles), C.c_void_p(tiles.data_ptr()),
                C.c_void_p(summary.data_ptr()))
    return tiles, summary


def device_descend_samples(dist_dev, starts, fields, tile, lattice_origin=(0, 0), max_tiles=16):
    """(tiles, summary, visit_cells int32 [n, max_tiles], cells int32 [n, max_tiles, 64, 2]) on dist_dev's device: descend_samples() for
    every query in one launch (mmd_grid_descend_samples).  tiles and summary are device_descend's; rows of visit_cells and cells behind a
    query's n_tiles, and all rows of a query whose status is not ROUTE_OK, are zero."""
    if dist_dev.dim() != 3 or dist_dev.dtype != torch.int32 or not dist_dev.is_cuda or not dist_dev.is_contiguous():
        raise ValueError("device_descend_samples: dist must be a contiguous int32 CUDA(HIP) tensor [n_fields, nx, ny]")
    starts_dev = _int32_dev(starts, (-1, 2), dist_dev.device, "device_descend_samples: starts")
    n = starts_dev.shape[0]
    fields_dev = _int32_dev(fields, (n,), dist_dev.device, "device_descend_samples: fields")
    tiles = torch.zeros(n, int(max_tiles), 2, dtype=torch.int32, device=dist_dev.device)
    summary = torch.zeros(n, 4, dtype=torch.int32, device=dist_dev.device)
    visit_cells = torch.empty(n, int(max_tiles), dtype=torch.int32, device=dist_dev.device)
    cells = torch.empty(n, int(max_tiles), SEED_POINTS, 2, dtype=torch.int32, device=dist_dev.device)
    _lib.launch("mmd_grid_descend_samples", dist_dev, C.c_void_p(dist_dev.data_ptr()), int(dist_dev.shape[1]), int(dist_dev.shape[2]),
                int(dist_dev.shape[0]), C.c_void_p(starts_dev.data_ptr()), C.c_void_p(fields_dev.data_ptr()), n, int(tile),
                (C.c_int32 * 2)(int(lattice_origin[0]), int(lattice_origin[1])), int(max_tiles), C.c_void_p(tiles.data_ptr()),
                C.c_void_p(summary.data_ptr()), C.c_void_p(visit_cells.data_ptr()), C.c_void_p(cells.data_ptr()))
    return tiles, summary, visit_cells, cells


def device_route_seeds(tex_dev, lo, hi, cells, tiles, summary, tile, lattice_origin, start_points, goal_points, clearance=OBSTACLE_MARGIN,
                       smooth_iters=64, dt=5.0 / 64):
    """(seeds float32 [n, max_tiles * 64, 4], clear_min float32 [n]) on tex_dev's device: seed_trajectory() for every route in one launch
    (mmd_route_seeds), from device_descend_samples' cells, tiles and summary.  Route q's seed is seeds[q, :64 * n_tiles]; the rows behind
    it, and every row of a route whose status is not ROUTE_OK, are zero."""
    if tex_dev.dim() != 3 or tex_dev.shape[2] != 4:
        raise ValueError(f"device_route_seeds: a texture [nx, ny, 4], got {tuple(tex_dev.shape)}")
    tex_p = _lib.require_gpu(tex_dev, "texture")
    dev = tex_dev.device
    ok = lambda t, shape: t.dtype == torch.int32 and t.device == dev and t.is_contiguous() and tuple(t.shape[1:]) == shape      # noqa: E731
    n, max_tiles = int(summary.shape[0]), int(tiles.shape[1]) if tiles.dim() == 3 else 0
    if not (summary.dim() == 2 and n >= 1 and ok(summary, (4,)) and ok(tiles, (max_tiles, 2)) and ok(cells, (max_tiles, SEED_POINTS, 2))
            and tiles.shape[0] == n and cells.shape[0] == n):
        raise ValueError("device_route_seeds: cells [n, max_tiles, 64, 2], tiles [n, max_tiles, 2] and summary [n, 4], contiguous int32 on the "
                         "texture's device, as device_descend_samples returns them")
    pts = [torch.as_tensor(p, dtype=torch.float32).reshape(n, 2).contiguous().to(dev) for p in (start_points, goal_points)]
    seeds = torch.empty(n, max_tiles * SEED_POINTS, 4, dtype=torch.float32, device=dev)
    clear_min = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.launch("mmd_route_seeds", tex_dev, tex_p, int(tex_dev.shape[0]), int(tex_dev.shape[1]), (C.c_float * 2)(*map(float, lo)),
                (C.c_float * 2)(*map(float, hi)), float(clearance), C.c_void_p(cells.data_ptr()), C.c_void_p(tiles.data_ptr()),
                C.c_void_p(summary.data_ptr()), n, int(tile), (C.c_int32 * 2)(int(lattice_origin[0]), int(lattice_origin[1])), max_tiles,
                C.c_void_p(pts[0].data_ptr()), C.c_void_p(pts[1].data_ptr()), int(smooth_iters), float(np.float32(2.0 * float(dt))),
                C.c_void_p(seeds.data_ptr()), C.c_void_p(clear_min.data_ptr()))
    return seeds, clear_min


# ---- world maps --------------------------------------------------------------------------------------------------------------------------
class WorldRoute(NamedTuple):
    """One route on a world map: K windows from the start's to the goal's, consecutive ones sharing an edge (a window may occur twice)."""
    tiles: np.ndarray           # int32 [K, 2]: the lattice indices (a, b)
    origins: np.ndarray         # int32 [K, 2]: the windows' origin cells in the world
    offsets: np.ndarray         # float32 [K, 2]: the windows' offsets, global = local + offset (environments.snap_to_world_map's formula)
    transforms: dict            # {k: float32 tensor [2]}: MPDEnsemble's transforms
    env_ids: list               # [environments.world_window_name(name, origins[k])]: MPDEnsemble's env_ids
    steps: int                  # the length of the cell path, in cells


def world_cells(name, points_global):
    """int32 [n, 2]: the cell of the world map `name` that holds each global point [n, 2]: the texel every consumer of the world texture
    reads for it (environments._texel_indices over world_map_limits).  A point that is not finite or lies outside the world is refused."""
    pts = np.ascontiguousarray(environments._host_array(torch.as_tensor(points_global, dtype=torch.float32)), dtype=np.float32).reshape(-1, 2)
    lo, hi = environments.world_map_limits(name)
    shape = environments.world_map_occupancy(name).shape
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(~((pts >= np.asarray(lo, np.float32)) & (pts <= np.asarray(hi, np.float32))).all(1))
    if bad.size:
        raise ValueError(f"world_cells: point {int(bad[0])} = {pts[bad[0]].tolist()} lies outside the world map {name!r}, {lo} .. {hi}")
    ix, iy, _ = environments._texel_indices(pts, lo, hi, shape)
    return np.stack([ix, iy], axis=1).astype(np.int32)


def world_lattice(name, lattice_origin=(0, 0)):
    """(region, (na, nb)): the tile lattice of the world map `name`.  Lattice tile (a, b) is the window whose origin cell is
    lattice_origin + (a, b) * 400; lattice_origin = (o_i, o_j) with 0 <= o < 400 per axis.  na x nb tiles lie wholly inside the world and
    region = (o_i, o_j, o_i + na * 400, o_j + nb * 400) is their union: the cells of the leftover strips are not routable."""
    shape = environments.world_map_occupancy(name).shape
    tile = environments.grid_shape()
    o = (int(lattice_origin[0]), int(lattice_origin[1]))
    if not all(0 <= o[k] < tile[k] for k in range(2)):
        raise ValueError(f"world_lattice: lattice_origin = {lattice_origin!r}: per axis a cell in 0 .. {tile[0] - 1}")
    n = tuple((shape[k] - o[k]) // tile[k] for k in range(2))
    if min(n) < 1:
        raise ValueError(f"world_lattice: no whole tile of the world map {name!r} ({shape[0]} x {shape[1]} cells) at lattice_origin = {o}")
    return (o[0], o[1], o[0] + n[0] * tile[0], o[1] + n[1] * tile[1]), n


def _route(name, tiles, steps, lattice_origin):
    tile = environments.grid_shape()
    tiles = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 2)
    origins = (tiles.astype(np.int64) * np.asarray(tile) + np.asarray(lattice_origin, np.int64)).astype(np.int32)
    offsets = (origins.astype(np.float64) * np.float64(SDF_CELL_SIZE) + np.asarray(environments.world_map_origin(name), np.float64)
               - np.asarray(LIMITS[0], np.float64)).astype(np.float32)
    return WorldRoute(tiles, origins, offsets, {k: torch.from_numpy(offsets[k].copy()) for k in range(len(tiles))},
                      [environments.world_window_name(name, origins[k]) for k in range(len(tiles))], int(steps))


def _points(points):
    return np.ascontiguousarray(environments._host_array(torch.as_tensor(points, dtype=torch.float32)), dtype=np.float32).reshape(-1, 2)


def world_routes(name, starts, goals, clearance=OBSTACLE_MARGIN, device=None, lattice_origin=(0, 0), max_tiles=16):
    """[WorldRoute]: route q from the global point starts[q] to goals[q] ([n, 2] each) on the world map `name`.  One distance field per
    distinct goal cell over the cells whose texture value exceeds `clearance` (default: the margin random_world_map_instance accepts starts
    and goals by) inside world_lattice's region, then one descent per query.  device=None: the definitions on world_map_texture(name) (slow
    to build for a large world).  With a device: the kernels on the resident world texture (map_textures.device_world_texture), all fields
    in one launch sequence and all descents in one launch; the results are equal.  Route again after update_world_map.
    ValueError: a start or goal outside the world or in the leftover strip of the lattice; a goal that cannot be reached (the message
    names the start and goal cells); a route of more than max_tiles tiles (it names max_tiles and the count needed)."""
    return _world_routes(name, starts, goals, clearance, device, lattice_origin, max_tiles)[0]


def _world_routes(name, starts, goals, clearance, device, lattice_origin, max_tiles, seed_args=None):
    """world_routes' body -> (routes, seeds).  seed_args: None (no seeds) or world_routes_seeded's (smooth_iters, dt): the descents then
    keep their support cells, and the seeds are built from them after the routes have passed world_routes' checks."""
    seeded, seeds = seed_args is not None, None
    tile = environments.grid_shape()
    region, _ = world_lattice(name, lattice_origin)
    s_cells, g_cells = world_cells(name, starts), world_cells(name, goals)
    if s_cells.shape != g_cells.shape or s_cells.shape[0] == 0:
        raise ValueError(f"world_routes: {s_cells.shape[0]} starts and {g_cells.shape[0]} goals (equal and at least 1)")
    for what, cells in (("start", s_cells), ("goal", g_cells)):
        bad = np.flatnonzero(~((cells >= region[:2]) & (cells < region[2:])).all(1))
        if bad.size:
            raise ValueError(f"world_routes: the {what} of route {int(bad[0])}, cell {cells[bad[0]].tolist()}, lies in the leftover strip of "
                             f"the world map {name!r}: the lattice tiles cover the cells {region[:2]} .. {region[2:]} (upper bounds exclusive)")
    fields, which = np.unique(g_cells, axis=0, return_inverse=True)
    which = which.reshape(-1)
    if device is None:
        dist = grid_distance_field(routable_cells(environments.world_map_texture(name), clearance, region), fields)
        walk = descend_samples if seeded else descend
        found = [walk(dist[which[q]], s_cells[q], tile[0], lattice_origin, max_tiles) for q in range(len(s_cells))]
    else:
        from . import map_textures
        tex = map_textures.device_world_texture(name, device)
        dist, _ = device_distance_field(tex, fields, clearance, region)
        if seeded:
            tiles_dev, summary_dev, _, cells_dev = device_descend_samples(dist, s_cells, which, tile[0], lattice_origin, max_tiles)
        else:
            tiles_dev, summary_dev = device_descend(dist, s_cells, which, tile[0], lattice_origin, max_tiles)
        tiles, summary = tiles_dev.cpu().numpy(), summary_dev.cpu().numpy()
        found = [(tiles[q, :min(int(summary[q, 1]), int(max_tiles))], int(summary[q, 0]), int(summary[q, 1]), int(summary[q, 2]))
                 for q in range(len(s_cells))]
    routes = []
    for q, (tiles, steps, n_tiles, status, *_) in enumerate(found):
        if status == ROUTE_UNREACHED:
            raise ValueError(f"world_routes: route {q} on {name!r}: the goal cell {g_cells[q].tolist()} cannot be reached from the start cell "
                             f"{s_cells[q].tolist()} at clearance {clearance}")
        if status == ROUTE_TOO_MANY_TILES:
            raise ValueError(f"world_routes: route {q} on {name!r} crosses {n_tiles} tiles, above max_tiles = {max_tiles}")
        if status != ROUTE_OK:
            raise RuntimeError(f"world_routes: route {q} on {name!r}: descent status {status} from the start cell {s_cells[q].tolist()}")
        routes.append(_route(name, tiles, steps, lattice_origin))
    if seeded:
        smooth_iters, dt = seed_args
        lo, hi = environments.world_map_limits(name)
        s_pts, g_pts = _points(starts), _points(goals)
        if device is None:
            tex = environments.world_map_texture(name)
            seeds = [torch.from_numpy(seed_trajectory(tex, lo, hi, found[q][5], found[q][0], tile[0], lattice_origin, s_pts[q], g_pts[q],
                                                      clearance, smooth_iters, dt)[0]) for q in range(len(found))]
        else:
            rows, _ = device_route_seeds(tex, lo, hi, cells_dev, tiles_dev, summary_dev, tile[0], lattice_origin, s_pts, g_pts, clearance,
                                         smooth_iters, dt)
            seeds = [rows[q, :SEED_POINTS * len(routes[q].tiles)] for q in range(len(routes))]
    return routes, seeds


def world_route(name, start, goal, clearance=OBSTACLE_MARGIN, device=None, lattice_origin=(0, 0), max_tiles=16):
    """world_routes for one start and one goal (global points [2]) -> WorldRoute"""
    one = lambda p: np.asarray(environments._host_array(torch.as_tensor(p, dtype=torch.float32)), np.float32).reshape(1, 2)   # noqa: E731
    return world_routes(name, one(start), one(goal), clearance, device, lattice_origin, max_tiles)[0]


def world_routes_seeded(name, starts, goals, clearance=OBSTACLE_MARGIN, device=None, lattice_origin=(0, 0), max_tiles=16, smooth_iters=64,
                        trajectory_duration=5.0):
    """(routes, seeds): world_routes' routes for the same arguments, and per route the seed trajectory of its cell path, a float32 tensor
    [K_q * 64, 4] in the global frame and in trajs_final's format (seed_trajectory over descend_samples; dt = trajectory_duration / 64,
    guides.py's dt).  device=None: the definitions on world_map_texture(name).  With a device: the kernels on the resident world texture
    and on the fields the routes were found on, all samples from one launch (mmd_grid_descend_samples) and all seeds from one launch
    (mmd_route_seeds); the seeds live on that device, and the results are equal bit for bit.  The same ValueErrors as world_routes, and
    one for max_tiles above 16 or a negative smooth_iters.
    smooth_iters = 64 is a documented choice, not a measured optimum (profiles/route_seeds.txt records the seed's length against it);
    the definition is exact for any value.  The seed keeps the clearance at its support points, not on the segments between them."""
    if not 1 <= int(max_tiles) <= _lib.ROUTE_SEED_MAX_TILES or int(smooth_iters) < 0 or not float(trajectory_duration) > 0:
        raise ValueError(f"world_routes_seeded: max_tiles = {max_tiles} (1 to {_lib.ROUTE_SEED_MAX_TILES}), smooth_iters = {smooth_iters} "
                         f"(>= 0), trajectory_duration = {trajectory_duration} (> 0)")
    return _world_routes(name, starts, goals, clearance, device, lattice_origin, max_tiles,
                         (int(smooth_iters), float(trajectory_duration) / SEED_POINTS))


def world_route_seeded(name, start, goal, clearance=OBSTACLE_MARGIN, device=None, lattice_origin=(0, 0), max_tiles=16, smooth_iters=64,
                       trajectory_duration=5.0):
    """world_routes_seeded for one start and one goal (global points [2]) -> (WorldRoute, seed [K * 64, 4])"""
    routes, seeds = world_routes_seeded(name, _points(start), _points(goal), clearance, device, lattice_origin, max_tiles, smooth_iters,
                                        trajectory_duration)
    return routes[0], seeds[0]


def route_experience(seed, n_samples):
    """The PathBatchExperience of a seed [K * 64, 4] repeated to [n_samples, K * 64, 4]: what a route's planner takes as `experience`,
    planner = route_planner(route, ...); planner(start, goal, experience=route_experience(seed, planner.num_samples)).  The call then runs
    MPDEnsemble's local inference: the seed forward-noised a few steps, split into the tile frames and denoised under the guide."""
    from .planners import PathBatchExperience
    seed = torch.as_tensor(seed, dtype=torch.float32)
    if seed.dim() != 2 or seed.shape[1] != 4 or seed.shape[0] == 0 or seed.shape[0] % SEED_POINTS or int(n_samples) < 1:
        raise ValueError(f"route_experience: a seed [K * 64, 4] and n_samples >= 1, got {tuple(seed.shape)} and {n_samples}")
    return PathBatchExperience(seed.unsqueeze(0).repeat(int(n_samples), 1, 1))


def route_planner(route, model_id, start_state_pos, goal_state_pos, **mpd_ensemble_kwargs):
    """The MPDEnsemble of a route: one tile model per window, the windows' offsets as transforms and their map names as env_ids.  Starts
    and goals are global, as MPDEnsemble takes them; a route of one window is allowed.  This is what replaces a hand-written tile skeleton
    (the reference's inference_multi_agent.py:418-431)."""
    from .planners import MPDEnsemble
    K = len(route.env_ids)
    return MPDEnsemble(model_ids=(model_id,) * K, transforms=route.transforms, env_ids=route.env_ids, start_state_pos=start_state_pos,
                       goal_state_pos=goal_state_pos, **mpd_ensemble_kwargs)
