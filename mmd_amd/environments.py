"""2-D maps of the reference (geometry only) and their precomputed SDF grids (host side, init time).

Geometry: deps/torch_robotics/torch_robotics/environments/env_{empty,empty_nowait,highways,conveyor,drop_region}_2d.py.
SDF: MultiRoundedBoxField (primitives.py:312-333) composed with the empty MultiSphereField's constant 1
(primitives.py:109-110) through ObjectField's min (:567-570); grid = GridMapSDF.precompute_sdf
(grid_map_sdf.py:34-63): value and autograd gradient on linspace(lo,hi,ceil(dim/cell))^2.
The reference rebuilds this grid N+1 times per trial (once per planner); here it is built once per map and shared.

Custom maps (register_map): any set of spheres and rounded boxes on the same tile at the same cell size, what the reference's EnvBase
takes as ObjectField([MultiSphereField, MultiBoxField]).  The host texture (sdf_grid_texture, torch autograd) is the definition; the
resident device texture of a registered map is built by the library (mmd_sdf_grid_build, csrc/sdf_grid.hip), bit for bit the same.

Occupancy maps (register_occupancy_map): a [nx, ny] bitmap of the tile's cells -- a floor plan, a benchmark grid, a costmap -- instead
of primitives.  occupancy_sdf_texture (numpy, an exact Euclidean distance transform with nearest-site tracking) is the definition;
the resident texture is built by mmd_sdf_grid_from_occupancy, bit for bit the same.  Both kinds share one name space.

World maps (register_world_map): one bitmap for a world larger than a tile, up to 2048 cells per side.  The world's texture is
occupancy_sdf_texture of the whole bitmap; a robot's map is the 400 x 400 window of it at the robot's offset (world_map_windows is the
definition, world_window_name its map name); on a device the windows are cut from the resident world texture by mmd_sdf_grid_windows.
The section at the end of this file.
"""
import ctypes as C

import numpy as np
import torch

MAP_BOXES = {
    "EnvEmpty2D": ([], []),
    "EnvEmptyNoWait2D": ([], []),
    "EnvHighways2D": ([[0, 0.0], [0., 0.875], [0., -0.875], [0.875, 0.0], [-0.875, 0.0], [0.875, 0.875],
                       [0.875, -0.875], [-0.875, 0.875], [-0.875, -0.875]],
                      [[0.5, 0.5], [0.5, 0.25], [0.5, 0.25], [0.25, 0.5], [0.25, 0.5], [0.25, 0.25], [0.25, 0.25],
                       [0.25, 0.25], [0.25, 0.25]]),
    "EnvConveyor2D": ([[0, 0], [0, 0.35], [0, -0.35]], [[0.8, 0.1], [1.0, 0.1], [1.0, 0.1]]),
    "EnvDropRegion2D": ([[0.4, 0.4], [-0.4, 0.4], [0.4, -0.4], [-0.4, -0.4]], [[0.4, 0.4]] * 4),
}
LIMITS = ((-1.0, -1.0), (1.0, 1.0))
SDF_CELL_SIZE = 0.005

_EXTRA_SUFFIX = "ExtraObjects"
_REGISTERED = {}           # name -> (boxes, spheres): tuples of float tuples, rounded to fp32
_OCCUPANCY = {}            # name -> the [nx, ny] uint8 bitmap (0 / 1) as bytes, row-major: the other kind of registered map
_TEXTURE_CACHE = {}        # (base name, cell size) -> (content the texture was built from, texture)


def _base_name(map_name):
    return map_name.replace(_EXTRA_SUFFIX, "")


def _primitive_rows(rows, width, what):
    a = np.asarray(list(rows), dtype=np.float32)
    if a.size == 0:
        return ()
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what}: [n][{width}] numbers, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: every number must be finite")
    if not (a[:, 2:] > 0).all():
        raise ValueError(f"{what}: sizes and radii must be positive")
    return tuple(tuple(float(v) for v in row) for row in a)


def _checked_primitives(boxes, spheres):
    return (_primitive_rows(boxes, 4, "boxes [(cx, cy, size_x, size_y)]"), _primitive_rows(spheres, 3, "spheres [(cx, cy, r)]"))


def register_map(name, boxes=(), spheres=()):
    """A map of rounded boxes [(cx, cy, size_x, size_y)] (MultiBoxField's centers and sizes) and spheres [(cx, cy, r)] (MultiSphereField's
    centers and radii) on the tile LIMITS at SDF_CELL_SIZE, usable wherever a shipped map name is.  Registering the same content under a
    name twice is a no-op; other content under a taken name, a shipped name and a name that contains 'ExtraObjects' (the suffix is
    stripped from every map name) are refused."""
    if not isinstance(name, str) or not name:
        raise ValueError(f"register_map: a non-empty string name, got {name!r}")
    if name in MAP_BOXES:
        raise ValueError(f"register_map: {name!r} is a shipped map")
    if _EXTRA_SUFFIX in name:
        raise ValueError(f"register_map: {name!r} contains {_EXTRA_SUFFIX!r}, which is stripped from map names")
    content = _checked_primitives(boxes, spheres)
    _refuse_world_name(name, "register_map")
    if name in _OCCUPANCY:
        raise ValueError(f"register_map: {name!r} is registered as an occupancy map")
    if name in _REGISTERED and _REGISTERED[name] != content:
        raise ValueError(f"register_map: {name!r} is registered with other primitives (update_map replaces them)")
    _REGISTERED[name] = content


def unregister_map(name):
    """Forget a registered map of either kind, its host texture and every resident device texture that holds it (objects built on it
    keep theirs)."""
    if name not in _REGISTERED and name not in _OCCUPANCY:
        raise ValueError(f"unregister_map: {name!r} is not a registered map")
    _REGISTERED.pop(name, None)
    _OCCUPANCY.pop(name, None)
    _drop_host_texture(name)
    from . import guides
    guides.drop_resident_textures(name)


def registered_maps():
    """The names of the registered maps of both kinds, sorted."""
    return tuple(sorted(set(_REGISTERED) | set(_OCCUPANCY)))


def map_primitives(name):
    """(boxes [(cx, cy, size_x, size_y)], spheres [(cx, cy, r)]) of a shipped or registered map."""
    base = _base_name(name)
    if _window_of(base) is not None:
        raise ValueError(f"map_primitives: {name!r} is a window of a world map (world_map_occupancy returns the world's bitmap)")
    if base in _OCCUPANCY:
        raise ValueError(f"map_primitives: {name!r} is an occupancy map (map_occupancy returns its bitmap)")
    if base in _REGISTERED:
        return _REGISTERED[base]
    if base not in MAP_BOXES:
        raise KeyError(f"unknown map {name!r} (shipped: {sorted(MAP_BOXES)}; registered: {list(registered_maps())})")
    centers, sizes = MAP_BOXES[base]
    return tuple((float(c[0]), float(c[1]), float(s[0]), float(s[1])) for c, s in zip(centers, sizes)), ()


def is_registered(name):
    base = _base_name(name)
    return base in _REGISTERED or base in _OCCUPANCY


def is_occupancy_map(name):
    return _base_name(name) in _OCCUPANCY


def map_has_obstacles(name):
    """Whether the map's fixed objects have an SDF grid (mmd_guide_desc.n_grids = 1).  A registered map always has one, even without
    primitives or occupied cells: update_map / update_occupancy_map may give it some while a guide that reads the grid is alive.
    A window of a world map: whether the world has an occupied cell now (a guide built on a window of an empty world reads no grid, and
    an update_world_map that adds the first obstacle does not reach it)."""
    base = _base_name(name)
    window = _window_of(base)
    if window is not None:
        return b"\x01" in _WORLD_MAPS[window[0]][1]
    return base in _REGISTERED or base in _OCCUPANCY or len(MAP_BOXES[base][0]) > 0


def _rounded_box_sdfs(x, centers, sizes):
    """MultiRoundedBoxField.compute_signed_distance_impl before its min over the boxes (primitives.py:324-332)."""
    radius = torch.min(sizes, dim=-1)[0] * 0.15
    q = torch.abs(x.unsqueeze(-2) - centers.unsqueeze(0)) - (sizes / 2).unsqueeze(0) + radius.unsqueeze(0).unsqueeze(-1)
    max_q = torch.amax(q, dim=-1)
    return torch.minimum(max_q, torch.zeros_like(max_q)) + torch.linalg.norm(torch.relu(q), dim=-1) - radius.unsqueeze(0)


def _primitives_sdf(x, boxes, spheres):
    """ObjectField([MultiSphereField(spheres), MultiBoxField(boxes)]) at the identity pose (primitives.py:108-115, :326-333, :569-572):
    torch.min over the stacked fields, spheres first, so the first of equal minima takes the gradient; an empty sphere field is the
    constant 1, an empty box field is left out."""
    fields = []
    if len(spheres) == 0:
        fields.append(torch.ones_like(x[..., 0]))
    else:
        s = torch.tensor(spheres, dtype=torch.float32)
        fields.append(torch.min(torch.norm(x.unsqueeze(-2) - s[:, :2].unsqueeze(0), dim=-1) - s[:, 2], dim=-1)[0])
    if len(boxes):
        b = torch.tensor(boxes, dtype=torch.float32)
        fields.append(torch.min(_rounded_box_sdfs(x, b[:, :2], b[:, 2:]), dim=-1)[0])
    return torch.min(torch.stack(fields, dim=-1), dim=-1)[0]


def map_sdf(points, map_name):
    x = torch.as_tensor(points, dtype=torch.float32)
    base = _base_name(map_name)
    if base in _OCCUPANCY or _window_of(base) is not None:
        return _nearest_cell_sdf(x, sdf_grid_texture(base))
    if base in _REGISTERED:
        return _primitives_sdf(x, *_REGISTERED[base])
    centers, sizes = MAP_BOXES[base]
    ones = torch.ones_like(x[..., 0])
    if len(centers) == 0:
        return ones
    centers = torch.tensor(centers, dtype=torch.float32)
    sizes = torch.tensor(sizes, dtype=torch.float32)
    return torch.minimum(ones, torch.min(_rounded_box_sdfs(x, centers, sizes), dim=-1)[0])


def grid_shape(cell_size=SDF_CELL_SIZE):
    lo, hi = torch.tensor(LIMITS[0]), torch.tensor(LIMITS[1])
    cmap = torch.ceil(torch.abs(hi - lo) / cell_size).long()
    return int(cmap[0]), int(cmap[1])


def grid_node_rows(cell_size=SDF_CELL_SIZE):
    """The node coordinates of the grid per axis, torch.linspace on the CPU as GridMapSDF.precompute_sdf computes them."""
    lo, hi = torch.tensor(LIMITS[0]), torch.tensor(LIMITS[1])
    nx, ny = grid_shape(cell_size)
    return torch.linspace(lo[0], hi[0], nx), torch.linspace(lo[1], hi[1], ny)


def _drop_host_texture(name):
    for key in [k for k in _TEXTURE_CACHE if k[0] == name]:
        del _TEXTURE_CACHE[key]


def sdf_grid_texture(map_name, cell_size=SDF_CELL_SIZE):
    """float32 numpy [nx, ny, 4] = (sdf, dsdf/dx, dsdf/dy, 0): the texture layout mmd_guide_desc expects."""
    base = _base_name(map_name)
    window = _window_of(base)
    if window is not None:                                       # (the host crop of the world's texture, which is cached by content)
        if grid_shape(cell_size) != grid_shape():
            raise ValueError(f"sdf_grid_texture: the world map {window[0]!r} has one cell per grid cell at {SDF_CELL_SIZE}, not at {cell_size}")
        return world_map_windows(window[0], [window[1:]])[0]
    content = _OCCUPANCY.get(base, _REGISTERED.get(base))        # (None: a shipped map, whose content never changes)
    hit = _TEXTURE_CACHE.get((base, cell_size))
    if hit is not None and hit[0] == content:
        return hit[1]
    if base in _OCCUPANCY:
        if grid_shape(cell_size) != grid_shape():
            raise ValueError(f"sdf_grid_texture: the occupancy map {base!r} has one cell per grid cell at {SDF_CELL_SIZE}, not at {cell_size}")
        tex = occupancy_sdf_texture(map_occupancy(base), cell_size)
    else:
        tex = _texture(lambda pts: map_sdf(pts, map_name), *grid_node_rows(cell_size))
    _TEXTURE_CACHE[(base, cell_size)] = (content, tex)
    return tex


def _texture(sdf_fn, xs, ys):
    """GridMapSDF.precompute_sdf (grid_map_sdf.py:34-63): value and autograd gradient of sdf_fn at the nodes (xs[ix], ys[iy])."""
    pts = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), dim=-1)
    pts.requires_grad_(True)
    sdf = sdf_fn(pts)
    grad = torch.autograd.grad(sdf.sum(), pts)[0] if sdf.requires_grad else torch.zeros_like(pts)
    tex = torch.zeros(xs.shape[0], ys.shape[0], 4)
    tex[..., 0] = sdf.detach()
    tex[..., 1:3] = grad
    return np.ascontiguousarray(tex.numpy())


def primitives_sdf_texture(boxes, spheres, xs, ys):
    """The host texture [len(xs), len(ys), 4] of a set of primitives on ANY node rows (float32 CPU tensors): the definition
    mmd_sdf_grid_build is held to on grids other than the tile's."""
    boxes, spheres = _checked_primitives(boxes, spheres)
    return _texture(lambda pts: _primitives_sdf(pts, boxes, spheres), torch.as_tensor(xs, dtype=torch.float32),
                    torch.as_tensor(ys, dtype=torch.float32))


# ---- the grid on the device ---------------------------------------------------------------------------------------
_NODE_ROWS_DEV = {}        # device -> (xs, ys) of the tile's grid


def primitive_tables(boxes, spheres):
    """The library's tables: spheres [n][4] = (cx, cy, r, 0), boxes [n][4] = (cx, cy, half x, half y) -- mmd_guide_desc's extra_spheres_dev /
    extra_boxes_dev layouts -- as float32 numpy."""
    boxes, spheres = _checked_primitives(boxes, spheres)
    sph = np.asarray(spheres, dtype=np.float32).reshape(-1, 3)
    box = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return (np.concatenate([box[:, :2], box[:, 2:] / np.float32(2)], 1),
            np.concatenate([sph, np.zeros((len(sph), 1), np.float32)], 1))


def device_sdf_grid(boxes, spheres, device, out=None):
    """The [nx, ny, 4] texture of a map of these primitives, built on `device` by mmd_sdf_grid_build: what sdf_grid_texture computes on the
    host, bit for bit but for the sign of a zero (+0 here), for the upload of the primitives and the two rows of node coordinates.  out= rebuilds a resident texture in place
    on the current stream."""
    from . import _lib
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    nx, ny = grid_shape()
    if out is None:
        out = torch.empty(nx, ny, 4, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (nx, ny, 4) or out.device != device:
        raise ValueError(f"device_sdf_grid: out must be [{nx}, {ny}, 4] on {device}, got {tuple(out.shape)} on {out.device}")
    box, sph = primitive_tables(boxes, spheres)
    rows = _NODE_ROWS_DEV.get(str(device))
    if rows is None:
        rows = _NODE_ROWS_DEV[str(device)] = tuple(r.to(device) for r in grid_node_rows())
    box_dev = torch.from_numpy(box).to(device) if len(box) else None
    sph_dev = torch.from_numpy(sph).to(device) if len(sph) else None
    _lib.launch("mmd_sdf_grid_build", out, C.c_void_p(sph_dev.data_ptr()) if sph_dev is not None else None, len(sph),
                C.c_void_p(box_dev.data_ptr()) if box_dev is not None else None, len(box),
                _lib.require_gpu(rows[0], "xs"), nx, _lib.require_gpu(rows[1], "ys"), ny, _lib.require_gpu(out, "out"))
    return out


def update_map(name, boxes=(), spheres=()):
    """Replace a registered map's primitives and rebuild every resident device texture slice of that name in place (same storage): guides
    and task facades that share it see the new map on their next call.  The host texture of the name is dropped."""
    if name in _OCCUPANCY:
        raise ValueError(f"update_map: {name!r} is an occupancy map (update_occupancy_map replaces its bitmap)")
    if name not in _REGISTERED:
        raise ValueError(f"update_map: {name!r} is not a registered map")
    _REGISTERED[name] = _checked_primitives(boxes, spheres)
    _drop_host_texture(name)
    from . import guides
    guides.rebuild_resident_textures(name)


# ---- occupancy maps -------------------------------------------------------------------------------------------------
_OCC_NONE = 1 << 14        # "this row holds no such cell": its square is above every real squared distance (csrc/sdf_grid.hip: OCC_NONE)
OCCUPANCY_MAX_SIDE = 2048  # MMD_OCCUPANCY_MAX_SIDE: 2 * 2047^2 < 2^24, so every squared distance is an exact float32


def _row_offsets(site):
    """Pass 1: [nx, ny] signed iy offset to the nearest True cell of the same ix row, a tie to the smaller jy; _OCC_NONE in a row without."""
    nx, ny = site.shape
    iy = np.arange(ny)
    out = np.full((nx, ny), _OCC_NONE, np.int32)
    for ix in range(nx):
        js = np.flatnonzero(site[ix])
        if len(js):
            d = js[None, :] - iy[:, None]
            out[ix] = d[iy, np.argmin(np.abs(d), axis=1)]              # argmin: the first minimum = the smaller jy (js ascends)
    return out


def _nearest_site(site):
    """(D2, ix - jx, iy - jy) [nx, ny] int32 to every cell's nearest True cell (jx, jy): minimal D2 = dx^2 + dy^2, the lexicographically
    smallest (jx, jy) among equal D2.  Pass 2 over the row offsets: the first minimum over jx, ascending, strict <.  D2 >= _OCC_NONE^2
    where `site` holds no True cell."""
    nx, ny = site.shape
    g = _row_offsets(site)
    g2 = g * g
    best = np.full((nx, ny), np.iinfo(np.int32).max, np.int32)
    best_dx, best_dy = np.zeros((nx, ny), np.int32), np.zeros((nx, ny), np.int32)
    ix = np.arange(nx, dtype=np.int32)[:, None]
    for jx in range(nx):
        dx = ix - np.int32(jx)
        d2 = dx * dx + g2[jx][None, :]
        m = d2 < best
        best = np.where(m, d2, best)
        best_dx = np.where(m, dx, best_dx)
        best_dy = np.where(m, -g[jx][None, :], best_dy)
    return best, best_dx, best_dy


def _checked_occupancy(occupancy, what, shape=None):
    occ = np.asarray(occupancy)
    if occ.ndim != 2 or occ.size == 0 or (shape is not None and occ.shape != tuple(shape)):
        raise ValueError(f"{what}: an occupancy bitmap of shape {'[nx, ny]' if shape is None else list(shape)}, got {list(occ.shape)}")
    if occ.dtype.kind not in "buif":
        raise ValueError(f"{what}: a numeric or boolean bitmap (non-zero = occupied), got dtype {occ.dtype}")
    return np.ascontiguousarray(occ != 0).view(np.uint8)


def occupancy_sdf_texture(occ, cell=SDF_CELL_SIZE):
    """THE DEFINITION of an occupancy map's SDF texture: float32 [nx, ny, 4] = (sdf, d/dx, d/dy, 0) of the bitmap occ [nx, ny] (non-zero
    = occupied), indexed like the texture: cell (ix, iy) is the cell the grid lookup floor((p - lo) / (hi - lo) * n) gives a point, the
    cell pitch is `cell`.  For a cell, the site is the nearest cell of the other class: D2 = (ix - jx)^2 + (iy - jy)^2 minimal (an exact
    integer), the lexicographically smallest (jx, jy) among equal D2.  s = sqrt(float32(D2)), v = cell * s - 0.5 * cell (the obstacle's
    surface lies on the cell edge), every operation in fp32 with one rounding.  A free cell: (+v, (ix - jx) / s, (iy - jy) / s), away from
    the obstacle -- or (1, 0, 0) where v is not below 1, the constant-1 field of the primitive maps.  An occupied cell: (-v, (jx - ix) / s,
    (jy - iy) / s), towards free space.  A zero component is +0.  No occupied cell: (1, 0, 0, 0) everywhere; no free cell: (-1, 0, 0, 0)."""
    occ = _checked_occupancy(occ, "occupancy_sdf_texture").astype(bool)
    nx, ny = occ.shape
    if max(nx, ny) > OCCUPANCY_MAX_SIDE:
        raise ValueError(f"occupancy_sdf_texture: {nx} x {ny} cells, at most {OCCUPANCY_MAX_SIDE} per side")
    f = np.float32
    cell = f(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"occupancy_sdf_texture: cell = {cell} (finite and positive)")
    tex = np.zeros((nx, ny, 4), f)
    for own, sign in ((~occ, 1), (occ, -1)):
        d2, dx, dy = _nearest_site(~own)
        none = d2 >= _OCC_NONE * _OCC_NONE
        s = np.sqrt(np.where(none | ~own, 1, d2).astype(f))          # (a cell of the other class is its own site: not its turn)
        v = cell * s - f(0.5) * cell
        const = none | ~(v < f(1)) if sign > 0 else none
        val = np.where(const, f(1), v) * f(sign)
        gx = np.where(const, f(0), (dx * sign).astype(f) / s)
        gy = np.where(const, f(0), (dy * sign).astype(f) / s)
        for k, a in enumerate((val, gx, gy)):
            tex[..., k][own] = a[own]
    return tex


def _nearest_cell_sdf(x, tex):
    """The texture's value at points x [..., 2] by GridMapSDF's cell lookup (grid_map_sdf.py:81-99), as every consumer of the texture reads it."""
    lo, hi = torch.tensor(LIMITS[0]), torch.tensor(LIMITS[1])
    dims = torch.tensor(tex.shape[:2])
    idx = torch.floor((x - lo) / (hi - lo) * dims.to(torch.float32)).long()
    idx = torch.minimum(torch.maximum(idx, torch.zeros_like(dims)), dims - 1)
    return torch.from_numpy(tex[..., 0])[idx[..., 0], idx[..., 1]]


def _checked_map_name(name, what):
    if not isinstance(name, str) or not name:
        raise ValueError(f"{what}: a non-empty string name, got {name!r}")
    if name in MAP_BOXES:
        raise ValueError(f"{what}: {name!r} is a shipped map")
    if _EXTRA_SUFFIX in name:
        raise ValueError(f"{what}: {name!r} contains {_EXTRA_SUFFIX!r}, which is stripped from map names")


def register_occupancy_map(name, occupancy):
    """A map given as a bitmap of the tile's cells: occupancy [400, 400] (grid_shape()), non-zero = occupied, indexed [ix, iy] like the SDF
    texture (x along the first axis; occupancy_from_ascii and resize_occupancy bring a text grid there).  Usable wherever a map name is;
    the name rules are register_map's, and both kinds share the names: the same bitmap under a name twice is a no-op, other content under a
    taken name -- of either kind -- is refused."""
    _checked_map_name(name, "register_occupancy_map")
    content = _checked_occupancy(occupancy, "register_occupancy_map", grid_shape()).tobytes()
    _refuse_world_name(name, "register_occupancy_map")
    if name in _REGISTERED:
        raise ValueError(f"register_occupancy_map: {name!r} is registered as a map of primitives")
    if name in _OCCUPANCY and _OCCUPANCY[name] != content:
        raise ValueError(f"register_occupancy_map: {name!r} is registered with another bitmap (update_occupancy_map replaces it)")
    _OCCUPANCY[name] = content


def map_occupancy(name):
    """The bitmap of a registered occupancy map: a uint8 [nx, ny] copy, 1 = occupied."""
    base = _base_name(name)
    if base not in _OCCUPANCY:
        raise ValueError(f"map_occupancy: {name!r} is not a registered occupancy map")
    return np.frombuffer(_OCCUPANCY[base], np.uint8).reshape(grid_shape()).copy()


def device_occupancy_sdf_grid(occupancy, device, out=None):
    """The [nx, ny, 4] texture of the tile's bitmap `occupancy` (numpy or torch, on the host or already on `device`), built on `device` by
    mmd_sdf_grid_from_occupancy: occupancy_sdf_texture bit for bit, for the upload of 160 kB (none for a device tensor).  out= rebuilds a
    resident texture in place on the current stream."""
    from . import _lib
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    nx, ny = grid_shape()
    if out is None:
        out = torch.empty(nx, ny, 4, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (nx, ny, 4) or out.device != device:
        raise ValueError(f"device_occupancy_sdf_grid: out must be [{nx}, {ny}, 4] on {device}, got {tuple(out.shape)} on {out.device}")
    if isinstance(occupancy, torch.Tensor) and occupancy.device == device:
        if tuple(occupancy.shape) != (nx, ny):
            raise ValueError(f"device_occupancy_sdf_grid: an occupancy bitmap of shape [{nx}, {ny}], got {list(occupancy.shape)}")
        occ = (occupancy != 0).to(torch.uint8).contiguous()
    else:
        host = occupancy.cpu().numpy() if isinstance(occupancy, torch.Tensor) else occupancy
        occ = torch.from_numpy(_checked_occupancy(host, "device_occupancy_sdf_grid", (nx, ny))).to(device)
    return _occupancy_build(occ, out)


def _occupancy_build(occ, out):
    """mmd_sdf_grid_from_occupancy of the uint8 device bitmap occ [nx, ny] into out [nx, ny, 4], with a workspace of its own, on the
    current stream of out's device."""
    from . import _lib
    nx, ny = occ.shape
    n_bytes = int(_lib.load().mmd_sdf_grid_occupancy_work_bytes(nx, ny))
    work = torch.empty(n_bytes, dtype=torch.uint8, device=out.device)
    _lib.launch("mmd_sdf_grid_from_occupancy", out, C.c_void_p(occ.data_ptr()), nx, ny, SDF_CELL_SIZE, _lib.require_gpu(out, "out"),
                C.c_void_p(work.data_ptr()), n_bytes)
    return out


def build_resident_texture(map_name, device, out):
    """The registered map's texture into the resident slice `out`, by the builder of its kind."""
    base = _base_name(map_name)
    if base in _OCCUPANCY:
        return device_occupancy_sdf_grid(map_occupancy(base), device, out=out)
    return device_sdf_grid(*map_primitives(map_name), device, out=out)


def update_occupancy_map(name, occupancy):
    """Replace a registered occupancy map's bitmap (numpy or torch, on the host or on a device) and rebuild every resident device texture
    slice of that name in place (same storage), on the current stream: guides and task facades that share it see the new map on their next
    call.  A bitmap that is already on a slice's device is used where it is; the registry keeps a host copy.  The host texture of the name is dropped."""
    if name in _REGISTERED:
        raise ValueError(f"update_occupancy_map: {name!r} is a map of primitives (update_map replaces those)")
    if name not in _OCCUPANCY:
        raise ValueError(f"update_occupancy_map: {name!r} is not a registered occupancy map")
    dev_occ = occupancy if isinstance(occupancy, torch.Tensor) and occupancy.is_cuda else None
    host = occupancy.cpu().numpy() if isinstance(occupancy, torch.Tensor) else occupancy
    _OCCUPANCY[name] = _checked_occupancy(host, "update_occupancy_map", grid_shape()).tobytes()
    _drop_host_texture(name)
    from . import guides
    guides.rebuild_resident_textures(name, device_occupancy=dev_occ)


def occupancy_from_ascii(rows, occupied="@OTW"):
    """The bitmap of a text grid (the MAPF benchmarks' .map body: '.' free, '@' 'O' 'T' 'W' blocked): rows[r][c] is the cell of text row r,
    column c.  Axis convention: the result is indexed [ix, iy] like the texture, with x along a text row to the right and y UP, so the
    FIRST text row is the top of the map: out[c, n_rows - 1 - r] = rows[r][c] in occupied.  Shape [n_columns, n_rows], uint8; ragged
    rows and an empty grid are refused."""
    rows = [str(r) for r in rows]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError(f"occupancy_from_ascii: rows of one non-zero length, got lengths {[len(r) for r in rows][:8]}")
    text = np.array([[ch in occupied for ch in r] for r in rows], dtype=np.uint8)            # [row, column]
    return np.ascontiguousarray(text[::-1].T)


def resize_occupancy(occ, shape=(400, 400)):
    """Nearest-neighbour resize of a bitmap to `shape` (default: the tile's grid) on integer index arithmetic: cell i of n takes
    source cell (2 i + 1) * m // (2 n) of m, the source cell that holds its centre.  uint8 out."""
    occ = _checked_occupancy(occ, "resize_occupancy")
    nx, ny = int(shape[0]), int(shape[1])
    if nx < 1 or ny < 1:
        raise ValueError(f"resize_occupancy: a shape of at least 1 x 1, got {shape}")
    jx = (2 * np.arange(nx, dtype=np.int64) + 1) * occ.shape[0] // (2 * nx)
    jy = (2 * np.arange(ny, dtype=np.int64) + 1) * occ.shape[1] // (2 * ny)
    return np.ascontiguousarray(occ[jx[:, None], jy[None, :]])


# ---- world maps: one bitmap for a world larger than a tile, a robot's map is a window of it ------------------------------------------------
# register_world_map takes a floor plan of up to OCCUPANCY_MAX_SIDE cells per side at the tile's cell pitch.  Its SDF texture is
# occupancy_sdf_texture of the whole bitmap (world_map_texture); the map of a robot whose window covers global offset + LIMITS is the
# 400 x 400 crop of that texture at the window's origin cell (world_map_windows).  The crop of the world's transform is NOT the
# transform of the cropped bitmap: an obstacle just outside a window still acts on the cells near its border, and overlapping windows
# agree where they overlap.  A window has a map name of its own (world_window_name), usable wherever a map name is.  On a device the world
# texture is resident once (guides.device_world_texture, built by mmd_sdf_grid_from_occupancy) and the windows of a map set are cut
# from it by mmd_sdf_grid_windows.  World maps have a registry of their own: registered_maps() does not list them.
_WORLD_MAPS = {}           # name -> ((WX, WY), the uint8 bitmap (0 / 1) as bytes, row-major, (origin x, origin y) as floats)
_WORLD_TEXTURE_CACHE = {}  # name -> (content the texture was built from, texture)
_WINDOW_SEPARATOR = "@"    # a window's map name: "<world>@<i0>,<j0>", the window's origin cell in the world


def _window_of(map_name):
    """(world, i0, j0) of the map name of a window of a REGISTERED world map (the last '@' splits it), else None."""
    head, sep, tail = _base_name(map_name).rpartition(_WINDOW_SEPARATOR) if isinstance(map_name, str) else ("", "", "")
    if not sep or head not in _WORLD_MAPS:
        return None
    cells = tail.split(",")
    if len(cells) != 2 or not all(c.isascii() and c.isdigit() for c in cells):
        return None
    return head, int(cells[0]), int(cells[1])


def _refuse_world_name(name, what):
    if name in _WORLD_MAPS:
        raise ValueError(f"{what}: {name!r} is registered as a world map")
    if _window_of(name) is not None:
        raise ValueError(f"{what}: {name!r} names a window of the world map {_window_of(name)[0]!r}")


def _host_array(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _world(name, what):
    if name not in _WORLD_MAPS:
        raise ValueError(f"{what}: {name!r} is not a registered world map (registered: {list(registered_world_maps())})")
    return _WORLD_MAPS[name]


def _checked_world_occupancy(occupancy, what, shape=None):
    occ = _checked_occupancy(_host_array(occupancy), what, shape)
    lo = grid_shape()
    if not all(lo[k] <= occ.shape[k] <= OCCUPANCY_MAX_SIDE for k in range(2)):
        raise ValueError(f"{what}: a world of {occ.shape[0]} x {occ.shape[1]} cells; each side holds {lo[0]} x {lo[1]} (one window) to "
                         f"{OCCUPANCY_MAX_SIDE} cells")
    return occ


def register_world_map(name, occupancy, origin=None):
    """A map larger than a tile: occupancy [WX, WY], non-zero = occupied, indexed [ix, iy] like the texture, each side between
    grid_shape() (400) and OCCUPANCY_MAX_SIDE (2048) cells of SDF_CELL_SIZE.  origin: the global position of the lower corner of cell
    (0, 0); default (-WX, -WY) * SDF_CELL_SIZE / 2, the world centred on the global origin.  The name rules are register_map's; world
    maps have a registry of their own (registered_world_maps), but the names are shared: a shipped or registered tile map's name is
    refused here, a world map's name (and the name of one of its windows) is refused by register_map and register_occupancy_map.  The
    same content under a name twice is a no-op; other content under a taken name is refused (update_world_map replaces a bitmap)."""
    _checked_map_name(name, "register_world_map")
    if _WINDOW_SEPARATOR in name and _window_of(name) is not None:
        raise ValueError(f"register_world_map: {name!r} names a window of the world map {_window_of(name)[0]!r}")
    occ = _checked_world_occupancy(occupancy, "register_world_map")
    if origin is None:
        origin = (-occ.shape[0] * SDF_CELL_SIZE / 2.0, -occ.shape[1] * SDF_CELL_SIZE / 2.0)
    org = np.asarray(_host_array(origin), dtype=np.float64).reshape(-1)
    if org.shape != (2,) or not np.isfinite(org).all():
        raise ValueError(f"register_world_map: origin = two finite numbers, got {origin!r}")
    if name in _REGISTERED or name in _OCCUPANCY:
        raise ValueError(f"register_world_map: {name!r} is registered as a tile map")
    taken = [n for n in registered_maps() if n.startswith(name + _WINDOW_SEPARATOR)]
    if name not in _WORLD_MAPS and taken:
        raise ValueError(f"register_world_map: the registered map {taken[0]!r} has the form of a window name of {name!r}")
    content = (tuple(occ.shape), occ.tobytes(), (float(org[0]), float(org[1])))
    if name in _WORLD_MAPS and _WORLD_MAPS[name] != content:
        raise ValueError(f"register_world_map: {name!r} is registered with another bitmap or origin (update_world_map replaces the bitmap)")
    _WORLD_MAPS[name] = content


def update_world_map(name, occupancy):
    """Replace a world map's bitmap (same shape, same origin).  Every resident world texture of the name is rebuilt in place and every
    resident window slice cut from it is cut again in place (same storage, same pointers), on the current stream of its device, one
    cut launch per map set: live guides and samplers see the new obstacles on their next call.  The host texture is dropped."""
    shape, _, origin = _world(name, "update_world_map")
    occ = _checked_world_occupancy(occupancy, "update_world_map", shape)
    _WORLD_MAPS[name] = (shape, occ.tobytes(), origin)
    _WORLD_TEXTURE_CACHE.pop(name, None)
    from . import guides
    guides.rebuild_world_textures(name)


def unregister_world_map(name):
    """Forget a world map, its host texture, its resident world textures and every resident map set that holds one of its windows
    (objects built on one keep theirs)."""
    _world(name, "unregister_world_map")
    from . import guides
    guides.drop_world_textures(name)            # (while the name still parses as a world's)
    del _WORLD_MAPS[name]
    _WORLD_TEXTURE_CACHE.pop(name, None)


def registered_world_maps():
    """The names of the registered world maps, sorted."""
    return tuple(sorted(_WORLD_MAPS))


def is_world_map(name):
    return isinstance(name, str) and name in _WORLD_MAPS


def is_world_window(name):
    """Whether `name` is the map name of a window of a registered world map (world_window_name)."""
    return _window_of(name) is not None


def world_window(name):
    """(world, (i0, j0)) of a window's map name."""
    w = _window_of(name)
    if w is None:
        raise ValueError(f"world_window: {name!r} is not a window of a registered world map")
    return w[0], (w[1], w[2])


def world_map_occupancy(name):
    """The bitmap of a world map: a uint8 [WX, WY] copy, 1 = occupied."""
    shape, content, _ = _world(name, "world_map_occupancy")
    return np.frombuffer(content, np.uint8).reshape(shape).copy()


def world_map_origin(name):
    """The global position of the lower corner of cell (0, 0)."""
    return _world(name, "world_map_origin")[2]


def world_map_limits(name):
    """(lo, hi), global: the lower corner of cell (0, 0) and the upper corner of the last cell."""
    shape, _, origin = _world(name, "world_map_limits")
    return origin, tuple(origin[k] + shape[k] * SDF_CELL_SIZE for k in range(2))


def world_map_texture(name):
    """float32 [WX, WY, 4]: occupancy_sdf_texture of the world's bitmap, THE DEFINITION of the world's texture.  Cached by content
    (seconds in numpy at 640 x 520, minutes at 2048 x 2048: the resident device texture is the practical one at full size)."""
    _, content, _ = _world(name, "world_map_texture")
    hit = _WORLD_TEXTURE_CACHE.get(name)
    if hit is None or hit[0] != content:
        hit = _WORLD_TEXTURE_CACHE[name] = (content, occupancy_sdf_texture(world_map_occupancy(name)))
    return hit[1]


def _checked_window_origins(name, origins, what):
    """int32 [n, 2] origin cells, each a window that lies inside the world"""
    shape = _world(name, what)[0]
    raw = _host_array(origins)
    org = raw.reshape(-1, 2)
    if raw.size == 0 or org.dtype.kind not in "iu":
        raise ValueError(f"{what}: origins [n, 2] of integer cells, got dtype {raw.dtype}, shape {raw.shape}")
    n = grid_shape()
    bad = np.flatnonzero(((org < 0) | (org > np.asarray([shape[0] - n[0], shape[1] - n[1]]))).any(1))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{what}: window {k} at origin cell {org[k].tolist()} is outside the world {name!r}: origins 0 .. "
                         f"{[shape[0] - n[0], shape[1] - n[1]]}")
    return np.ascontiguousarray(org, dtype=np.int32)


def world_map_windows(name, origins):
    """float32 [n, 400, 400, 4]: window k is world_map_texture(name)[i0:i0 + 400, j0:j0 + 400] for origins[k] = (i0, j0), a copy, bit for
    bit: THE DEFINITION of a window's texture.  Origins outside [0, W - 400] are refused."""
    org = _checked_window_origins(name, origins, "world_map_windows")
    tex = world_map_texture(name)
    nx, ny = grid_shape()
    return np.stack([tex[i0:i0 + nx, j0:j0 + ny] for i0, j0 in org.tolist()])


def _window_cells(name, offsets, what):
    """(q, shape): the windows' origins in cells, float64 [n, 2], not yet rounded -- q = (offset + LIMITS[0] - origin) / cell"""
    shape, _, origin = _world(name, what)
    off = np.asarray(_host_array(offsets), dtype=np.float64)
    if off.size == 0 or off.shape[-1] != 2:
        raise ValueError(f"{what}: offsets [n, 2], got shape {off.shape}")
    return (off.reshape(-1, 2) + np.asarray(LIMITS[0], np.float64) - np.asarray(origin, np.float64)) / np.float64(SDF_CELL_SIZE), shape


def world_map_window_origins(name, offsets):
    """int32 [N, 2]: the origin cells of the robots' windows.  Robot r's window covers global offsets[r] + LIMITS, so its origin is
    (offset + LIMITS[0] - origin) / SDF_CELL_SIZE per axis, in float64.  It must lie within 1e-3 of an integer (float32 offsets that are
    multiples of the cell pitch are not exact; half a cell off is an error) and inside [0, W - 400]; otherwise ValueError names the
    first robot at fault and whether it is off the cell grid or outside the world.  snap_to_world_map gives offsets that pass."""
    q, shape = _window_cells(name, offsets, "world_map_window_origins")
    r = np.rint(q)
    n = grid_shape()
    with np.errstate(invalid="ignore"):
        off_grid = ~(np.abs(q - r) <= 1e-3)
        outside = ~off_grid & ((r < 0) | (r > np.asarray([shape[0] - n[0], shape[1] - n[1]], np.float64)))
    bad = np.flatnonzero((off_grid | outside).any(1))
    if bad.size:
        k = int(bad[0])
        if off_grid[k].any():
            raise ValueError(f"world_map_window_origins: the window of robot {k} is off the cell grid of {name!r}: its origin is at cell "
                             f"{q[k].tolist()} (snap_to_world_map gives the nearest valid offsets)")
        raise ValueError(f"world_map_window_origins: the window of robot {k} is outside the world {name!r}: its origin cell "
                         f"{r[k].astype(np.int64).tolist()} is not in 0 .. {[shape[0] - n[0], shape[1] - n[1]]}")
    return r.astype(np.int32)


def snap_to_world_map(name, offsets):
    """float32 offsets of the shape given: per robot the nearest offsets whose window starts on a cell and lies inside the world."""
    q, shape = _window_cells(name, offsets, "snap_to_world_map")
    if not np.isfinite(q).all():
        raise ValueError("snap_to_world_map: every offset must be finite")
    n = grid_shape()
    cells = np.clip(np.rint(q), 0, np.asarray([shape[0] - n[0], shape[1] - n[1]], np.float64))
    origin = np.asarray(_WORLD_MAPS[name][2], np.float64)
    out = cells * np.float64(SDF_CELL_SIZE) + origin - np.asarray(LIMITS[0], np.float64)
    return out.astype(np.float32).reshape(np.shape(_host_array(offsets)))


def world_window_name(name, offset_or_origin):
    """The map name of one window of the world map `name`, usable wherever a map name is (GuideManagerTrajectoriesWithVelocity env_id /
    robot_env_ids, MPD env_id, MPDEnsemble env_ids, MultiRobotSampler env_id): "<name>@<i0>,<j0>".  offset_or_origin: two INTEGERS are the
    window's origin cell (i0, j0); two floats are a robot's offset (world_map_window_origins' rules apply).  Windows at equal origins have
    equal names and share a resident slice."""
    a = _host_array(offset_or_origin)
    if a.size != 2:
        raise ValueError(f"world_window_name: one offset (x, y) or one origin cell (i0, j0), got shape {a.shape}")
    if a.dtype.kind in "iu":
        i0, j0 = _checked_window_origins(name, a.reshape(1, 2), "world_window_name")[0].tolist()
    else:
        i0, j0 = world_map_window_origins(name, a.reshape(1, 2))[0].tolist()
    return f"{name}{_WINDOW_SEPARATOR}{i0},{j0}"


def _texel_indices(points, lo, hi, shape):
    """(ix, iy, finite): the texel of float32 points [n, 2] on a grid of `shape` over lo .. hi, the fp32 sequence of every consumer of a
    texture and of mmd_sdf_grid_lookup: floor((p - lo) / |hi - lo| * n) clamped to [0, n - 1] (as a float, then converted)."""
    f = np.float32
    lo, hi = np.asarray(lo, f), np.asarray(hi, f)
    dim = np.abs(hi - lo)
    finite = np.isfinite(points).all(1)
    p = np.where(finite[:, None], points, f(0))
    with np.errstate(over="ignore"):
        idx = [np.clip(np.floor((p[:, k] - lo[k]) / dim[k] * f(shape[k])), f(0), f(shape[k] - 1)).astype(np.int64) for k in range(2)]
    return idx[0], idx[1], finite


def world_map_sdf(points_global, name, device=None):
    """The world texture's nearest-cell value at global points [..., 2] -> float32 [...], NaN at a point with a non-finite coordinate.
    device=None: on the host texture (world_map_texture: slow to build at full world size), a CPU tensor.  With a device: read off the
    resident world texture by mmd_sdf_grid_lookup, a tensor on that device -- the practical source of truth for "is this start free"."""
    shape = _world(name, "world_map_sdf")[0]
    lo, hi = world_map_limits(name)
    if device is None:
        pts = np.ascontiguousarray(_host_array(points_global), dtype=np.float32)
        ix, iy, finite = _texel_indices(pts.reshape(-1, 2), lo, hi, shape)
        val = np.where(finite, world_map_texture(name)[ix, iy, 0], np.float32(np.nan))
        return torch.from_numpy(np.ascontiguousarray(val.reshape(pts.shape[:-1]), dtype=np.float32))
    from . import _lib, guides
    tex = guides.device_world_texture(name, device)
    pts = torch.as_tensor(points_global, dtype=torch.float32).to(tex.device).contiguous()
    flat = pts.reshape(-1, 2)
    out = torch.empty(flat.shape[0], 4, dtype=torch.float32, device=tex.device)
    _lib.launch("mmd_sdf_grid_lookup", tex, _lib.require_gpu(tex, "world texture"), shape[0], shape[1], (C.c_float * 2)(*lo),
                (C.c_float * 2)(*hi), _lib.require_gpu(flat, "points"), flat.shape[0], _lib.require_gpu(out, "out"))
    return out[:, 0].reshape(pts.shape[:-1])


def device_world_sdf_grid(name, device, out=None):
    """The [WX, WY, 4] texture of the world map `name`, built on `device` by mmd_sdf_grid_from_occupancy: world_map_texture bit for
    bit, for the upload of one byte per cell.  out= rebuilds a resident texture in place on the current stream."""
    shape = _world(name, "device_world_sdf_grid")[0]
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty(shape[0], shape[1], 4, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (shape[0], shape[1], 4) or out.device != device:
        raise ValueError(f"device_world_sdf_grid: out must be [{shape[0]}, {shape[1]}, 4] on {device}, got {tuple(out.shape)} on {out.device}")
    return _occupancy_build(torch.from_numpy(world_map_occupancy(name)).to(device), out)
