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
    primitives or occupied cells: update_map / update_occupancy_map may give it some while a guide that reads the grid is alive."""
    base = _base_name(name)
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
    if base in _OCCUPANCY:
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
    n_bytes = int(_lib.load().mmd_sdf_grid_occupancy_work_bytes(nx, ny))
    work = torch.empty(n_bytes, dtype=torch.uint8, device=device)
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
