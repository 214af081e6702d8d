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
the resident texture is built by mmd_sdf_grid_from_occupancy, bit for bit the same.

World maps (register_world_map): one bitmap for a world larger than a tile, up to 2048 cells per side.  The world's texture is
occupancy_sdf_texture of the whole bitmap; a robot's map is the 400 x 400 window of it at the robot's offset (world_map_windows is the
definition, world_window_name its map name); on a device the windows are cut from the resident world texture by mmd_sdf_grid_windows.

The shipped maps are the constant table MAP_BOXES; the three registered kinds share ONE registry and one name space, and resolve_map is
the one reading of a map name: what differs per kind is a `match` on the kind it returns.  The host textures of every kind share one
cache keyed by content.  The textures resident on a device, and what an update or an unregistration does to them, are map_textures.py's.
"""
import ctypes as C
from typing import NamedTuple

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
OCCUPANCY_MAX_SIDE = 2048  # MMD_OCCUPANCY_MAX_SIDE: 2 * 2047^2 < 2^24, so every squared distance is an exact float32


# ---- the registry and the map names ---------------------------------------------------------------------------------------------------
class MapRecord(NamedTuple):
    kind: str              # "primitives" | "occupancy" (the tile kinds: registered_maps) | "world" (registered_world_maps)
    content: object        # hashable; "the same content under a name twice is a no-op" compares it, and so does the host texture cache:
    #                        primitives: (boxes, spheres), tuples of float tuples rounded to fp32; occupancy: the [nx, ny] uint8 bitmap
    #                        (0 / 1) as bytes, row-major; world: ((WX, WY), its bitmap as bytes, (origin x, origin y) as floats)


_TILE_KINDS = ("primitives", "occupancy")
# kind -> (what a refusal calls it, what register_* calls other content under a taken name, the two calls that take a map of the kind)
_KINDS = {"primitives": ("map of primitives", "other primitives", "update_map", "unregister_map"),
          "occupancy": ("occupancy map", "another bitmap", "update_occupancy_map", "unregister_map"),
          "world": ("world map", "another bitmap or origin", "update_world_map", "unregister_world_map")}
_MAPS = {}                 # name -> MapRecord
_EXTRA_SUFFIX = "ExtraObjects"
_WINDOW_SEPARATOR = "@"    # a window's map name: "<world>@<i0>,<j0>", the window's origin cell in the world


def resolve_map(map_name, unknown_ok=False):
    """(kind, base name, record, window origin) of a map name, the one reading of it.  The suffix 'ExtraObjects' is stripped from every
    name.  kind "shipped": a key of MAP_BOXES (record None); "primitives" / "occupancy": a registered tile map and its record; "window":
    "<world>@<i0>,<j0>" of a REGISTERED world map, split at the last '@' -- the base name is the world's, the record the world's, the
    origin (i0, j0), elsewhere None.  Any other name, a world map's own among them, and anything that is no string: KeyError, or four
    times None with unknown_ok (the predicates)."""
    if isinstance(map_name, str):
        base = map_name.replace(_EXTRA_SUFFIX, "")
        if base in MAP_BOXES:
            return "shipped", base, None, None
        rec = _MAPS.get(base)
        if rec is not None and rec.kind in _TILE_KINDS:
            return rec.kind, base, rec, None
        world, _, tail = base.rpartition(_WINDOW_SEPARATOR)
        cells = tail.split(",")
        rec = _MAPS.get(world)
        if rec is not None and rec.kind == "world" and len(cells) == 2 and all(c.isascii() and c.isdigit() for c in cells):
            return "window", world, rec, (int(cells[0]), int(cells[1]))
    if unknown_ok:
        return None, None, None, None
    raise KeyError(f"unknown map {map_name!r} (shipped: {sorted(MAP_BOXES)}; registered: {list(registered_maps())}; windows of the "
                   f"world maps {list(registered_world_maps())})")


def is_registered(name):
    return resolve_map(name, True)[0] in _TILE_KINDS


def is_occupancy_map(name):
    return resolve_map(name, True)[0] == "occupancy"


def is_world_window(name):
    """Whether `name` is the map name of a window of a registered world map (world_window_name)."""
    return resolve_map(name, True)[0] == "window"


def is_world_map(name):
    return isinstance(name, str) and name in _MAPS and _MAPS[name].kind == "world"


def registered_maps():
    """The names of the registered tile maps of both kinds, sorted."""
    return tuple(sorted(n for n, rec in _MAPS.items() if rec.kind in _TILE_KINDS))


def registered_world_maps():
    """The names of the registered world maps, sorted."""
    return tuple(sorted(n for n, rec in _MAPS.items() if rec.kind == "world"))


def _register(what, name, kind, content):
    """The name rules and the clash rule of every register_*.  A new name is a non-empty string, no shipped name, without 'ExtraObjects'.
    A name belongs to at most ONE kind, a window's name to its world: a name taken by another kind is refused, a tile or world name may
    not be a window name of a registered world, and a world may not be registered while a tile map's name begins "<world>@".  The same
    content under a taken name is a no-op, other content is refused."""
    if not isinstance(name, str) or not name:
        raise ValueError(f"{what}: a non-empty string name, got {name!r}")
    if name in MAP_BOXES:
        raise ValueError(f"{what}: {name!r} is a shipped map")
    if _EXTRA_SUFFIX in name:
        raise ValueError(f"{what}: {name!r} contains {_EXTRA_SUFFIX!r}, which is stripped from map names")
    content = content()                                     # (checked only under a name that may be registered at all)
    taken = _MAPS.get(name)
    if taken is not None and taken.kind != kind:
        raise ValueError(f"{what}: {name!r} is the name of a registered {_KINDS[taken.kind][0]}{', a tile map' * (taken.kind in _TILE_KINDS)}")
    if is_world_window(name):
        raise ValueError(f"{what}: {name!r} names a window of the world map {world_window(name)[0]!r}")
    tiles = [n for n in registered_maps() if n.startswith(name + _WINDOW_SEPARATOR)] if kind == "world" and taken is None else []
    if tiles:
        raise ValueError(f"{what}: the registered map {tiles[0]!r} has the form of a window name of {name!r}")
    if taken is not None and taken.content != content:
        raise ValueError(f"{what}: {name!r} is registered with {_KINDS[kind][1]} ({_KINDS[kind][2]} replaces the content)")
    _MAPS[name] = MapRecord(kind, content)


def _record(what, name, *kinds):
    """The record of `name`, which must be registered as one of `kinds`; the refusal names the calls that take the kind it is."""
    rec = _MAPS.get(name) if isinstance(name, str) else None
    if rec is None or rec.kind not in kinds:
        has = "" if rec is None else ": it is a registered {0}, which {2} and {3} take".format(*_KINDS[rec.kind])
        raise ValueError(f"{what}: {name!r} is not a registered {' or '.join(_KINDS[k][0] for k in kinds)}{has}")
    return rec


def _resident():
    """The textures resident on the devices (map_textures.py): the one place this module reaches them."""
    from . import map_textures
    return map_textures


def _replace(name, content, **how):
    """update_*: the new content, no host texture of the old one, and every resident texture that holds the name rebuilt in place."""
    _MAPS[name] = MapRecord(_MAPS[name].kind, content)
    _drop_host_texture(name)
    _resident().rebuild_resident_textures(name, **how)


def _forget(name):
    """unregister_*: the resident textures that hold the name go while it still resolves, then its host texture and the name itself."""
    _resident().drop_resident_textures(name)
    _drop_host_texture(name)
    del _MAPS[name]


# ---- maps of primitives -----------------------------------------------------------------------------------------------------------------
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
    _register("register_map", name, "primitives", lambda: _checked_primitives(boxes, spheres))


def update_map(name, boxes=(), spheres=()):
    """Replace a registered map's primitives and rebuild every resident device texture slice of that name in place (same storage): guides
    and task facades that share it see the new map on their next call.  The host texture of the name is dropped."""
    _record("update_map", name, "primitives")
    _replace(name, _checked_primitives(boxes, spheres))


def unregister_map(name):
    """Forget a registered map of either kind, its host texture and every resident device texture that holds it (objects built on it
    keep theirs)."""
    _record("unregister_map", name, *_TILE_KINDS)
    _forget(name)


def map_primitives(name):
    """(boxes [(cx, cy, size_x, size_y)], spheres [(cx, cy, r)]) of a shipped or registered map."""
    kind, base, rec, _ = resolve_map(name)
    match kind:
        case "shipped":
            return tuple((float(c[0]), float(c[1]), float(s[0]), float(s[1])) for c, s in zip(*MAP_BOXES[base])), ()
        case "primitives":
            return rec.content
        case "occupancy":
            raise ValueError(f"map_primitives: {name!r} is an occupancy map (map_occupancy returns its bitmap)")
        case "window":
            raise ValueError(f"map_primitives: {name!r} is a window of a world map (world_map_occupancy returns the world's bitmap)")


def map_has_obstacles(name):
    """Whether the map's fixed objects have an SDF grid (mmd_guide_desc.n_grids = 1).  A registered map always has one, even without
    primitives or occupied cells: update_map / update_occupancy_map may give it some while a guide that reads the grid is alive.
    A window of a world map: whether the world has an occupied cell now (a guide built on a window of an empty world reads no grid, and
    an update_world_map that adds the first obstacle does not reach it)."""
    kind, base, rec, _ = resolve_map(name)
    if kind == "window":
        return b"\x01" in rec.content[1]
    return kind != "shipped" or len(MAP_BOXES[base][0]) > 0


def _rounded_box_sdfs(x, centers, sizes):
    """MultiRoundedBoxField.compute_signed_distance_impl before its min over the boxes (primitives.py:324-332)."""
    radius = torch.min(sizes, dim=-1)[0] * 0.15
    q = torch.abs(x.unsqueeze(-2) - centers.unsqueeze(0)) - (sizes / 2).unsqueeze(0) + radius.unsqueeze(0).unsqueeze(-1)
    max_q = torch.amax(q, dim=-1)
    return torch.minimum(max_q, torch.zeros_like(max_q)) + torch.linalg.norm(torch.relu(q), dim=-1) - radius.unsqueeze(0)


def _primitives_sdf(x, boxes, spheres):
    """ObjectField([MultiSphereField(spheres), MultiBoxField(boxes)]) at the identity pose (primitives.py:108-115, :326-333, :569-572):
    torch.min over the stacked fields, spheres first, so the first of equal minima takes the gradient; an empty sphere field is the
    constant 1, an empty box field is left out.  The shipped maps are their boxes and no spheres."""
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
    """The map's SDF at points [..., 2] -> float32 tensor [...]: the analytic field of a map of primitives, shipped or registered; the
    nearest-cell value of the host texture (texel_values) of an occupancy map or a window, which have no analytic field."""
    if resolve_map(map_name)[0] in ("shipped", "primitives"):
        return _primitives_sdf(torch.as_tensor(points, dtype=torch.float32), *map_primitives(map_name))
    return torch.from_numpy(texel_values(sdf_grid_texture(map_name), points)[0])


def grid_shape(cell_size=SDF_CELL_SIZE):
    lo, hi = torch.tensor(LIMITS[0]), torch.tensor(LIMITS[1])
    cmap = torch.ceil(torch.abs(hi - lo) / cell_size).long()
    return int(cmap[0]), int(cmap[1])


def grid_node_rows(cell_size=SDF_CELL_SIZE):
    """The node coordinates of the grid per axis, torch.linspace on the CPU as GridMapSDF.precompute_sdf computes them."""
    lo, hi = torch.tensor(LIMITS[0]), torch.tensor(LIMITS[1])
    nx, ny = grid_shape(cell_size)
    return torch.linspace(lo[0], hi[0], nx), torch.linspace(lo[1], hi[1], ny)


# ---- host textures ------------------------------------------------------------------------------------------------------------------------
_HOST_TEXTURES = {}        # (tile map's base name or world map's name, cell size) -> (content the texture was built from, texture)


def _host_texture(name, cell_size, content, build):
    hit = _HOST_TEXTURES.get((name, cell_size))
    if hit is None or hit[0] != content:
        hit = _HOST_TEXTURES[(name, cell_size)] = (content, build())
    return hit[1]


def _drop_host_texture(name):
    for key in [k for k in _HOST_TEXTURES if k[0] == name]:
        del _HOST_TEXTURES[key]


def sdf_grid_texture(map_name, cell_size=SDF_CELL_SIZE):
    """float32 numpy [nx, ny, 4] = (sdf, dsdf/dx, dsdf/dy, 0): the texture layout mmd_guide_desc expects."""
    kind, base, rec, origin = resolve_map(map_name)
    if kind in ("occupancy", "window") and grid_shape(cell_size) != grid_shape():
        raise ValueError(f"sdf_grid_texture: the {_KINDS[rec.kind][0]} {base!r} has one cell per grid cell at {SDF_CELL_SIZE}, not at "
                         f"{cell_size}")
    match kind:
        case "window":                                           # (the host crop of the world's texture, which is cached by content)
            return world_map_windows(base, [origin])[0]
        case "occupancy":
            return _host_texture(base, cell_size, rec.content, lambda: occupancy_sdf_texture(map_occupancy(base), cell_size))
    prims = map_primitives(base)                                 # (a shipped map's content never changes: None)
    return _host_texture(base, cell_size, rec and rec.content,
                         lambda: _texture(lambda pts: _primitives_sdf(pts, *prims), *grid_node_rows(cell_size)))


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


def _host_array(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


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


def texel_values(tex, points, lo=LIMITS[0], hi=LIMITS[1]):
    """(values, finite), float32 and bool numpy [...]: channel 0 of texture `tex` [nx, ny, 4] over lo .. hi at the texel of every point
    [..., 2] (GridMapSDF's cell lookup, grid_map_sdf.py:81-99, by _texel_indices), THE host lookup of a texture: a point however far out
    reads the clamped border cell, as on the device; a point with a non-finite coordinate reads as point 0 and has finite = False."""
    pts = np.ascontiguousarray(_host_array(points), dtype=np.float32)
    ix, iy, finite = _texel_indices(pts.reshape(-1, 2), lo, hi, tex.shape[:2])
    return tex[ix, iy, 0].reshape(pts.shape[:-1]), finite.reshape(pts.shape[:-1])


# ---- the grid on the device ---------------------------------------------------------------------------------------
_NODE_ROWS_DEV = {}        # device -> (xs, ys) of the tile's grid


def resolved_device(device):
    """torch.device(device), a 'cuda' without an index resolved to the current device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _out_texture(what, shape, device, out):
    """(device, out): the device resolved; `out` allocated as the float32 texture [shape[0], shape[1], 4] there, or checked to be one."""
    device = resolved_device(device)
    if out is None:
        out = torch.empty(shape[0], shape[1], 4, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (shape[0], shape[1], 4) or out.device != device:
        raise ValueError(f"{what}: out must be [{shape[0]}, {shape[1]}, 4] on {device}, got {tuple(out.shape)} on {out.device}")
    return device, out


def primitive_table_layout(boxes, spheres):
    """The library's tables of float32 boxes [n, 4] = (cx, cy, size_x, size_y) and spheres [n, 3] = (cx, cy, r): boxes [n][4] = (cx, cy,
    half x, half y), spheres [n][4] = (cx, cy, r, 0) -- mmd_guide_desc's extra_boxes_dev / extra_spheres_dev layouts.  Layout only."""
    return (np.concatenate([boxes[:, :2], boxes[:, 2:] / np.float32(2)], 1),
            np.concatenate([spheres, np.zeros((len(spheres), 1), np.float32)], 1))


def primitive_tables(boxes, spheres):
    """(boxes, spheres) checked as register_map checks them, in the library's layouts (primitive_table_layout), as float32 numpy."""
    boxes, spheres = _checked_primitives(boxes, spheres)
    return primitive_table_layout(np.asarray(boxes, dtype=np.float32).reshape(-1, 4), np.asarray(spheres, dtype=np.float32).reshape(-1, 3))


def device_sdf_grid(boxes, spheres, device, out=None):
    """The [nx, ny, 4] texture of a map of these primitives, built on `device` by mmd_sdf_grid_build: what sdf_grid_texture computes on the
    host, bit for bit but for the sign of a zero (+0 here), for the upload of the primitives and the two rows of node coordinates.  out= rebuilds a resident texture in place
    on the current stream."""
    from . import _lib
    nx, ny = grid_shape()
    device, out = _out_texture("device_sdf_grid", (nx, ny), device, out)
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


def build_resident_texture(map_name, device, out):
    """The registered map's texture into the resident slice `out`, by the builder of its kind."""
    kind, _, rec, _ = resolve_map(map_name)
    match kind:
        case "primitives":
            return device_sdf_grid(*rec.content, device, out=out)
        case "occupancy":
            return device_occupancy_sdf_grid(_bitmap(rec.content, grid_shape()), device, out=out)
    raise ValueError(f"build_resident_texture: {map_name!r} is no registered tile map")


# ---- occupancy maps -------------------------------------------------------------------------------------------------
_OCC_NONE = 1 << 14        # "this row holds no such cell": its square is above every real squared distance (csrc/sdf_grid.hip: OCC_NONE)


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


def _bitmap(content, shape):
    """The uint8 [nx, ny] bitmap (1 = occupied) a registry record holds as bytes, read-only"""
    return np.frombuffer(content, np.uint8).reshape(shape)


def register_occupancy_map(name, occupancy):
    """A map given as a bitmap of the tile's cells: occupancy [400, 400] (grid_shape()), non-zero = occupied, indexed [ix, iy] like the SDF
    texture (x along the first axis; occupancy_from_ascii and resize_occupancy bring a text grid there).  Usable wherever a map name is;
    the name rules are register_map's, and both kinds share the names: the same bitmap under a name twice is a no-op, other content under a
    taken name -- of either kind -- is refused."""
    _register("register_occupancy_map", name, "occupancy",
              lambda: _checked_occupancy(occupancy, "register_occupancy_map", grid_shape()).tobytes())


def map_occupancy(name):
    """The bitmap of a registered occupancy map: a uint8 [nx, ny] copy, 1 = occupied."""
    kind, _, rec, _ = resolve_map(name, True)
    if kind != "occupancy":
        raise ValueError(f"map_occupancy: {name!r} is not a registered occupancy map")
    return _bitmap(rec.content, grid_shape()).copy()


def device_occupancy_sdf_grid(occupancy, device, out=None):
    """The [nx, ny, 4] texture of the tile's bitmap `occupancy` (numpy or torch, on the host or already on `device`), built on `device` by
    mmd_sdf_grid_from_occupancy: occupancy_sdf_texture bit for bit, for the upload of 160 kB (none for a device tensor).  out= rebuilds a
    resident texture in place on the current stream."""
    nx, ny = grid_shape()
    device, out = _out_texture("device_occupancy_sdf_grid", (nx, ny), device, out)
    if isinstance(occupancy, torch.Tensor) and occupancy.device == device:
        if tuple(occupancy.shape) != (nx, ny):
            raise ValueError(f"device_occupancy_sdf_grid: an occupancy bitmap of shape [{nx}, {ny}], got {list(occupancy.shape)}")
        occ = (occupancy != 0).to(torch.uint8).contiguous()
    else:
        occ = torch.from_numpy(_checked_occupancy(_host_array(occupancy), "device_occupancy_sdf_grid", (nx, ny))).to(device)
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


def update_occupancy_map(name, occupancy):
    """Replace a registered occupancy map's bitmap (numpy or torch, on the host or on a device) and rebuild every resident device texture
    slice of that name in place (same storage), on the current stream: guides and task facades that share it see the new map on their next
    call.  A bitmap that is already on a slice's device is used where it is; the registry keeps a host copy.  The host texture of the name is dropped."""
    _record("update_occupancy_map", name, "occupancy")
    dev_occ = occupancy if isinstance(occupancy, torch.Tensor) and occupancy.is_cuda else None
    _replace(name, _checked_occupancy(_host_array(occupancy), "update_occupancy_map", grid_shape()).tobytes(), device_occupancy=dev_occ)


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
# texture is resident once (map_textures.device_world_texture, built by mmd_sdf_grid_from_occupancy) and the windows of a map set are cut
# from it by mmd_sdf_grid_windows.  registered_maps() does not list the world maps.
def _world(name, what):
    """(shape, bitmap as bytes, origin) of a registered world map"""
    return _record(what, name, "world").content


def _max_origin(shape):
    """The largest window origin of a world of `shape` cells, per axis"""
    n = grid_shape()
    return [shape[0] - n[0], shape[1] - n[1]]


def _checked_world_occupancy(occupancy, what, shape=None):
    occ = _checked_occupancy(_host_array(occupancy), what, shape)
    lo = grid_shape()
    if not all(lo[k] <= occ.shape[k] <= OCCUPANCY_MAX_SIDE for k in range(2)):
        raise ValueError(f"{what}: a world of {occ.shape[0]} x {occ.shape[1]} cells; each side holds {lo[0]} x {lo[1]} (one window) to "
                         f"{OCCUPANCY_MAX_SIDE} cells")
    return occ


def _world_content(occupancy, origin):
    occ = _checked_world_occupancy(occupancy, "register_world_map")
    if origin is None:
        origin = (-occ.shape[0] * SDF_CELL_SIZE / 2.0, -occ.shape[1] * SDF_CELL_SIZE / 2.0)
    org = np.asarray(_host_array(origin), dtype=np.float64).reshape(-1)
    if org.shape != (2,) or not np.isfinite(org).all():
        raise ValueError(f"register_world_map: origin = two finite numbers, got {origin!r}")
    return tuple(occ.shape), occ.tobytes(), (float(org[0]), float(org[1]))


def register_world_map(name, occupancy, origin=None):
    """A map larger than a tile: occupancy [WX, WY], non-zero = occupied, indexed [ix, iy] like the texture, each side between
    grid_shape() (400) and OCCUPANCY_MAX_SIDE (2048) cells of SDF_CELL_SIZE.  origin: the global position of the lower corner of cell
    (0, 0); default (-WX, -WY) * SDF_CELL_SIZE / 2, the world centred on the global origin.  The name rules are register_map's; world
    maps are listed apart (registered_world_maps), but the names are shared: a shipped or registered tile map's name is
    refused here, a world map's name (and the name of one of its windows) is refused by register_map and register_occupancy_map.  The
    same content under a name twice is a no-op; other content under a taken name is refused (update_world_map replaces a bitmap)."""
    _register("register_world_map", name, "world", lambda: _world_content(occupancy, origin))


def update_world_map(name, occupancy):
    """Replace a world map's bitmap (same shape, same origin).  Every resident world texture of the name is rebuilt in place and every
    resident window slice cut from it is cut again in place (same storage, same pointers), on the current stream of its device, one
    cut launch per map set: live guides and samplers see the new obstacles on their next call.  The host texture is dropped."""
    shape, _, origin = _world(name, "update_world_map")
    _replace(name, (shape, _checked_world_occupancy(occupancy, "update_world_map", shape).tobytes(), origin))


def unregister_world_map(name):
    """Forget a world map, its host texture, its resident world textures and every resident map set that holds one of its windows
    (objects built on one keep theirs)."""
    _world(name, "unregister_world_map")
    _forget(name)


def world_window(name):
    """(world, (i0, j0)) of a window's map name."""
    kind, world, _, origin = resolve_map(name, True)
    if kind != "window":
        raise ValueError(f"world_window: {name!r} is not a window of a registered world map")
    return world, origin


def world_map_occupancy(name):
    """The bitmap of a world map: a uint8 [WX, WY] copy, 1 = occupied."""
    shape, content, _ = _world(name, "world_map_occupancy")
    return _bitmap(content, shape).copy()


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
    content = _world(name, "world_map_texture")
    return _host_texture(name, SDF_CELL_SIZE, content, lambda: occupancy_sdf_texture(world_map_occupancy(name)))


def checked_window_origins(name, origins, what):
    """int32 [n, 2] origin cells, each a window that lies inside the world; `what` names the caller in a refusal"""
    limit = _max_origin(_world(name, what)[0])
    raw = _host_array(origins)
    org = raw.reshape(-1, 2)
    if raw.size == 0 or org.dtype.kind not in "iu":
        raise ValueError(f"{what}: origins [n, 2] of integer cells, got dtype {raw.dtype}, shape {raw.shape}")
    bad = np.flatnonzero(((org < 0) | (org > np.asarray(limit))).any(1))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{what}: window {k} at origin cell {org[k].tolist()} is outside the world {name!r}: origins 0 .. {limit}")
    return np.ascontiguousarray(org, dtype=np.int32)


def world_map_windows(name, origins):
    """float32 [n, 400, 400, 4]: window k is world_map_texture(name)[i0:i0 + 400, j0:j0 + 400] for origins[k] = (i0, j0), a copy, bit for
    bit: THE DEFINITION of a window's texture.  Origins outside [0, W - 400] are refused."""
    org = checked_window_origins(name, origins, "world_map_windows")
    tex = world_map_texture(name)
    nx, ny = grid_shape()
    return np.stack([tex[i0:i0 + nx, j0:j0 + ny] for i0, j0 in org.tolist()])


def _window_cells(name, offsets, what):
    """(q, limit): the windows' origins in cells, float64 [n, 2], not yet rounded -- q = (offset + LIMITS[0] - origin) / cell -- and the
    largest origin of the world"""
    shape, _, origin = _world(name, what)
    off = np.asarray(_host_array(offsets), dtype=np.float64)
    if off.size == 0 or off.shape[-1] != 2:
        raise ValueError(f"{what}: offsets [n, 2], got shape {off.shape}")
    q = (off.reshape(-1, 2) + np.asarray(LIMITS[0], np.float64) - np.asarray(origin, np.float64)) / np.float64(SDF_CELL_SIZE)
    return q, _max_origin(shape)


def world_map_window_origins(name, offsets):
    """int32 [N, 2]: the origin cells of the robots' windows.  Robot r's window covers global offsets[r] + LIMITS, so its origin is
    (offset + LIMITS[0] - origin) / SDF_CELL_SIZE per axis, in float64.  It must lie within 1e-3 of an integer (float32 offsets that are
    multiples of the cell pitch are not exact; half a cell off is an error) and inside [0, W - 400]; otherwise ValueError names the
    first robot at fault and whether it is off the cell grid or outside the world.  snap_to_world_map gives offsets that pass."""
    q, limit = _window_cells(name, offsets, "world_map_window_origins")
    r = np.rint(q)
    with np.errstate(invalid="ignore"):
        off_grid = ~(np.abs(q - r) <= 1e-3)
        outside = ~off_grid & ((r < 0) | (r > np.asarray(limit, np.float64)))
    bad = np.flatnonzero((off_grid | outside).any(1))
    if bad.size:
        k = int(bad[0])
        if off_grid[k].any():
            raise ValueError(f"world_map_window_origins: the window of robot {k} is off the cell grid of {name!r}: its origin is at cell "
                             f"{q[k].tolist()} (snap_to_world_map gives the nearest valid offsets)")
        raise ValueError(f"world_map_window_origins: the window of robot {k} is outside the world {name!r}: its origin cell "
                         f"{r[k].astype(np.int64).tolist()} is not in 0 .. {limit}")
    return r.astype(np.int32)


def world_map_window_offsets(name, origins):
    """float32 [n, 2]: the offsets of the windows at the origin cells `origins` (integers [n, 2], each a window inside the world), the
    inverse of world_map_window_origins: origin * SDF_CELL_SIZE + world origin - LIMITS[0] per axis in float64, then float32
    (snap_to_world_map's formula on whole cells).  world_map_window_origins accepts the result and returns the origins."""
    org = checked_window_origins(name, origins, "world_map_window_offsets")
    out = org.astype(np.float64) * np.float64(SDF_CELL_SIZE) + np.asarray(world_map_origin(name), np.float64) - np.asarray(LIMITS[0], np.float64)
    return out.astype(np.float32)


def snap_to_world_map(name, offsets):
    """float32 offsets of the shape given: per robot the nearest offsets whose window starts on a cell and lies inside the world."""
    q, limit = _window_cells(name, offsets, "snap_to_world_map")
    if not np.isfinite(q).all():
        raise ValueError("snap_to_world_map: every offset must be finite")
    cells = np.clip(np.rint(q), 0, np.asarray(limit, np.float64))
    out = cells * np.float64(SDF_CELL_SIZE) + np.asarray(world_map_origin(name), np.float64) - np.asarray(LIMITS[0], np.float64)
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
        i0, j0 = checked_window_origins(name, a.reshape(1, 2), "world_window_name")[0].tolist()
    else:
        i0, j0 = world_map_window_origins(name, a.reshape(1, 2))[0].tolist()
    return f"{name}{_WINDOW_SEPARATOR}{i0},{j0}"


def world_map_sdf(points_global, name, device=None):
    """The world texture's nearest-cell value at global points [..., 2] -> float32 [...], NaN at a point with a non-finite coordinate.
    device=None: on the host texture (world_map_texture: slow to build at full world size), a CPU tensor.  With a device: read off the
    resident world texture by mmd_sdf_grid_lookup, a tensor on that device -- the practical source of truth for "is this start free"."""
    shape = _world(name, "world_map_sdf")[0]
    lo, hi = world_map_limits(name)
    if device is None:
        val, finite = texel_values(world_map_texture(name), points_global, lo, hi)
        return torch.from_numpy(np.where(finite, val, np.float32(np.nan)))
    from . import _lib
    tex = _resident().device_world_texture(name, device)
    pts = torch.as_tensor(points_global, dtype=torch.float32).to(tex.device).contiguous()
    flat = pts.reshape(-1, 2)
    out = torch.empty(flat.shape[0], 4, dtype=torch.float32, device=tex.device)
    _lib.launch("mmd_sdf_grid_lookup", tex, _lib.require_gpu(tex, "world texture"), shape[0], shape[1], (C.c_float * 2)(*lo),
                (C.c_float * 2)(*hi), _lib.require_gpu(flat, "points"), flat.shape[0], _lib.require_gpu(out, "out"))
    return out[:, 0].reshape(pts.shape[:-1])


def device_world_sdf_grid(name, device, out=None):
    """The [WX, WY, 4] texture of the world map `name`, built on `device` by mmd_sdf_grid_from_occupancy: world_map_texture bit for
    bit, for the upload of one byte per cell.  out= rebuilds a resident texture in place on the current stream."""
    device, out = _out_texture("device_world_sdf_grid", _world(name, "device_world_sdf_grid")[0], device, out)
    return _occupancy_build(torch.from_numpy(world_map_occupancy(name)).to(device), out)
