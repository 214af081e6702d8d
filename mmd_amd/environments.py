"""2-D maps of the reference (geometry only) and their precomputed SDF grids (host side, init time).

Geometry: deps/torch_robotics/torch_robotics/environments/env_{empty,empty_nowait,highways,conveyor,drop_region}_2d.py.
SDF: MultiRoundedBoxField (primitives.py:312-333) composed with the empty MultiSphereField's constant 1
(primitives.py:109-110) through ObjectField's min (:567-570); grid = GridMapSDF.precompute_sdf
(grid_map_sdf.py:34-63): value and autograd gradient on linspace(lo,hi,ceil(dim/cell))^2.
The reference rebuilds this grid N+1 times per trial (once per planner); here it is built once per map and shared.

Custom maps (register_map): any set of spheres and rounded boxes on the same tile at the same cell size, what the reference's EnvBase
takes as ObjectField([MultiSphereField, MultiBoxField]).  The host texture (sdf_grid_texture, torch autograd) is the definition; the
resident device texture of a registered map is built by the library (mmd_sdf_grid_build, csrc/sdf_grid.hip), bit for bit the same.
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
    if name in _REGISTERED and _REGISTERED[name] != content:
        raise ValueError(f"register_map: {name!r} is registered with other primitives (update_map replaces them)")
    _REGISTERED[name] = content


def unregister_map(name):
    """Forget a registered map, its host texture and every resident device texture that holds it (objects built on it keep theirs)."""
    if name not in _REGISTERED:
        raise ValueError(f"unregister_map: {name!r} is not a registered map")
    del _REGISTERED[name]
    _drop_host_texture(name)
    from . import guides
    guides.drop_resident_textures(name)


def registered_maps():
    return tuple(sorted(_REGISTERED))


def map_primitives(name):
    """(boxes [(cx, cy, size_x, size_y)], spheres [(cx, cy, r)]) of a shipped or registered map."""
    base = _base_name(name)
    if base in _REGISTERED:
        return _REGISTERED[base]
    if base not in MAP_BOXES:
        raise KeyError(f"unknown map {name!r} (shipped: {sorted(MAP_BOXES)}; registered: {sorted(_REGISTERED)})")
    centers, sizes = MAP_BOXES[base]
    return tuple((float(c[0]), float(c[1]), float(s[0]), float(s[1])) for c, s in zip(centers, sizes)), ()


def is_registered(name):
    return _base_name(name) in _REGISTERED


def map_has_obstacles(name):
    """Whether the map's fixed objects have an SDF grid (mmd_guide_desc.n_grids = 1).  A registered map always has one, even without
    primitives: update_map may give it some while a guide that reads the grid is alive."""
    base = _base_name(name)
    return base in _REGISTERED or len(MAP_BOXES[base][0]) > 0


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
    content = _REGISTERED.get(base)                  # (None: a shipped map, whose content never changes)
    hit = _TEXTURE_CACHE.get((base, cell_size))
    if hit is not None and hit[0] == content:
        return hit[1]
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
    if name not in _REGISTERED:
        raise ValueError(f"update_map: {name!r} is not a registered map")
    _REGISTERED[name] = _checked_primitives(boxes, spheres)
    _drop_host_texture(name)
    from . import guides
    guides.rebuild_resident_textures(name)
