"""The SDF textures resident on the devices: one per (map set, device) and one per (world map, device) for every guide / task facade of
the process (the reference precomputes the grid once per planner object, grid_map_sdf.py:34-63, N+1 times per instance),
and what environments.update_* / unregister_* do to them: rebuild in place, or forget."""
import ctypes as C

import numpy as np
import torch

from . import _lib, environments

_TEXTURES = {}                      # (map names, device) -> the set's resident textures [n_maps, n_grids=1, nx, ny, 4]
_WORLD_TEXTURES = {}                # (world map, device) -> its resident texture [WX, WY, 4]
_WINDOW_CUTS = {}                   # key of _TEXTURES -> [(world map, first slice, origins int32 [n, 2] on the device)]: its window slices
_WINDOW_SETS = []                   # the live WorldWindowSets: window slices owned by their user, not keyed by names
N_TEXTURE_UPLOADS = 0               # host-built textures copied to a device: 1 per map set that holds a shipped map, however many
# Texture slices built on a device, by ONE rule: + 1 for every texture a library call writes whole.  A registered map's slice built or rebuilt
# (mmd_sdf_grid_build / mmd_sdf_grid_from_occupancy): 1.  A world texture built or rebuilt from its bitmap (mmd_sdf_grid_from_occupancy):
# 1.  A cut (mmd_sdf_grid_windows): 1 per window slice it writes, so n for a launch of n windows; a moved cut (mmd_sdf_grid_windows_moved): 1
# per slice whose origin changed, which the caller of WorldWindowSet.move knows on the host.
N_TEXTURE_BUILDS = 0


def device_world_texture(name, device):
    """[WX, WY, 4] float32: the texture of the world map `name` (environments.register_world_map), resident once per (name, device), built
    there by mmd_sdf_grid_from_occupancy: environments.world_map_texture bit for bit.  Counts 1 in N_TEXTURE_BUILDS when it is built."""
    global N_TEXTURE_BUILDS
    key = (name, str(environments.resolved_device(device)))
    if key not in _WORLD_TEXTURES:
        _WORLD_TEXTURES[key] = environments.device_world_sdf_grid(name, device)
        N_TEXTURE_BUILDS += 1
    return _WORLD_TEXTURES[key]


def _window_runs(maps):
    """[(world, first slice, [(i0, j0), ...])]: the window names among `maps`, as runs of neighbouring slices of one world.  The names of a
    world's windows share a prefix, so in a sorted map set they are one run per world (another map whose name sorts in between splits it)."""
    runs = []
    for i, m in enumerate(maps):
        kind, world, _, origin = environments.resolve_map(m)
        if kind != "window":
            continue
        if runs and runs[-1][0] == world and runs[-1][1] + len(runs[-1][2]) == i:
            runs[-1][2].append(origin)
        else:
            runs.append((world, i, [origin]))
    return runs


def _cut_windows(tex, cuts):
    """One mmd_sdf_grid_windows launch per (world, first slice, origins): the window slices straight into the set's storage `tex`, on the
    current stream of its device."""
    global N_TEXTURE_BUILDS
    for world, first, origins in cuts:
        wtex = device_world_texture(world, tex.device)
        n = origins.shape[0]
        _lib.launch("mmd_sdf_grid_windows", tex, _lib.require_gpu(wtex, "world texture"), wtex.shape[0], wtex.shape[1],
                    C.c_void_p(origins.data_ptr()), n, tex.shape[2], tex.shape[3], _lib.require_gpu(tex[first:first + n], "window slices"))
        N_TEXTURE_BUILDS += n


def device_sdf_textures(maps, device):
    """[n_maps, n_grids=1, nx, ny, 4] float32 on `device`, resident once per process.  The shipped maps' slices are the host textures,
    stacked and uploaded in one copy; a registered map's (environments.register_map / register_occupancy_map) is built on the device
    from its primitives or its bitmap; the slice of a window of a world map (environments.world_window_name) is cut on the device from
    the world's resident texture (device_world_texture), all windows of one world in one mmd_sdf_grid_windows launch.  The set is of
    unique names: windows at equal origins are one slice.  The counters count by the rules stated at their definitions."""
    global N_TEXTURE_UPLOADS, N_TEXTURE_BUILDS
    device = environments.resolved_device(device)
    key = (tuple(maps), str(device))
    if key not in _TEXTURES:
        kinds = [environments.resolve_map(m)[0] for m in maps]
        tex = torch.empty(len(maps), 1, *environments.grid_shape(), 4, dtype=torch.float32, device=device)
        shipped = [i for i, kind in enumerate(kinds) if kind == "shipped"]
        if shipped:
            host = np.stack([environments.sdf_grid_texture(maps[i]) for i in shipped])
            tex[shipped, 0] = torch.from_numpy(host).to(device)
            N_TEXTURE_UPLOADS += 1
        for i, kind in enumerate(kinds):
            if kind in ("primitives", "occupancy"):
                environments.build_resident_texture(maps[i], device, tex[i, 0])
                N_TEXTURE_BUILDS += 1
        cuts = [(world, first, torch.from_numpy(environments.checked_window_origins(world, np.asarray(origins), "device_sdf_textures"))
                 .to(device)) for world, first, origins in _window_runs(maps)]
        _cut_windows(tex, cuts)
        _TEXTURES[key] = tex
        if cuts:
            _WINDOW_CUTS[key] = cuts
    return _TEXTURES[key]


def release_sdf_textures(maps, device):
    """Forget the resident textures of exactly the map set `maps` on `device` (the names in device_sdf_textures' order) and its window
    cuts: the next device_sdf_textures of the set builds it again, and update_* no longer reaches it.  An object built on the set keeps
    its tensor.  For a caller that builds map sets it will not use again (world_fleet.WorldFleet: one set of windows per epoch, 2.56 MB a
    window).  -> whether the set was resident."""
    key = (tuple(maps), str(environments.resolved_device(device)))
    _WINDOW_CUTS.pop(key, None)
    return _TEXTURES.pop(key, None) is not None


class WorldWindowSet:
    """n window slices of the world map `world` on one device, owned by their user: slice r is robot r's, whatever the origins (equal
    origins do not share a slice), the set has no names, and its storage `tex` [n, n_grids=1, nx, ny, 4] and its pointers are stable
    for its lifetime.  It holds two origin buffers on the device, this move's and the last one's, so that no launch reads and writes
    one.  The set is registered: environments.update_world_map(world, ..) cuts every slice again in place at its CURRENT origin,
    unregister_world_map forgets the set (it keeps its tensors), release() takes it out of the registry."""

    def __init__(self, world, n, device):
        if not environments.is_world_map(world):
            raise ValueError(f"WorldWindowSet: {world!r} is not a registered world map")
        if int(n) < 1:
            raise ValueError(f"WorldWindowSet: n = {n} slices (at least 1)")
        self.world, self.n, self.device = world, int(n), environments.resolved_device(device)
        self.tex = torch.empty(self.n, 1, *environments.grid_shape(), 4, dtype=torch.float32, device=self.device)
        self._origins = [torch.empty(self.n, 2, dtype=torch.int32, device=self.device) for _ in range(2)]
        self._current = None            # which buffer holds the origins the slices were cut at; None before the first move
        _WINDOW_SETS.append(self)

    @property
    def origins(self):
        """int32 [n, 2] on the device: the origins the slices hold now (the set's own buffer; read only), None before the first move"""
        return None if self._current is None else self._origins[self._current]

    def _cut(self, origins, held):
        wtex = device_world_texture(self.world, self.device)
        _lib.launch("mmd_sdf_grid_windows_moved", self.tex, _lib.require_gpu(wtex, "world texture"), wtex.shape[0], wtex.shape[1],
                    C.c_void_p(origins.data_ptr()), C.c_void_p(held.data_ptr()) if held is not None else None, self.n, self.tex.shape[2],
                    self.tex.shape[3], _lib.require_gpu(self.tex, "window slices"))

    def move(self, origins_dev, n_moved):
        """Move the windows to origins_dev (int32 [n, 2], contiguous, on the set's device; each a window inside the world, which the
        caller has checked): one device copy of the origins into the set's other buffer and one mmd_sdf_grid_windows_moved launch
        against the buffer of the last move, on the current stream.  The first move cuts every slice.  n_moved: the slices whose
        origin differs from the last move's (n on the first), which the caller knows on the host; N_TEXTURE_BUILDS grows by it."""
        global N_TEXTURE_BUILDS
        if not (isinstance(origins_dev, torch.Tensor) and origins_dev.dtype == torch.int32 and tuple(origins_dev.shape) == (self.n, 2)
                and origins_dev.device == self.device and origins_dev.is_contiguous()):
            raise ValueError(f"WorldWindowSet.move: origins must be a contiguous int32 tensor [{self.n}, 2] on {self.device}")
        if not 0 <= int(n_moved) <= self.n or (self._current is None and int(n_moved) != self.n):
            raise ValueError(f"WorldWindowSet.move: n_moved = {n_moved} of {self.n} slices (all of them on the first move)")
        nxt = 0 if self._current is None else 1 - self._current
        self._origins[nxt].copy_(origins_dev)
        self._cut(self._origins[nxt], self.origins)
        self._current = nxt
        N_TEXTURE_BUILDS += int(n_moved)

    def recut(self):
        """update_world_map: every slice again from the world's texture at its current origin, in place.  Nothing before the first move."""
        global N_TEXTURE_BUILDS
        if self._current is not None:
            with torch.cuda.device(self.device):
                self._cut(self.origins, None)
            N_TEXTURE_BUILDS += self.n

    def release(self):
        """Take the set out of the registry: update_world_map no longer reaches it.  -> whether it was registered."""
        live = any(s is self for s in _WINDOW_SETS)
        _WINDOW_SETS[:] = [s for s in _WINDOW_SETS if s is not self]
        return live


def rebuild_resident_textures(name, device_occupancy=None):
    """environments.update_*: whatever resident texture holds the registered name is rebuilt in place -- same storage, same pointers -- on
    the current stream of its device.  A tile map: every slice of the name, by the builder of its kind; device_occupancy is the new
    bitmap as a device tensor, used as it is for the slices on its device.  A world map: every resident world texture from the registry's
    bitmap, then every window slice cut from it again, one launch per (map set, run of its windows), and every WorldWindowSet of the world at its current origins.  Counted 1 per slice and world texture."""
    global N_TEXTURE_BUILDS
    for (world, _), wtex in _WORLD_TEXTURES.items():
        if world == name:
            environments.device_world_sdf_grid(name, wtex.device, out=wtex)
            N_TEXTURE_BUILDS += 1
    for key, tex in _TEXTURES.items():
        for i, m in enumerate(key[0]):
            kind, base, _, _ = environments.resolve_map(m, unknown_ok=True)
            if base == name and kind != "window":                   # (a window of the world map `name`: cut again below)
                with torch.cuda.device(tex.device):
                    if device_occupancy is not None and device_occupancy.device == tex.device:
                        environments.device_occupancy_sdf_grid(device_occupancy, tex.device, out=tex[i, 0])
                    else:
                        environments.build_resident_texture(m, tex.device, tex[i, 0])
                N_TEXTURE_BUILDS += 1
        if key in _WINDOW_CUTS:
            _cut_windows(tex, [c for c in _WINDOW_CUTS[key] if c[0] == name])
    for ws in _WINDOW_SETS:
        if ws.world == name:
            ws.recut()


def drop_resident_textures(name):
    """environments.unregister_*, called while the name still resolves: forget the resident textures of the world map `name` and every map
    set that holds the tile map `name` or a window of the world map `name`, and every WorldWindowSet of the world map `name` (an object
    built on one keeps its tensor)."""
    for key in [k for k in _WORLD_TEXTURES if k[0] == name]:
        del _WORLD_TEXTURES[key]
    for key in [k for k in _TEXTURES if any(environments.resolve_map(m, unknown_ok=True)[1] == name for m in k[0])]:
        del _TEXTURES[key]
        _WINDOW_CUTS.pop(key, None)
    _WINDOW_SETS[:] = [ws for ws in _WINDOW_SETS if ws.world != name]
