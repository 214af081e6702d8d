"""constraints.framed_slot_bound computed with broadcast comparisons, a chunk of rows at a time, is the loop over robots it replaced: the
loop is written out here, with the same comparisons, the same eps and the same integers, and the two must agree on offsets on the cell
grid, on sharded ranges, with chunks smaller than the range, and on offsets placed exactly on, one float32 ulp inside and one float32 ulp
outside the boundary of the intersection.  Then the surface of the persistent fleet as far as it shows without a GPU: the two new entry
points are built, declared and answer their argument errors before any launch; a window set registers, releases and is forgotten with its
world; `move` on a sampler of the shared named windows is refused."""
import numpy as np
import pytest
import torch

from mmd_amd import constraints
from mmd_amd.constraints import VERTEX_CONSTRAINT_RADIUS, framed_slot_bound, framed_window
from mmd_amd.environments import LIMITS, SDF_CELL_SIZE


def loop_slot_bound(offsets, robot0, n_local, limits=LIMITS, radius=VERTEX_CONSTRAINT_RADIUS):
    """framed_slot_bound as a loop over the local robots: per robot the other robots whose window box meets its widened window"""
    off = np.asarray(offsets, dtype=np.float64).reshape(-1, 2)
    n = off.shape[0]
    wlo, whi = (np.asarray(v, dtype=np.float64) for v in framed_window(limits, radius))
    lo, hi = np.asarray(limits[0], dtype=np.float64), np.asarray(limits[1], dtype=np.float64)
    eps = 4.0 * float(np.finfo(np.float32).eps) * (np.abs(off).max() + max(np.abs(wlo).max(), np.abs(whi).max()))
    worst = 0
    for r in range(robot0, robot0 + n_local):
        hit = np.all((off + hi >= off[r] + wlo - eps) & (off + lo <= off[r] + whi + eps), axis=1)
        worst = max(worst, int(hit.sum()) - 1)
    return min(max(worst, 1), n - 1)


def grid_offsets(n, extent_cells, seed):
    """float32 offsets on the cell grid, as a fleet's windows have them: whole cells times the cell size, in float64, then float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, extent_cells, (n, 2)).astype(np.float64) * SDF_CELL_SIZE - extent_cells * SDF_CELL_SIZE / 2).astype(np.float32)


def shards(n):
    """(robot0, n_local): the whole range, its halves where they are whole, single robots at both ends and an inner range"""
    out = [(0, n), (0, 1), (n - 1, 1), (n // 3, n - n // 3 - n // 4)]
    if n % 2 == 0:
        out += [(0, n // 2), (n // 2, n // 2)]
    return [s for s in out if s[1] >= 1]


@pytest.mark.parametrize("n", [2, 3, 65, 300])
@pytest.mark.parametrize("extent_cells", [500, 2048])           # dense (most windows meet) and sparse
def test_slot_bound_is_the_loop_on_the_cell_grid(n, extent_cells):
    off = grid_offsets(n, extent_cells, 11 * n + extent_cells)
    for robot0, n_local in shards(n):
        assert framed_slot_bound(off, robot0, n_local) == loop_slot_bound(off, robot0, n_local), (n, robot0, n_local)


@pytest.mark.parametrize("n", [3, 65, 300])
def test_slot_bound_is_the_loop_in_small_chunks(n, monkeypatch):
    """the chunking itself: chunks of 1 row, of a few rows that do not divide the range, and of exactly the range"""
    off = grid_offsets(n, 700, n)
    for pairs in (1, 7 * n, n * n):
        monkeypatch.setattr(constraints, "SLOT_BOUND_CHUNK_PAIRS", pairs)
        for robot0, n_local in shards(n):
            assert framed_slot_bound(off, robot0, n_local) == loop_slot_bound(off, robot0, n_local), (n, pairs, robot0, n_local)


def ulps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


@pytest.mark.parametrize("n", [2, 3, 65, 300])
@pytest.mark.parametrize("base", [0.0, 3.0, -40.0])
def test_slot_bound_is_the_loop_at_the_boundary(n, base):
    """Robot 0 at `base`; the others at the separation at which their box just touches robot 0's widened window -- (hi - wlo) along x,
    the float32 nearest to it, and that float32 one and two ulp to either side -- on both sides and along both axes, the rest far away.
    The count with the eps is whatever the comparisons give: the vectorised form must give the loop's, robot for robot."""
    wlo, whi = framed_window(LIMITS, VERTEX_CONSTRAINT_RADIUS)
    touch = [np.float32(np.float64(LIMITS[1][0]) - np.float64(wlo[0])), np.float32(np.float64(whi[0]) - np.float64(LIMITS[0][0]))]
    near = [ulps(t, k) for t in touch for k in (-2, -1, 0, 1, 2)]
    rows = [(np.float32(base), np.float32(base))]
    for k in range(1, n):
        d, axis, sign = near[k % len(near)], (k // len(near)) % 2, 1 if (k // (2 * len(near))) % 2 == 0 else -1
        if k > 4 * len(near):
            rows.append((np.float32(base + 100.0 + k), np.float32(base - 100.0 - k)))
            continue
        p = [np.float32(base), np.float32(base)]
        p[axis] = np.float32(np.float32(base) + np.float32(sign) * d)
        rows.append(tuple(p))
    off = np.asarray(rows, np.float32)
    for robot0, n_local in shards(n):
        assert framed_slot_bound(off, robot0, n_local) == loop_slot_bound(off, robot0, n_local), (n, base, robot0, n_local)
    # and per robot, so that no maximum hides a difference
    for r in range(min(n, 24)):
        assert framed_slot_bound(off, r, 1) == loop_slot_bound(off, r, 1), (n, base, r)


# ---- the surface of the persistent fleet, as far as it shows without a GPU -----------------------------------------------------------------
def test_new_entry_points_are_built_declared_and_answer_before_any_launch():
    import ctypes as C
    import os
    import __graft_entry__ as G
    from mmd_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "mmd_amd/csrc/fleet_epoch.hip" in G.SOURCES and "mmd_amd/csrc/fleet_epoch.hip" in open(os.path.join(root, "build.sh")).read()
    header = open(os.path.join(root, "include", "mmd_amd.h")).read()
    assert "int mmd_sdf_grid_windows_moved(" in header and "int mmd_fleet_epoch_frames(" in header and _lib.ABI_VERSION == 9
    lib = _lib.load()
    p = C.c_void_p(256)                                         # never dereferenced: every call below returns before a launch
    for args, word in (((p, 37, 45, p, None, -1, 5, 7, p), "n_windows"), ((p, 0, 45, p, None, 1, 5, 7, p), "world"),
                       ((p, 37, 45, p, p, 1, 38, 7, p), "windows"), ((None, 37, 45, p, p, 1, 5, 7, p), "NULL world"),
                       ((p, 37, 45, None, p, 1, 5, 7, p), "NULL origins"), ((p, 37, 45, p, None, 1, 5, 7, None), "NULL windows"),
                       ((p, 46341, 46341, p, None, 1, 1, 1, p), "32-bit")):
        rc = lib.mmd_sdf_grid_windows_moved(*args, None)
        assert rc != 0 and word in lib.mmd_last_error().decode() and "mmd_sdf_grid_windows_moved" in lib.mmd_last_error().decode(), args
    assert lib.mmd_sdf_grid_windows_moved(None, 37, 45, None, None, 0, 5, 7, None, None) == 0
    d5, f4 = (C.c_double * 5)(), (C.c_float * 4)()
    good = [p, p, p, p, 2, p, 3, d5, f4, f4, f4, p, p, p, p, p, p]
    for at, value, word in ((6, -1, "n_robots"), (4, 3, "points_stride"), (4, 0, "points_stride"), (7, None, "offset_terms"),
                            (0, None, "cells"), (2, C.c_void_p(264), "summary"), (3, C.c_void_p(260), "points"), (11, None, "line"),
                            (12, C.c_void_p(260), "offsets"), (14, C.c_void_p(264), "hard"), (16, None, "lines")):
        args = list(good)
        args[at] = value
        rc = lib.mmd_fleet_epoch_frames(*args, None)
        assert rc != 0 and word in lib.mmd_last_error().decode() and "mmd_fleet_epoch_frames" in lib.mmd_last_error().decode(), (at, word)
    args = list(good)
    args[6] = 0
    assert lib.mmd_fleet_epoch_frames(*args, None) == 0         # no robots: nothing launched


def test_window_set_registry_and_sampler_refusals():
    import inspect
    import types
    from mmd_amd import environments as E, map_textures, world_fleet as F
    from mmd_amd.world import WorldRobotSampler
    assert inspect.signature(F.WorldFleet.__init__).parameters["persistent"].default is False
    assert inspect.signature(WorldRobotSampler.__init__).parameters["own_windows"].default is False
    assert list(inspect.signature(WorldRobotSampler.move).parameters) == ["self", "starts", "goals", "offsets"]
    name = "PersistHostWorld"
    E.register_world_map(name, np.zeros((400, 400), np.uint8))
    try:
        before = len(map_textures._WINDOW_SETS)
        a, b = map_textures.WorldWindowSet(name, 3, "cpu"), map_textures.WorldWindowSet(name, 1, "cpu")
        assert a.tex.shape == (3, 1, 400, 400, 4) and a.origins is None and len(map_textures._WINDOW_SETS) == before + 2
        E.update_world_map(name, np.ones((400, 400), np.uint8))           # a set that was never moved has nothing to cut
        assert a.release() is True and a.release() is False and len(map_textures._WINDOW_SETS) == before + 1
        with pytest.raises(ValueError, match="n_moved"):
            b.move(torch.zeros(1, 2, dtype=torch.int32), 0)                 # the first move cuts every slice
        with pytest.raises(ValueError, match="origins"):
            b.move(torch.zeros(2, 2, dtype=torch.int32), 1)
        with pytest.raises(ValueError, match="not a registered world map"):
            map_textures.WorldWindowSet("EnvEmpty2D", 2, "cpu")
        named = types.SimpleNamespace(_window_ids=[name + "@0,0"], env_id=name)
        with pytest.raises(ValueError, match="own_windows=True"):
            WorldRobotSampler.move(named, np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32))
    finally:
        E.unregister_world_map(name)                                        # forgets the set that is left
    assert len(map_textures._WINDOW_SETS) == before
