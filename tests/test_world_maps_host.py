"""CPU: world maps (environments.register_world_map) -- the registry and its name rules, the window origins of float32 offsets, the host
definition (a window is the crop of the world's transform, not the transform of the cropped bitmap), the one-tile world, random
instances, and the surface and the argument checks of mmd_sdf_grid_windows / mmd_sdf_grid_lookup, which answer before any launch."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import world_map_model as M
from mmd_amd import _lib, environments as E

WORLD = "TestWorld"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world():
    """(bitmap, host texture) of the 640 x 520 test world, registered for the module: the texture is computed once and read-only."""
    occ = M.world_bitmap()
    E.register_world_map(WORLD, occ)
    tex = E.world_map_texture(WORLD)
    occ.setflags(write=False)
    tex.setflags(write=False)
    yield occ, tex
    E.unregister_world_map(WORLD)


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    tiles, worlds = set(E.registered_maps()), set(E.registered_world_maps())
    yield
    for name in set(E.registered_world_maps()) - worlds:
        E.unregister_world_map(name)
    for name in set(E.registered_maps()) - tiles:
        E.unregister_map(name)


def test_registry_and_name_clashes(registry):
    tile = np.zeros((400, 400), np.uint8)
    occ = np.zeros((400, 500), np.uint8)
    occ[10, 20] = 1
    before = E.registered_maps()
    for name in ("EnvEmpty2D", "EnvHighways2D", "BigExtraObjects", "", None):
        with pytest.raises(ValueError):
            E.register_world_map(name, occ)
    E.register_world_map("Big", occ)
    assert E.registered_world_maps() == ("Big",) and E.is_world_map("Big") and not E.is_world_map("EnvEmpty2D")
    assert E.registered_maps() == before and not E.is_registered("Big")                      # a registry of its own
    E.register_world_map("Big", occ.astype(np.float64) * 2.5)                                # the same cells: a no-op
    E.register_world_map("Big", occ, origin=(-1.0, -1.25))                                   # the default origin, spelled out
    other = occ.copy()
    other[0, 0] = 1
    with pytest.raises(ValueError, match="update_world_map"):
        E.register_world_map("Big", other)
    with pytest.raises(ValueError, match="update_world_map"):
        E.register_world_map("Big", occ, origin=(0.0, 0.0))
    # the names are shared, in both directions
    for register in (lambda n: E.register_map(n, [(0, 0, 0.1, 0.1)]), lambda n: E.register_occupancy_map(n, tile)):
        with pytest.raises(ValueError, match="world map"):
            register("Big")
        with pytest.raises(ValueError, match="world map"):
            register(E.world_window_name("Big", (0, 37)))
    E.register_map("Prims", [(0, 0, 0.1, 0.1)])
    E.register_occupancy_map("Floor", tile)
    for name in ("Prims", "Floor"):
        with pytest.raises(ValueError, match="tile map"):
            E.register_world_map(name, occ)
    # what register_map accepts today stays accepted: a name with the separator in it, next to a world map it is no window of
    E.register_map("Other@3,4", [(0, 0, 0.1, 0.1)])
    assert "Other@3,4" in E.registered_maps() and not E.is_world_window("Other@3,4")
    with pytest.raises(ValueError, match="window name"):
        E.register_world_map("Other", occ)
    # update: same shape only; unregister
    E.update_world_map("Big", other)
    assert np.array_equal(E.world_map_occupancy("Big"), other) and E.world_map_occupancy("Big").dtype == np.uint8
    with pytest.raises(ValueError):
        E.update_world_map("Big", np.zeros((400, 501)))
    for name in ("Prims", "EnvEmpty2D", "Never"):
        with pytest.raises(ValueError, match="not a registered world map"):
            E.update_world_map(name, occ)
    with pytest.raises(ValueError):
        E.unregister_map("Big")
    assert E.world_map_limits("Big") == ((-1.0, -1.25), (1.0, 1.25))
    E.unregister_world_map("Big")
    assert E.registered_world_maps() == () and not E.is_world_window("Big@0,37")
    with pytest.raises(ValueError):
        E.unregister_world_map("Big")
    E.register_map("Big@0,37", [(0, 0, 0.1, 0.1)])                                           # free again, as before the world map
    assert E.registered_maps() == tuple(sorted(before + ("Big@0,37", "Floor", "Other@3,4", "Prims")))


def test_resolve_map_agrees_with_the_predicates(registry):
    """environments.resolve_map is the one reading of a map name: over a fixed list of names, the kind it returns (None: KeyError) is what
    every public predicate answers, and base name, record and origin are the registry's."""
    E.register_map("Prims", [(0, 0, 0.1, 0.1)])
    E.register_occupancy_map("Floor", np.zeros((400, 400), np.uint8))
    E.register_world_map("World", np.zeros((400, 500), np.uint8))
    window = E.world_window_name("World", (0, 37))
    assert window == "World@0,37"
    names = (("EnvHighways2D", "shipped"), ("EnvHighways2DExtraObjects", "shipped"), ("Prims", "primitives"), ("Floor", "occupancy"),
             ("World", None), (window, "window"), ("World@1,", None), ("World@-1,2", None), ("Other@3,4", None), (7, None))
    for name, kind in names:
        try:
            got = E.resolve_map(name)
        except KeyError:
            got = (None,) * 4
        assert got[0] == kind, name
        assert E.is_registered(name) == (kind in ("primitives", "occupancy")), name
        assert E.is_occupancy_map(name) == (kind == "occupancy"), name
        assert E.is_world_window(name) == (kind == "window"), name
        assert E.is_world_map(name) == (name == "World"), name
    assert E.resolve_map("EnvHighways2DExtraObjects") == ("shipped", "EnvHighways2D", None, None)
    kind, base, rec, origin = E.resolve_map("PrimsExtraObjects")
    assert (kind, base, origin) == ("primitives", "Prims", None) and rec.kind == "primitives" and rec.content == E.map_primitives("Prims")
    kind, base, rec, origin = E.resolve_map(window + "ExtraObjects")
    assert (kind, base, origin) == ("window", "World", (0, 37)) and rec.kind == "world" and E.world_window(window) == ("World", (0, 37))
    with pytest.raises(KeyError, match="Other@3,4"):
        E.sdf_grid_texture("Other@3,4")


def test_guides_reads_the_residency_counters_live():
    """guides still answers to the counters' and caches' names: the values of map_textures at the time of the read, never a copy."""
    from mmd_amd import guides, map_textures
    assert guides._TEXTURES is map_textures._TEXTURES and guides._WORLD_TEXTURES is map_textures._WORLD_TEXTURES
    assert guides.device_world_texture is map_textures.device_world_texture
    before = map_textures.N_TEXTURE_BUILDS
    map_textures.N_TEXTURE_BUILDS = before + 3
    try:
        assert guides.N_TEXTURE_BUILDS == before + 3 and guides.N_TEXTURE_UPLOADS == map_textures.N_TEXTURE_UPLOADS
    finally:
        map_textures.N_TEXTURE_BUILDS = before
    with pytest.raises(AttributeError):
        guides.N_TEXTURE_NOTHING


def _texel_model(p, lo, hi, n):
    """One axis of the texel of a point in plain Python: the fp32 sequence (p - lo) / |hi - lo| * n, one rounding per operation, then
    min(max(floor, 0), n - 1) on Python integers.  No float outside the integer range is converted: an infinite product is past the
    border it points to."""
    f = np.float32
    with np.errstate(over="ignore"):
        t = (f(p) - f(lo)) / abs(f(hi) - f(lo)) * f(n)
    if np.isinf(t):
        return n - 1 if t > 0 else 0
    return min(max(math.floor(float(t)), 0), n - 1)


def test_one_texel_lookup_on_the_host(registry):
    """The host has ONE texel lookup (environments.texel_values on _texel_indices).  400 x 400 over LIMITS: every cell edge on both axes,
    10 000 random points in +-1.2, the limits themselves and points far outside, +-1e30 and +-3e38 (whose scaled coordinate is past
    int64, or infinite) -- exactly the indices of the plain-Python model; map_sdf of an occupancy map and trials._grid_sdf return the
    texture's value at those indices."""
    import torch
    from mmd_amd import trials
    f = np.float32
    edges = np.arange(-210, 211) * 0.005
    special = [1.0, -1.0, np.nextafter(f(1), f(0)), -np.nextafter(f(1), f(0)), 1e30, -1e30, 3e38, -3e38]
    pts = np.concatenate([np.stack([edges, edges[::-1]], 1), np.stack([special, special[::-1]], 1),
                          np.random.Generator(np.random.PCG64(11)).uniform(-1.2, 1.2, (10000, 2))]).astype(f)
    assert np.isfinite(pts).all()
    want = np.array([[_texel_model(p[k], E.LIMITS[0][k], E.LIMITS[1][k], 400) for k in range(2)] for p in pts.tolist()])
    assert want.min() == 0 and want.max() == 399 and len(np.unique(want[:, 0])) == 400
    ix, iy, finite = E._texel_indices(pts, E.LIMITS[0], E.LIMITS[1], (400, 400))
    assert finite.all() and np.array_equal(ix, want[:, 0]) and np.array_equal(iy, want[:, 1])
    # a texture that names its texel, in the place of the map's own (the transform of a bitmap takes longer than this whole test)
    E.register_occupancy_map("Lookup", np.zeros((400, 400), np.uint8))
    tex = np.zeros((400, 400, 4), f)
    tex[..., 0] = np.arange(160000, dtype=f).reshape(400, 400)
    E._HOST_TEXTURES[("Lookup", E.SDF_CELL_SIZE)] = (E.resolve_map("Lookup")[2].content, tex)
    assert E.sdf_grid_texture("Lookup") is tex
    value = (want[:, 0] * 400 + want[:, 1]).astype(f)
    got = E.map_sdf(pts, "Lookup")
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), value)
    assert np.array_equal(trials._grid_sdf("Lookup", pts), value)
    values, finite = E.texel_values(tex, pts[:10400].reshape(100, 104, 2))                   # any leading shape
    assert values.shape == finite.shape == (100, 104) and finite.all() and np.array_equal(values.reshape(-1), value[:10400])


def test_shape_limits(registry):
    for shape in ((399, 400), (400, 399), (2049, 400), (400, 2049), (400,), (400, 400, 1)):
        with pytest.raises(ValueError):
            E.register_world_map("Edge", np.zeros(shape, np.uint8))
        assert not E.is_world_map("Edge")
    E.register_world_map("Edge", np.zeros((400, 2048), np.uint8))
    assert E.world_map_limits("Edge") == ((-1.0, -5.12), (1.0, 5.12))
    E.register_world_map("Edge2", np.zeros((2048, 400), bool), origin=(3.0, -7.5))
    lo, hi = E.world_map_limits("Edge2")
    assert lo == (3.0, -7.5) and hi == (3.0 + 2048 * 0.005, -7.5 + 400 * 0.005)
    with pytest.raises(ValueError):
        E.register_world_map("Edge3", np.zeros((400, 400)), origin=(0.0, float("nan")))


def test_origins_of_float32_offsets(registry):
    """Every valid origin of a 2048-cell world from its float32 offset k * 0.005, computed as a product and as a rounded float64: exact."""
    E.register_world_map("Wide", np.zeros((2048, 2048), np.uint8))
    k = np.arange(-824, 825)
    for off_x in ((k.astype(np.float32) * np.float32(0.005)), (k * 0.005).astype(np.float32)):
        offsets = np.stack([off_x, off_x[::-1]], 1)
        got = E.world_map_window_origins("Wide", offsets)
        assert got.dtype == np.int32 and got.shape == (len(k), 2)
        assert np.array_equal(got[:, 0], k + 824) and np.array_equal(got[:, 1], (k + 824)[::-1])
    import torch
    assert E.world_map_window_origins("Wide", torch.zeros(3, 2)).tolist() == [[824, 824]] * 3
    ok = np.zeros((4, 2), np.float32)
    for bad, word in ((np.float32([0.0025, 0]), "off the cell grid"), (np.float32([0, -0.0025]), "off the cell grid"),
                      (np.float32([-4.125, 0]), "outside the world"), (np.float32([4.125, 0]), "outside the world"),
                      (np.float32([0, -4.125]), "outside the world"), (np.float32([0, 4.125]), "outside the world"),
                      (np.float32([np.nan, 0]), "off the cell grid")):
        offsets = ok.copy()
        offsets[2] = bad
        with pytest.raises(ValueError, match=word) as e:
            E.world_map_window_origins("Wide", offsets)
        assert "robot 2" in str(e.value)
    assert E.world_map_window_origins("Wide", np.float32([[-4.12, 4.12]])).tolist() == [[0, 1648]]       # the last cell inside
    # the first robot at fault is named, by its own fault
    with pytest.raises(ValueError, match="robot 1 is outside the world"):
        E.world_map_window_origins("Wide", np.float32([[0, 0], [9, 0], [0.0025, 0]]))
    rng = np.random.Generator(np.random.PCG64(5))
    raw = rng.uniform(-6, 6, (64, 2)).astype(np.float32)
    snapped = E.snap_to_world_map("Wide", raw)
    assert snapped.dtype == np.float32 and snapped.shape == raw.shape
    org = E.world_map_window_origins("Wide", snapped)
    inside = (np.abs(raw) <= 4.12).all(1)
    assert inside.any() and not inside.all()
    assert (np.abs(snapped[inside] - raw[inside]) <= 0.0025 + 1e-6).all()                      # the nearest cell
    assert org.min() == 0 and org.max() == 1648
    assert E.snap_to_world_map("Wide", [0.0024, -9.0]).tolist() == [0.0, np.float32(-4.12)]


def test_windows_are_the_crop_of_the_worlds_transform(world):
    occ, tex = world
    assert tex.shape == M.SHAPE + (4,) and np.array_equal(bits(tex), bits(E.occupancy_sdf_texture(occ)))
    assert E.world_map_texture(WORLD) is tex                                                 # cached by content
    origins = [M.WINDOW_A, M.WINDOW_B, (240, 120), (0, 0), M.WINDOW_A]
    win = E.world_map_windows(WORLD, origins)
    assert win.dtype == np.float32 and win.shape == (5, 400, 400, 4)
    for k, (i0, j0) in enumerate(origins):
        assert np.array_equal(bits(win[k]), bits(tex[i0:i0 + 400, j0:j0 + 400])), k
    for bad in ([(241, 0)], [(0, 121)], [(-1, 0)], [(0, 0), (0, -1)], [(0.0, 0.0)]):
        with pytest.raises(ValueError):
            E.world_map_windows(WORLD, bad)
    # window A's lower border lies 5 cells above the bar, which is outside it: the crop knows the bar, the cropped bitmap's transform does not
    i0, j0 = M.WINDOW_A
    assert occ[M.BAR].all() and M.BAR[1].stop - 1 == j0 - 5 and not occ[M.BAR[0], M.BAR[1].stop:j0 + 60].any()
    own = E.occupancy_sdf_texture(occ[i0:i0 + 400, j0:j0 + 400])
    f = np.float32
    assert win[0][120, 0].tolist() == [f(0.005) * f(5) - f(0.0025), 0, 1, 0]                   # 5 cells above the bar's last row
    assert own[120, 0, 0] > 0.3 and np.abs(win[0][100:140, :20, 0] - own[100:140, :20, 0]).min() > 0.1
    # the two windows agree where they overlap
    assert np.array_equal(bits(win[0][240:]), bits(win[1][:160]))
    # names
    name = E.world_window_name(WORLD, M.WINDOW_A)
    assert name == E.world_window_name(WORLD, np.int32(M.WINDOW_A)) and E.is_world_window(name) and E.is_world_window(name + "ExtraObjects")
    lo = E.world_map_limits(WORLD)[0]
    offset = np.float32([lo[0] + 1.0 + 0.005 * i0, lo[1] + 1.0 + 0.005 * j0])
    assert E.world_window_name(WORLD, offset) == name and E.world_window(name) == (WORLD, M.WINDOW_A)
    assert np.array_equal(bits(E.sdf_grid_texture(name)), bits(win[0]))
    assert np.array_equal(bits(E.sdf_grid_texture(name + "ExtraObjects")), bits(win[0]))
    assert E.map_has_obstacles(name) and not E.is_registered(name)
    with pytest.raises(ValueError, match="window"):
        E.map_primitives(name)
    for bad in ((241, 0), (0, -1)):
        with pytest.raises(ValueError, match="outside"):
            E.world_window_name(WORLD, bad)
    import torch
    pts = np.random.Generator(np.random.PCG64(8)).uniform(-1, 1, (512, 2)).astype(np.float32)
    assert np.array_equal(bits(E.map_sdf(torch.from_numpy(pts), name).numpy()), bits(M.lookup(win[0], (-1, -1), (1, 1), pts)[:, 0]))


def test_world_map_sdf_on_the_host(world):
    occ, tex = world
    lo, hi = E.world_map_limits(WORLD)
    assert lo == (-1.6, -1.3) and hi == (-1.6 + 640 * 0.005, -1.3 + 520 * 0.005)
    rng = np.random.Generator(np.random.PCG64(9))
    pts = rng.uniform(-1.7, 1.7, (2048, 2)).astype(np.float32)
    pts[5] = [np.nan, 0]
    pts[6] = [0, np.inf]
    got = E.world_map_sdf(pts, WORLD).numpy()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(M.lookup(tex, lo, hi, pts)[:, 0]))
    assert np.isnan(got[5]) and np.isnan(got[6]) and np.isfinite(np.delete(got, [5, 6])).all()
    assert E.world_map_sdf(pts.reshape(32, 64, 2), WORLD).shape == (32, 64)
    centres = (np.argwhere(occ != 0)[::53] + 0.5) * 0.005 + np.asarray(lo)
    assert (E.world_map_sdf(centres, WORLD).numpy() < 0).all()


def test_one_tile_world_is_the_occupancy_map(registry):
    import occupancy_model
    occ = occupancy_model.test_occupancy()
    E.register_occupancy_map("Floor", occ)
    E.register_world_map("OneTile", occ, origin=(-1.0, -1.0))
    assert E.world_map_window_origins("OneTile", np.zeros((3, 2), np.float32)).tolist() == [[0, 0]] * 3
    name = E.world_window_name("OneTile", np.float32([0, 0]))
    assert np.array_equal(bits(E.sdf_grid_texture(name)), bits(E.sdf_grid_texture("Floor")))
    assert np.array_equal(bits(E.world_map_windows("OneTile", [(0, 0)])[0]), bits(E.sdf_grid_texture("Floor")))
    for off in ((0.005, 0), (0, -0.005)):
        with pytest.raises(ValueError, match="outside the world"):
            E.world_map_window_origins("OneTile", np.float32([off]))
    E.register_world_map("Empty", np.zeros((400, 400)), origin=(-1.0, -1.0))
    assert not E.map_has_obstacles(E.world_window_name("Empty", (0, 0)))
    E.update_world_map("Empty", occ)
    assert E.map_has_obstacles(E.world_window_name("Empty", (0, 0)))
    assert np.array_equal(bits(E.world_map_texture("Empty")), bits(E.sdf_grid_texture("Floor")))


def test_random_world_map_instance(world, registry):
    from mmd_amd.world import OBSTACLE_MARGIN, random_world_instance, random_world_map_instance
    occ, tex = world
    starts, goals, offsets = random_world_map_instance(WORLD, 24, seed=1)
    again = random_world_map_instance(WORLD, 24, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip((starts, goals, offsets), again))
    assert not np.array_equal(random_world_map_instance(WORLD, 24, seed=2)[2], offsets)
    assert all(a.dtype == np.float32 and a.shape == (24, 2) for a in (starts, goals, offsets))
    origins = E.world_map_window_origins(WORLD, offsets)
    assert len({tuple(o) for o in origins.tolist()}) > 12 and origins.min() >= 0 and (origins <= [240, 120]).all()
    lo, hi = E.world_map_limits(WORLD)
    assert OBSTACLE_MARGIN == 0.16
    for p in (starts, goals):
        assert (M.lookup(tex, lo, hi, p)[:, 0] > 0.16).all()
        assert (np.abs(p - offsets) <= 0.95 + 1e-6).all()
    for p in (starts, goals):
        d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)) + np.eye(24)
        assert d.min() > 0.15
    E.register_world_map("Solid", np.ones((400, 400), np.uint8))
    with pytest.raises(RuntimeError, match="not placed"):
        random_world_map_instance("Solid", 2, seed=0, max_draws=40)
    with pytest.raises(ValueError):
        random_world_map_instance("EnvHighways2D", 2, seed=0)
    # random_world_instance keeps its draws
    s, g, o = random_world_instance(6, 6.0, seed=1)
    assert o.shape == (6, 2) and np.abs(o).max() <= 2.0


def test_sampler_hook_and_refusals_before_any_device_work(world):
    import inspect
    import types
    from mmd_amd.multi_robot import MultiRobotSampler
    from mmd_amd.world import WorldRobotSampler
    assert MultiRobotSampler._robot_env_ids(types.SimpleNamespace(), 0, 4) is None
    assert list(inspect.signature(MultiRobotSampler._robot_env_ids).parameters) == ["self", "robot0", "n"]
    src = inspect.getsource(MultiRobotSampler)
    assert src.count("robot_env_ids=self._robot_env_ids(") == 2                               # __init__ and _subset_guide
    offsets = E.snap_to_world_map(WORLD, np.float32([[-0.6, 0.0], [0.6, 0.0], [-0.6, 0.0]]))
    ids = [E.world_window_name(WORLD, o) for o in offsets]
    fake = types.SimpleNamespace(_window_ids=ids)
    assert WorldRobotSampler._robot_env_ids(fake, 1, 2) == ids[1:] and ids[0] == ids[2] != ids[1]
    assert WorldRobotSampler._robot_env_ids(types.SimpleNamespace(_window_ids=None), 0, 3) is None
    starts = offsets + np.float32([0.2, 0.2])
    goals = offsets - np.float32([0.5, 0.1])
    for bad, word in ((np.float32([0.0025, 0]), "off the cell grid"), (np.float32([5, 0]), "outside the world")):
        off = offsets.copy()
        off[1] += bad
        with pytest.raises(ValueError, match=word):             # (a stand-in object: the refusal comes before any device work)
            WorldRobotSampler.__init__(types.SimpleNamespace(), None, starts + (off - offsets), goals + (off - offsets), off, env_id=WORLD,
                                       device="cpu")


def test_abi_symbols_and_argument_checks():
    """Both entry points are declared, exported and additive (ABI 9); the argument checks answer non-zero with a message before any device
    call: there is no GPU here, a check behind a launch could not answer like this."""
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmd_amd.h")).read()
    assert "int mmd_sdf_grid_windows(" in header and "int mmd_sdf_grid_lookup(" in header
    for name in ("mmd_sdf_grid_windows", "mmd_sdf_grid_lookup"):
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == 9 and hasattr(lib, name)
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9
    assert C.sizeof(_lib.ConsBins) == 56 and C.sizeof(_lib.Conflict) == 48 and C.sizeof(_lib.UnetOptions) == 20
    p = C.c_void_p(4096)              # never read: every call below is refused, or has nothing to do
    ok = (p, 37, 45, p, 3, 5, 7, p)
    for k, value, word in ((0, None, "NULL world"), (3, None, "NULL origins"), (7, None, "NULL windows"), (4, -1, "n_windows"),
                           (4, 65536, "n_windows"), (1, 0, "world of"), (2, -4, "world of"), (5, 0, "windows of"), (6, 0, "windows of"),
                           (5, 38, "windows of"), (6, 46, "windows of"), (5, -1, "windows of")):
        args = list(ok)
        args[k] = value
        rc = lib.mmd_sdf_grid_windows(*args, None)
        assert rc != 0 and word in lib.mmd_last_error().decode() and "mmd_sdf_grid_windows" in lib.mmd_last_error().decode(), (args, rc)
    assert lib.mmd_sdf_grid_windows(p, 46341, 46341, p, 1, 1, 1, p, None) != 0 and "32-bit" in lib.mmd_last_error().decode()
    assert lib.mmd_sdf_grid_windows(None, 37, 45, None, 0, 5, 7, None, None) == 0             # nothing to cut: nothing launched
    assert lib.mmd_sdf_grid_windows(None, 37, 45, None, 0, 38, 7, None, None) != 0            # (the sizes are checked all the same)
    lo, hi = (C.c_float * 2)(-1.0, -2.0), (C.c_float * 2)(1.0, 3.0)
    ok = (p, 31, 33, lo, hi, p, 5, p)
    flat = (C.c_float * 2)(1.0, -2.0)
    nan, inf = (C.c_float * 2)(float("nan"), 0.0), (C.c_float * 2)(0.0, float("inf"))
    for k, value, word in ((0, None, "NULL grid"), (5, None, "NULL points"), (7, None, "NULL out"), (3, None, "NULL limits"),
                           (4, None, "NULL limits"), (6, -1, "n_points"), (1, 0, "grid of"), (2, -1, "grid of"), (4, flat, "limits"),
                           (3, nan, "limits"), (4, nan, "limits"), (4, inf, "limits"), (3, inf, "limits")):
        args = list(ok)
        args[k] = value
        rc = lib.mmd_sdf_grid_lookup(*args, None)
        assert rc != 0 and word in lib.mmd_last_error().decode() and "mmd_sdf_grid_lookup" in lib.mmd_last_error().decode(), (args, rc)
    assert lib.mmd_sdf_grid_lookup(p, 65536, 65536, lo, hi, p, 5, p, None) != 0 and "32-bit" in lib.mmd_last_error().decode()
    assert lib.mmd_sdf_grid_lookup(None, 31, 33, lo, hi, None, 0, None, None) == 0            # no point: nothing launched
