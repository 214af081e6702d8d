"""CPU: occupancy maps (environments.register_occupancy_map).  environments.occupancy_sdf_texture (numpy, the two-pass exact distance
transform with nearest-site tracking) is the definition of such a map's SDF texture; tests/occupancy_model.py holds the brute-force
lexicographic model and the kernels' operation sequence, and g26 is scipy's distance transform of the test map
(tools/make_golden_occupancy.py).  All agree exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import occupancy_model as M
from cases import GOLDEN
from mmd_amd import _lib, environments as E

SMALL = M.small_grids()


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    before = set(E.registered_maps())
    yield
    for name in set(E.registered_maps()) - before:
        E.unregister_map(name)


@pytest.fixture(scope="module")
def test_map():
    occ = M.test_occupancy()
    occ.setflags(write=False)
    tex = E.occupancy_sdf_texture(occ)
    tex.setflags(write=False)
    return occ, tex


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_texture_invariants(tex, what):
    assert tex.dtype == np.float32 and tex.shape[2] == 4 and not tex[..., 3].any(), what
    assert not (bits(tex) == 0x80000000).any(), f"{what}: a word is -0"
    assert np.isfinite(tex).all() and tex[..., 0].min() >= -1 and tex[..., 0].max() <= 1, what
    const = np.abs(tex[..., 0]) == 1
    assert not tex[const][:, 1:].any(), f"{what}: a constant cell with a gradient"
    if (~const).any():
        g = tex[~const]
        norm = np.sqrt(g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
        assert np.abs(norm - np.float32(1)).max() <= 2e-7, (what, float(np.abs(norm - 1).max()))


@pytest.mark.parametrize("case", list(SMALL))
def test_definition_is_the_brute_force(case):
    """D2 and argmin (through the value and the gradient, which are injective in them at a fixed cell) and, directly, the integer nearest
    site of the two-pass form against the lexicographic brute force."""
    occ, cell = SMALL[case]
    tex = E.occupancy_sdf_texture(occ, cell)
    assert tex.shape == occ.shape + (4,)
    assert np.array_equal(bits(tex), bits(M.brute_texture(occ, cell))), case
    assert np.array_equal(bits(tex), bits(M.kernel_texture(occ, cell))), case                  # the kernels' sequence is the same function
    assert_texture_invariants(tex, case)
    ix, iy = np.indices(occ.shape)
    for site in (occ != 0, occ == 0):
        if site.any():
            d2, dx, dy = E._nearest_site(site)
            b2, bx, by = M.brute_nearest(site)
            assert np.array_equal(d2, b2) and np.array_equal(ix - dx, bx) and np.array_equal(iy - dy, by), case
    if case == "1x1 free":
        assert tex.tolist() == [[[1, 0, 0, 0]]]
    if case == "1x1 occupied":
        assert tex.tolist() == [[[-1, 0, 0, 0]]]
    if case == "31x33 coarse":
        capped = (tex[..., 0] == 1) & (occ == 0)
        assert capped.any() and not capped.all() and (tex[..., 0] < 0).sum() == occ.sum()
    if case == "corner 7x5":
        f = np.float32
        assert tex[0, 0].tolist() == [-f(0.0025), 0, 1, 0]                                    # site (0, 1) precedes (1, 0): the tie rule
        assert tex[6, 4, 0] == f(0.005) * np.sqrt(f(52)) - f(0.5) * f(0.005)


def test_all_free_and_all_occupied():
    for shape in ((5, 9), (400, 400)):
        assert (E.occupancy_sdf_texture(np.zeros(shape)) == np.array([1, 0, 0, 0], np.float32)).all()
        assert (E.occupancy_sdf_texture(np.ones(shape)) == np.array([-1, 0, 0, 0], np.float32)).all()
    for bad in (np.zeros((3,)), np.zeros((2, 2, 2)), np.zeros((0, 4)), np.zeros((2049, 1))):
        with pytest.raises(ValueError):
            E.occupancy_sdf_texture(bad)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            E.occupancy_sdf_texture(np.zeros((3, 3)), cell)


def test_test_map_vs_scipy(test_map):
    """g26: scipy's squared distance transform of the test map at ~8 000 listed nodes and its sums over both classes."""
    occ, tex = test_map
    g = np.load(os.path.join(GOLDEN, "g26_occupancy_map.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "g26_occupancy_map.npz")) < 100_000
    assert tuple(g["shape"]) == occ.shape and np.array_equal(np.unpackbits(g["bits"]).reshape(occ.shape), occ)
    assert 0.05 <= occ.mean() <= 0.30
    idx = g["idx"].astype(np.int64)
    assert len(idx) >= 7000
    to_occ, to_free = E._nearest_site(occ != 0)[0].astype(np.int64), E._nearest_site(occ == 0)[0].astype(np.int64)
    d2 = np.where(occ != 0, to_free, to_occ)
    assert np.array_equal(d2[idx[:, 0], idx[:, 1]], g["d2"])
    assert int(to_occ[occ == 0].sum()) == int(g["sum_d2_free"]) and int(to_free[occ != 0].sum()) == int(g["sum_d2_occupied"])
    # the texture's value is that D2's, cell by cell
    f = np.float32
    v = f(0.005) * np.sqrt(d2.astype(f)) - f(0.5) * f(0.005)
    assert np.array_equal(bits(tex[..., 0]), bits(np.where(occ != 0, -v, v)))
    assert_texture_invariants(tex, "test map")
    assert np.array_equal(bits(tex), bits(M.kernel_texture(occ, 0.005)))
    ties = M.tie_mask(occ)
    assert ties[230, 360] and ties[110, 340] and ties[idx[:, 0], idx[:, 1]].sum() >= 1000
    assert tex[110, 340].tolist() == [f(0.005) * np.sqrt(f(200)) - f(0.0025), f(10) / np.sqrt(f(200)), f(10) / np.sqrt(f(200)), 0]   # site (100, 330)
    assert tex[230, 360, 1:3].tolist() == [0, 1]                                               # site (230, 350), not (230, 370)
    assert tex[97, 200, 0] > 0 and tex[75, 255, 0] < 0 and tex[80, 260, 0] > 0 and tex[0, 0, 0] < 0


def test_registry(registry, test_map):
    occ, tex = test_map
    for name in ("EnvEmpty2D", "EnvHighways2D", "MyMapExtraObjects", "", None):
        with pytest.raises(ValueError):
            E.register_occupancy_map(name, occ)
    for bad in (np.zeros((400, 399)), np.zeros((200, 200)), np.zeros((400,)), np.zeros((400, 400, 1)), [["a"] * 400] * 400):
        with pytest.raises(ValueError):
            E.register_occupancy_map("Bad", bad)
        assert "Bad" not in E.registered_maps()
    E.register_occupancy_map("Floor", occ)
    E.register_occupancy_map("Floor", occ.astype(np.float64) * 3.5)                            # the same cells: a no-op
    E.register_occupancy_map("Floor", (occ != 0).tolist())
    other = occ.copy()
    other[200, 10] = 1
    with pytest.raises(ValueError, match="another bitmap"):
        E.register_occupancy_map("Floor", other)
    with pytest.raises(ValueError, match="occupancy map"):
        E.register_map("Floor", [(0, 0, 0.1, 0.1)])
    with pytest.raises(ValueError, match="occupancy map"):
        E.register_map("Floor")
    E.register_map("Prims", [(0, 0, 0.1, 0.1)])
    with pytest.raises(ValueError, match="primitives"):
        E.register_occupancy_map("Prims", occ)
    with pytest.raises(ValueError, match="occupancy map"):
        E.update_map("Floor", [(0, 0, 0.1, 0.1)])
    with pytest.raises(ValueError, match="primitives"):
        E.update_occupancy_map("Prims", occ)
    for name in ("EnvHighways2D", "NeverRegistered"):
        with pytest.raises(ValueError):
            E.update_occupancy_map(name, occ)
    with pytest.raises(ValueError):
        E.map_primitives("Floor")
    with pytest.raises(ValueError):
        E.map_occupancy("Prims")
    with pytest.raises(ValueError):
        E.update_occupancy_map("Floor", np.zeros((10, 10)))
    assert E.registered_maps() == ("Floor", "Prims")
    assert E.is_registered("Floor") and E.is_registered("FloorExtraObjects") and E.is_registered("Prims") and not E.is_registered("EnvEmpty2D")
    assert E.is_occupancy_map("Floor") and not E.is_occupancy_map("Prims")
    assert E.map_has_obstacles("Floor") and E.map_has_obstacles("FloorExtraObjects")
    got = E.map_occupancy("Floor")
    assert got.dtype == np.uint8 and np.array_equal(got, occ)
    got[:] = 0
    assert np.array_equal(E.map_occupancy("Floor"), occ)                                       # a copy
    assert np.array_equal(bits(E.sdf_grid_texture("Floor")), bits(tex))
    assert E.sdf_grid_texture("Floor") is E.sdf_grid_texture("FloorExtraObjects")              # cached, by base name
    E.unregister_map("Floor")
    assert E.registered_maps() == ("Prims",) and not E.is_registered("Floor")
    with pytest.raises(ValueError):
        E.unregister_map("Floor")


def test_reregistration_is_not_stale(registry, test_map):
    occ, tex = test_map
    E.register_occupancy_map("Moving", occ)
    a = E.sdf_grid_texture("Moving")
    assert E.sdf_grid_texture("Moving") is a
    E.unregister_map("Moving")
    with pytest.raises(KeyError):
        E.sdf_grid_texture("Moving")
    E.register_occupancy_map("Moving", np.zeros((400, 400), bool))
    assert (E.sdf_grid_texture("Moving") == np.array([1, 0, 0, 0], np.float32)).all() and E.map_has_obstacles("Moving")
    E.unregister_map("Moving")
    E.register_map("Moving", [(0.0, 0.0, 0.4, 0.4)])                                           # the other kind under the freed name
    assert E.sdf_grid_texture("Moving")[200, 200, 0] < 0 and not E.is_occupancy_map("Moving")
    E.unregister_map("Moving")
    E.register_occupancy_map("Moving", occ)
    assert np.array_equal(bits(E.sdf_grid_texture("Moving")), bits(tex))
    # update without a resident texture: the registry and the host texture follow
    flipped = np.ascontiguousarray(occ[::-1])
    E.update_occupancy_map("Moving", flipped)
    assert np.array_equal(E.map_occupancy("Moving"), flipped)
    assert np.array_equal(bits(E.sdf_grid_texture("Moving")[..., 0]), bits(tex[::-1, :, 0]))


def _cell_value(tex, pts):
    f = np.float32
    idx = np.clip(np.floor((np.asarray(pts, f) - f(-1)) / f(2) * f(400)).astype(np.int64), 0, 399)
    return tex[idx[:, 0], idx[:, 1], 0]


def test_map_sdf_and_instances(registry, test_map):
    import torch
    from mmd_amd.trials import get_start_goal_pos_random_in_env
    from mmd_amd.world import OBSTACLE_MARGIN, random_world_instance
    occ, tex = test_map
    E.register_occupancy_map("Floor", occ)
    pts = np.random.Generator(np.random.PCG64(7)).uniform(-1.02, 1.02, (4096, 2)).astype(np.float32)
    got = E.map_sdf(torch.from_numpy(pts), "Floor")
    assert got.dtype == torch.float32 and np.array_equal(bits(got.numpy()), bits(_cell_value(tex, pts)))
    assert np.array_equal(bits(E.map_sdf(pts.reshape(64, 64, 2), "FloorExtraObjects").numpy()), bits(_cell_value(tex, pts).reshape(64, 64)))
    # cell (ix, iy) covers [lo + ix * cell, lo + (ix + 1) * cell): the centre of an occupied cell is inside, of a free one outside
    centres = (np.argwhere(occ != 0)[::97] + 0.5) * 0.005 - 1
    assert (E.map_sdf(centres.astype(np.float32), "Floor").numpy() < 0).all()
    starts, goals, offsets = random_world_instance(24, 6.0, seed=1, env_id="Floor")
    assert set(np.unique(offsets).tolist()) <= {-2.0, 0.0, 2.0} and len({tuple(o) for o in offsets.tolist()}) > 1
    assert (_cell_value(tex, starts - offsets) > OBSTACLE_MARGIN).all() and (_cell_value(tex, goals - offsets) > OBSTACLE_MARGIN).all()
    s, g = get_start_goal_pos_random_in_env(6, "Floor", seed=2)
    assert (_cell_value(tex, np.asarray(s + g, np.float32).reshape(12, 2)) > 0.16).all()
    s2, g2 = get_start_goal_pos_random_in_env(6, "Floor", seed=2)
    assert np.array_equal(np.asarray(s2 + g2, np.float32), np.asarray(s + g, np.float32))


def test_abi_symbols_and_argument_checks():
    """Both entry points are declared, exported and additive (ABI 9, the pinned struct sizes stay); the argument checks answer non-zero
    with a message before any device call: there is no GPU here, a check behind a launch could not answer like this."""
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmd_amd.h")).read()
    assert "size_t mmd_sdf_grid_occupancy_work_bytes(int nx, int ny);" in header and "int mmd_sdf_grid_from_occupancy(" in header
    assert "mmd_sdf_grid_occupancy_work_bytes" in _lib.EXPORTED_SYMBOLS and "mmd_sdf_grid_from_occupancy" in _lib.EXPORTED_SYMBOLS
    assert "mmd_sdf_grid_build" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9
    assert C.sizeof(_lib.ConsBins) == 56 and C.sizeof(_lib.Conflict) == 48 and C.sizeof(_lib.UnetOptions) == 20
    work = lib.mmd_sdf_grid_occupancy_work_bytes
    assert work(400, 400) == 2 * 2 * 400 * 400 and work(1, 1) == 4 and work(2048, 2048) == 4 * 2048 * 2048 and work(7, 5) == 140
    assert work(0, 4) == 0 and work(4, -1) == 0 and work(2049, 4) == 0 and work(4, 2049) == 0
    p = C.c_void_p(4096)              # never read: every call below is refused
    ok = (p, 4, 4, 0.005, p, p, 64)
    for k, value, word in ((0, None, "occupancy"), (4, None, "grid"), (5, None, "workspace"), (1, 0, "cells"), (2, 0, "cells"),
                           (1, -3, "cells"), (1, 2049, "cells"), (2, 2049, "cells"), (3, 0.0, "cell ="), (3, -0.005, "cell ="),
                           (3, float("nan"), "cell ="), (3, float("inf"), "cell ="), (6, 63, "work_bytes"), (6, 0, "work_bytes")):
        args = list(ok)
        args[k] = value
        rc = lib.mmd_sdf_grid_from_occupancy(*args, None)
        assert rc != 0 and word in lib.mmd_last_error().decode(), (args, rc, lib.mmd_last_error())


def test_occupancy_from_ascii_and_resize():
    rows = ["@..",
            "..T",
            "...",
            "W.O"]
    occ = E.occupancy_from_ascii(rows)
    assert occ.dtype == np.uint8 and occ.shape == (3, 4)                                       # [columns = x, rows = y]
    # x runs along a text row, y runs up: the first text row is iy = 3
    assert occ.tolist() == [[1, 0, 0, 1], [0, 0, 0, 0], [1, 0, 1, 0]]
    assert E.occupancy_from_ascii(rows, occupied="T").sum() == 1 and E.occupancy_from_ascii(rows, occupied="T")[2, 2] == 1
    assert E.occupancy_from_ascii(["."]).tolist() == [[0]]
    for bad in (["..", "..."], [], [""], ["...", ""]):
        with pytest.raises(ValueError):
            E.occupancy_from_ascii(bad)
    big = E.resize_occupancy(occ)
    assert big.shape == (400, 400) and big.dtype == np.uint8
    # 3 -> 400: cell i takes source (2 i + 1) * 3 // 800; 4 -> 400: blocks of 100
    assert big[:, 0].tolist() == [1] * 133 + [0] * 134 + [1] * 133 and big[0].tolist() == [1] * 100 + [0] * 200 + [1] * 100
    assert np.array_equal(E.resize_occupancy(occ, (3, 4)), occ)
    assert E.resize_occupancy(occ, (6, 2)).tolist() == [[0, 1], [0, 1], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert E.resize_occupancy(np.eye(5), (1, 1)).tolist() == [[1]]                             # the centre cell
    small = E.resize_occupancy(big, (3, 4))
    assert np.array_equal(small, occ)
    for bad_shape in ((0, 4), (4, -1)):
        with pytest.raises(ValueError):
            E.resize_occupancy(occ, bad_shape)
