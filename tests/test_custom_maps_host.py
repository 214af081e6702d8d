"""CPU: custom maps (environments.register_map).  The host texture (torch autograd) is the definition of a registered map's SDF grid;
tests/sdf_grid_model.py is the kernel's operation sequence in numpy, and g25 is GridMapSDF.precompute_sdf of the genuine reference on
the test map (tools/make_golden_maps.py).  All three agree bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import sdf_grid_model as M
from cases import GOLDEN
from mmd_amd import _lib, environments as E

SHIPPED = ("EnvEmpty2D", "EnvEmptyNoWait2D", "EnvHighways2D", "EnvConveyor2D", "EnvDropRegion2D")


@pytest.fixture
def registry():
    """Names registered by a test are gone after it."""
    before = set(E.registered_maps())
    yield
    for name in set(E.registered_maps()) - before:
        E.unregister_map(name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(a, b, what):
    """The same fp32 words, but for the sign of a zero: autograd leaves -0 (= 0 * -1) in a gradient where a field has a single primitive
    and +0 where several contributions are summed; the model and the device grid write +0."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = (bits(a) != bits(b)) & ~((a == 0) & (b == 0))
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} nodes differ, first at {np.argwhere(bad)[:4].tolist()}"


def node_rows():
    return [r.numpy() for r in E.grid_node_rows()]


@pytest.mark.parametrize("env_id", ["EnvHighways2D", "EnvConveyor2D", "EnvDropRegion2D", "EnvEmpty2D"])
def test_model_is_host_texture_on_shipped_maps(env_id):
    boxes, spheres = E.map_primitives(env_id)
    tex = E.sdf_grid_texture(env_id)
    assert_same_bits(M.sdf_grid(boxes, spheres, *node_rows()), tex, env_id)
    if env_id == "EnvEmpty2D":
        assert (tex == np.array([1, 0, 0, 0], np.float32)).all()
    else:
        assert tex[..., 0].max() < 1                                  # the constant 1 never acts on a shipped map


@pytest.mark.parametrize("with_spheres", [True, False])
def test_model_is_host_texture_on_test_map(registry, with_spheres):
    boxes, spheres = M.tie_map(with_spheres)
    E.register_map("TieMap", boxes, spheres)
    tex = E.sdf_grid_texture("TieMap")
    assert tex.shape == (400, 400, 4) and tex.dtype == np.float32 and not tex[..., 3].any()
    assert not (bits(tex) == 0x80000000).any()                        # (several primitives per field: autograd leaves no -0 here)
    assert_same_bits(M.sdf_grid(boxes, spheres, *node_rows()), tex, f"test map, spheres {with_spheres}")
    ties = {k: int(v.sum()) for k, v in M.tie_masks(boxes, spheres, *node_rows()).items()}
    print(ties)
    assert ties["box_diagonal"] >= 1
    if with_spheres:
        assert ties["equal_minimum"] >= 1 and ties["zero_norm"] >= 1
        ix, iy = M.TEST_SPHERE_NODE
        assert tex[ix, iy].tolist() == [pytest.approx(-0.15), 0.0, 0.0, 0.0]
    else:
        assert ties["capped"] >= 1
        assert (tex[..., 0] == 1).sum() == ties["capped"] and not tex[tex[..., 0] == 1][:, 1:].any()


def test_same_boxes_same_texture(registry):
    import torch
    boxes, spheres = E.map_primitives("EnvHighways2D")
    assert len(boxes) == 9 and spheres == ()
    E.register_map("HighwaysCopy", boxes)
    assert_same_bits(E.sdf_grid_texture("HighwaysCopy"), E.sdf_grid_texture("EnvHighways2D"), "texture")
    pts = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).uniform(-1, 1, (4096, 2)).astype(np.float32))
    assert_same_bits(E.map_sdf(pts, "HighwaysCopy").numpy(), E.map_sdf(pts, "EnvHighways2D").numpy(), "map_sdf")
    assert_same_bits(E.map_sdf(pts, "HighwaysCopyExtraObjects").numpy(), E.map_sdf(pts, "EnvHighways2D").numpy(), "map_sdf, suffix stripped")


@pytest.mark.parametrize("variant", ["with_spheres", "no_spheres"])
def test_host_texture_vs_reference(registry, variant):
    """g25: the reference's grid of the test map at ~8 000 listed nodes (random, tie and surface-ring nodes) and two checksums.  Bit for
    bit, as g3 is for the shipped maps."""
    g = np.load(os.path.join(GOLDEN, "g25_custom_map.npz"))
    boxes, spheres = M.tie_map(variant == "with_spheres")
    assert_same_bits(np.asarray(boxes, np.float32).reshape(-1, 4), g[f"{variant}.boxes"], "the fixture's boxes")
    assert_same_bits(np.asarray(spheres, np.float32).reshape(-1, 3), g[f"{variant}.spheres"], "the fixture's spheres")
    E.register_map("TieMap", boxes, spheres)
    tex = E.sdf_grid_texture("TieMap")
    assert tuple(g[f"{variant}.shape"]) == tex.shape[:2]
    idx = g[f"{variant}.idx"]
    assert len(idx) >= 7000
    assert_same_bits(tex[idx[:, 0], idx[:, 1], 0], g[f"{variant}.sdf"], "sdf")
    assert_same_bits(tex[idx[:, 0], idx[:, 1], 1:3], g[f"{variant}.grad"], "gradient")
    assert np.float64(tex[..., 0].astype(np.float64).sum()) == g[f"{variant}.sum_sdf"]
    assert np.float64(np.abs(tex[..., 1:3].astype(np.float64)).sum()) == g[f"{variant}.sum_abs_grad"]


def test_registry_refusals(registry):
    for name in SHIPPED + ("MyMapExtraObjects", "ExtraObjectsMap", ""):
        with pytest.raises(ValueError):
            E.register_map(name, [(0, 0, 0.1, 0.1)])
    E.register_map("Taken", [(0, 0, 0.1, 0.1)], [(0.5, 0.5, 0.1)])
    E.register_map("Taken", [(0, 0, 0.1, 0.1)], [(0.5, 0.5, 0.1)])                # the same content: a no-op
    with pytest.raises(ValueError, match="other primitives"):
        E.register_map("Taken", [(0, 0, 0.1, 0.2)], [(0.5, 0.5, 0.1)])
    for boxes, spheres in (([(0, 0, 0.1)], ()), ((), [(0, 0, 0.1, 0.1)]), ([[(0, 0, 0.1, 0.1)]], ()), ([(0, 0, 0.0, 0.1)], ()),
                           ([(0, 0, 0.1, -0.1)], ()), ((), [(0, 0, 0.0)]), ((), [(0, 0, -1.0)]), ((), [(0, 0, float("inf"))]),
                           ((), [(float("nan"), 0, 0.1)]), ([(0, float("inf"), 0.1, 0.1)], ()), ([(0, 0, float("nan"), 0.1)], ())):
        with pytest.raises(ValueError):
            E.register_map("Bad", boxes, spheres)
        assert "Bad" not in E.registered_maps()
    with pytest.raises(ValueError):
        E.unregister_map("NeverRegistered")
    with pytest.raises(ValueError):
        E.update_map("EnvHighways2D", [(0, 0, 0.1, 0.1)])
    with pytest.raises(KeyError):
        E.map_primitives("NeverRegistered")
    assert E.registered_maps() == ("Taken",)
    assert E.map_primitives("Taken") == (((0.0, 0.0, float(np.float32(0.1)), float(np.float32(0.1))),),
                                         ((0.5, 0.5, float(np.float32(0.1))),))


def test_reregistration_is_not_stale(registry):
    E.register_map("Moving", [(0.0, 0.0, 0.4, 0.4)])
    a = E.sdf_grid_texture("Moving")
    assert E.sdf_grid_texture("Moving") is a                                       # cached
    E.unregister_map("Moving")
    with pytest.raises(KeyError):
        E.sdf_grid_texture("Moving")
    E.register_map("Moving", (), [(0.3, 0.3, 0.2)])
    b = E.sdf_grid_texture("Moving")
    assert_same_bits(b, M.sdf_grid((), [(0.3, 0.3, 0.2)], *node_rows()), "after re-registration")
    assert not np.array_equal(a, b)


def test_has_obstacles_and_shipped_maps_unchanged(registry):
    assert tuple(E.MAP_BOXES) == SHIPPED and E.LIMITS == ((-1.0, -1.0), (1.0, 1.0)) and E.SDF_CELL_SIZE == 0.005
    assert [E.map_has_obstacles(m) for m in SHIPPED] == [False, False, True, True, True]
    assert E.map_has_obstacles("EnvHighways2DExtraObjects") and not E.map_has_obstacles("EnvEmpty2DExtraObjects")
    E.register_map("Bare")
    assert E.map_has_obstacles("Bare") and E.map_primitives("Bare") == ((), ())    # a registered map always has a grid
    assert (E.sdf_grid_texture("Bare") == np.array([1, 0, 0, 0], np.float32)).all()
    g = np.load(os.path.join(GOLDEN, "g3_sdf.npz"))
    for env_id in ("EnvEmpty2D", "EnvHighways2D", "EnvConveyor2D", "EnvDropRegion2D"):
        tex, idx = E.sdf_grid_texture(env_id), g[f"{env_id}.idx"]
        assert_same_bits(tex[idx[:, 0], idx[:, 1], 0], g[f"{env_id}.sdf"], env_id)
        assert_same_bits(tex[idx[:, 0], idx[:, 1], 1:3], g[f"{env_id}.grad"], env_id)
        assert np.float64(tex[..., 0].astype(np.float64).sum()) == g[f"{env_id}.sum_sdf"]


def test_instances_on_a_registered_map(registry):
    from mmd_amd.trials import get_start_goal_pos_random_in_env
    from mmd_amd.world import random_world_instance
    boxes, spheres = M.tie_map()
    E.register_map("TieMap", boxes, spheres)
    starts, goals, offsets = random_world_instance(24, 6.0, seed=1, env_id="TieMap")
    assert set(np.unique(offsets).tolist()) <= {-2.0, 0.0, 2.0} and len({tuple(o) for o in offsets.tolist()}) > 1     # snapped
    assert (E.map_sdf(starts - offsets, "TieMap").numpy() > 0).all() and (E.map_sdf(goals - offsets, "TieMap").numpy() > 0).all()
    E.register_map("Bare")
    assert set(np.unique(random_world_instance(8, 6.0, seed=1, env_id="Bare")[2]).tolist()) <= {-2.0, 0.0, 2.0}     # snapped: it has a grid
    s, g = get_start_goal_pos_random_in_env(6, "TieMap", seed=2)
    pts = np.asarray(s + g, np.float32).reshape(12, 2)
    assert (E.map_sdf(pts, "TieMap").numpy() > 0.15).all()
    s2, g2 = get_start_goal_pos_random_in_env(6, "TieMap", seed=2)
    assert np.array_equal(np.asarray(s2 + g2, np.float32), np.asarray(s + g, np.float32))


def test_abi_symbol_and_argument_checks():
    """mmd_sdf_grid_build is declared, exported and additive (the ABI version stays 9); its argument checks return non-zero with a message
    before any device call: there is no GPU here, a check that came after a launch could not answer like this."""
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmd_amd.h")).read()
    assert "int mmd_sdf_grid_build(" in header and "mmd_sdf_grid_build" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 9 and lib.mmd_abi_version() == 9
    p = C.c_void_p(4096)              # never read: every call below is refused
    for args, word in (((None, 3, None, 0, p, 4, p, 4, p), "n_spheres"), ((p, -1, None, 0, p, 4, p, 4, p), "n_spheres"),
                       ((None, 0, None, 2, p, 4, p, 4, p), "n_boxes"), ((None, 0, p, -2, p, 4, p, 4, p), "n_boxes"),
                       ((None, 0, None, 0, p, 0, p, 4, p), "nodes"), ((None, 0, None, 0, p, 4, p, -1, p), "nodes"),
                       ((None, 0, None, 0, p, 1 << 16, p, 1 << 15, p), "32-bit"), ((None, 0, None, 0, None, 4, p, 4, p), "coordinates"),
                       ((None, 0, None, 0, p, 4, None, 4, p), "coordinates"), ((None, 0, None, 0, p, 4, p, 4, None), "grid")):
        rc = lib.mmd_sdf_grid_build(*args, None)
        assert rc != 0 and word in lib.mmd_last_error().decode(), (args, rc, lib.mmd_last_error())
