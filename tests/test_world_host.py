"""CPU: the host side of many-robot rounds with per-robot frames (mmd_framed_constraints_from_paths; constraints.framed_constraints_from_paths,
framed_slot_bound; world.WorldRobotSampler, random_world_instance) -- the numpy model of the framed table pinned to mmd_pack_constraints
word for word, the exactness of the culling replayed in fp32, the error paths decided before any launch, the signatures and the op's
meta shapes."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import world_model as M
from mmd_amd import _lib

H = 64
FAKE = 0x1000                                                # a non-NULL "device pointer": every call below returns before its launch
NAME = "mmd_framed_constraints_from_paths"


def test_abi_stays_9_and_has_the_entry_point():
    assert _lib.ABI_VERSION == 9 and _lib.load().mmd_abi_version() == 9
    assert NAME in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[NAME][1]) == 18
    assert hasattr(_lib.load(), NAME)


def test_op_meta_shapes():
    import torch
    import mmd_amd.ops  # noqa: F401
    paths = torch.zeros(37, 64, 2, device="meta")
    offsets = torch.zeros(37, 2, device="meta")
    ell, gso, gw, rgo, used, dropped = torch.ops.mmd_amd.framed_constraints_from_paths(paths, offsets, 5, 3, 7, 0.12, 0.02, -1.1, -1.1, 1.1, 1.1)
    assert ell.shape == (3 * 7, 64, 4) and ell.dtype == torch.float32
    assert gso.shape == (4,) and gso.dtype == torch.int32 and gw.shape == (3,) and gw.dtype == torch.float32
    assert rgo.shape == (4,) and rgo.dtype == torch.int32
    assert used.shape == (3,) and used.dtype == torch.int32 and dropped.shape == (3,) and dropped.dtype == torch.int32


def test_entry_point_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = ("paths", "offsets", "ell", "gso", "gw", "rgo", "used", "dropped")

    def call(n_all=8, robot0=2, n_local=3, horizon=64, slots=4, radius=0.12, wlo=(-1.1, -1.1), whi=(1.1, 1.1), **ptr):
        p = {k: ptr.get(k, FAKE) for k in names}
        lo = (C.c_float * 2)(*wlo) if wlo is not None else None
        hi = (C.c_float * 2)(*whi) if whi is not None else None
        rc = lib.mmd_framed_constraints_from_paths(p["paths"], p["offsets"], n_all, robot0, n_local, horizon, slots, radius, 0.02, lo, hi,
                                                   p["ell"], p["gso"], p["gw"], p["rgo"], p["used"], p["dropped"], None)
        return rc, lib.mmd_last_error().decode()

    cases = [({k: None}, "NULL") for k in names] + [({"wlo": None}, "NULL"), ({"whi": None}, "NULL")] + [
        ({"horizon": 63}, "horizon"), ({"horizon": 128}, "horizon"),
        ({"n_all": 1, "robot0": 0, "n_local": 1, "slots": 1}, "n_all"), ({"n_all": 4097}, "n_all"),
        ({"robot0": -1}, "robot range"), ({"robot0": 8}, "robot range"), ({"robot0": 6}, "robot range"), ({"n_local": 0}, "robot range"),
        ({"n_local": 7}, "robot range"),
        ({"slots": 0}, "slots"), ({"slots": 8}, "slots"), ({"slots": -2}, "slots"),
        ({"radius": 0.0}, "radius"), ({"radius": -0.12}, "radius"),
        ({"wlo": (1.1, -1.1)}, "window"), ({"whi": (1.1, -1.1)}, "window"), ({"wlo": (-1.1, 1.1)}, "window"),
        ({"wlo": (float("nan"), -1.1)}, "window")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc != 0 and text in err and NAME in err, (kw, rc, err)


def _instance(rng, n, spread):
    """n robots at offsets within `spread`, every global path inside its own window, with a few points pushed out of it"""
    offsets = rng.uniform(-spread, spread, (n, 2)).astype(np.float32)
    offsets[rng.integers(0, n)] = 0.0
    paths = (rng.uniform(-1.0, 1.0, (n, H, 2)).astype(np.float32) + offsets[:, None, :]).astype(np.float32)
    return paths, offsets


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_is_pack_constraints_word_for_word(seed):
    """mmd_pack_constraints' slot rule: the host pack of the model's included points, per robot, IS the model's table"""
    from mmd_amd.constraints import CostConstraint, pack_constraints
    rng = np.random.default_rng(900 + seed)
    n = 9 + seed
    paths, offsets = _instance(rng, n, [0.0, 1.2, 2.5][seed])
    paths[1, 7] = np.nan
    wlo, whi = M.default_window()
    robot0, n_local = 2, 4
    groups, n_pts = [], []
    for r in range(robot0, robot0 + n_local):
        q, tr = M.point_list(paths, offsets, r, wlo, whi)
        assert len(tr) > 0
        n_pts.append(len(tr))
        groups.append([(CostConstraint(None, H, q_l=[v for v in q], traj_range_l=tr, radius_l=[M.RADIUS] * len(tr), is_soft=True), 2e-2)])
    ell_h, gso_h, gw_h, rgo_h = (v.numpy() for v in pack_constraints(groups, "cpu"))
    full = M.framed_table(paths, offsets, robot0, n_local, n - 1)
    assert int(full[5].sum()) == 0
    if seed > 0:
        assert int(full[4].min()) < n - 1                          # some robot does not see every other: the culling is at work
    for i in range(n_local):
        blk = ell_h[gso_h[i]:gso_h[i + 1]]
        used = int(full[4][i])
        assert blk.shape[0] == used and (blk[..., 2] >= 0).sum() == n_pts[i]
        mine = full[0][i * (n - 1):(i + 1) * (n - 1)]
        assert np.array_equal(mine[:used].view(np.int32), blk.view(np.int32)), (seed, i)
        assert np.array_equal(mine[used:], np.tile(M.EMPTY, (n - 1 - used, H, 1)))
        assert np.array_equal(mine[:, 0], np.tile(M.EMPTY, (n - 1, 1)))
        fill = (blk[..., 2] >= 0).sum(0)
        # the cap: the first S slots of the same pack, the rest counted
        for S in {1, max(used - 1, 1)}:
            cut = M.framed_table(paths, offsets, robot0 + i, 1, S)
            assert np.array_equal(cut[0].view(np.int32), blk[:S].view(np.int32)), (seed, i, S)
            assert cut[4][0] == min(used, S) and cut[5][0] == int(np.maximum(fill - S, 0).sum())
    assert np.array_equal(gw_h, full[2]) and np.array_equal(rgo_h, full[3])
    assert np.array_equal(full[1], np.arange(n_local + 1) * (n - 1))


def test_model_meets_the_edges_of_the_gpu_instance():
    """the instance of the kernel's bit-for-bit test holds what it says: on / one ulp off an edge, a NaN, a shared point, an empty time
    step, drops"""
    paths, offsets = M.edge_instance()
    wlo, whi = M.default_window()
    _, inc2 = M.included(paths, offsets, 2, wlo, whi)
    _, inc3 = M.included(paths, offsets, 3, wlo, whi)
    assert inc2[0, 5] and not inc2[1, 5] and inc2[6, 5]
    assert inc3[0, 6] and not inc3[1, 6] and inc3[6, 6]
    assert not inc2[0, 7] and not inc2[1, 7] and not inc3[0, 7]
    assert inc2[0, 8] and inc2[1, 8] and np.array_equal(paths[0, 8], paths[1, 8])
    assert not inc2[:, 9].any() and not inc3[:, 9].any()
    ell, gso, gw, rgo, used, dropped = M.framed_table(paths, offsets, 2, 3, 3)
    assert used.max() == 3 and dropped[0] >= 3 and inc2[:, 10].sum() == 6
    assert np.array_equal(ell[:, 0], np.tile(M.EMPTY, (9, 1)))


def test_culling_is_exact_in_fp32():
    """A point q outside the default window is farther than the radius from every position p the guided step can measure from: p inside
    the position limits, the corners and one ulp beyond them (the rounding of the un-normalisation) included.  The distance is the
    kernels' own forms, sqrt(fma(dy, dy, dx * dx)) > R and fma(dx, dx, dy * dy) > R|R|, replayed in fp32; a q ON the window's edge is
    still included."""
    R = M.RADIUS
    wlo, whi = M.default_window()
    one, inf = np.float32(1.0), np.float32(np.inf)
    edge = [-one, np.nextafter(-one, -inf), np.nextafter(-one, inf), one, np.nextafter(one, inf), np.nextafter(one, -inf), np.float32(0.0)]
    rng = np.random.default_rng(5)
    ps = np.array([(x, y) for x in edge for y in edge], np.float32)
    ps = np.concatenate([ps, rng.uniform(-1, 1, (200, 2)).astype(np.float32)])
    out_x = [np.nextafter(whi[0], inf), np.nextafter(wlo[0], -inf), whi[0] + np.float32(1e-3), wlo[0] - np.float32(5.0)]
    qs = [(x, y) for x in out_x for y in (np.float32(-1.0), np.float32(0.3), np.float32(1.0), wlo[1], whi[1])]
    qs += [(y, x) for x, y in qs]
    qs = np.array(qs, np.float32)
    dx = (ps[:, None, 0] - qs[None, :, 0]).astype(np.float32)
    dy = (ps[:, None, 1] - qs[None, :, 1]).astype(np.float32)
    dxx = (dx * dx).astype(np.float32)
    s = (dy.astype(np.float64) * dy.astype(np.float64) + dxx.astype(np.float64)).astype(np.float32)         # fma: one rounding
    d = np.sqrt(s).astype(np.float32)
    assert (d > R).all() and (s > R * np.abs(R)).all()
    dyy = (dy * dy).astype(np.float32)                                           # the guided step's own form: fma(dx, dx, dy * dy) <= R|R| acts
    d2 = (dx.astype(np.float64) * dx.astype(np.float64) + dyy.astype(np.float64)).astype(np.float32)
    assert (d2 > R * np.abs(R)).all()
    assert float(d.min()) > float(R) * 1.06                                      # the 1/16 slack, less a few ulp
    # on the edge: included by the closed compare (robot 1's frame at offset 0: q = the point itself)
    on_edge = np.zeros((2, H, 2), np.float32)
    on_edge[0, 1] = (whi[0], wlo[1])
    on_edge[0, 2] = (np.nextafter(whi[0], inf), wlo[1])
    _, inc = M.included(on_edge, np.zeros((2, 2), np.float32), 1, wlo, whi)
    assert inc[0, 1] and not inc[0, 2]
    # and the Python layer's default window is the model's, bit for bit
    from mmd_amd.constraints import framed_window
    from mmd_amd.environments import LIMITS
    lo, hi = framed_window(LIMITS, float(R))
    assert lo.dtype == np.float32 and np.array_equal(lo, wlo) and np.array_equal(hi, whi)


def test_framed_slot_bound_is_the_brute_force_count():
    from mmd_amd.constraints import framed_slot_bound
    from mmd_amd.environments import LIMITS
    rng = np.random.default_rng(11)
    for n, spread in ((12, 3.0), (40, 6.0), (40, 1.0), (5, 30.0)):
        offsets = rng.uniform(-spread, spread, (n, 2)).astype(np.float32)
        for robot0, n_local in ((0, n), (3, 2), (n - 1, 1)):
            assert framed_slot_bound(offsets, robot0, n_local, LIMITS, float(M.RADIUS)) == M.slot_bound(offsets, robot0, n_local)
    assert framed_slot_bound(np.zeros((9, 2), np.float32), 2, 3, LIMITS, 0.12) == 8                # identical offsets: N - 1
    far = np.array([[0, 0], [10, 0], [20, 0]], np.float32)
    assert framed_slot_bound(far, 0, 3, LIMITS, 0.12) == 1                                        # clamped from below
    # no drop at the bound while every path stays in its own window
    offsets = rng.uniform(-2.5, 2.5, (30, 2)).astype(np.float32)
    paths = (rng.uniform(-1.0, 1.0, (30, H, 2)).astype(np.float32) + offsets[:, None, :]).astype(np.float32)
    S = framed_slot_bound(offsets, 0, 30, LIMITS, float(M.RADIUS))
    assert S < 29
    table = M.framed_table(paths, offsets, 0, 30, S)
    assert int(table[5].sum()) == 0 and int(table[4].max()) <= S
    with pytest.raises(ValueError):
        framed_slot_bound(offsets, 29, 2, LIMITS, 0.12)


def test_random_world_instance():
    from mmd_amd.world import random_world_instance
    a = random_world_instance(48, 5.0, seed=3)
    b = random_world_instance(48, 5.0, seed=3)
    c = random_world_instance(48, 5.0, seed=4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
    for env_id in ("EnvEmpty2D", "EnvHighways2D"):
        starts, goals, offsets = random_world_instance(24, 6.0, seed=1, env_id=env_id)
        assert all(v.dtype == np.float32 and v.shape == (24, 2) for v in (starts, goals, offsets))
        for p in (starts, goals):
            d = np.sqrt(((p[:, None] - p[None, :]).astype(np.float64) ** 2).sum(-1))
            assert d[~np.eye(24, dtype=bool)].min() > 0.15
            local = p - offsets
            assert (local >= -1.0).all() and (local <= 1.0).all()
        assert (np.abs(offsets) <= 2.0).all()                                  # the window lies inside the world
        if env_id == "EnvHighways2D":
            from mmd_amd.environments import map_sdf
            assert set(np.unique(offsets).tolist()) <= {-2.0, 0.0, 2.0}        # snapped to the tile pitch: three tiles per axis
            assert len({tuple(o) for o in offsets.tolist()}) > 1
            assert (map_sdf(starts - offsets, env_id).numpy() > 0).all() and (map_sdf(goals - offsets, env_id).numpy() > 0).all()
    with pytest.raises(RuntimeError, match="not placed"):
        random_world_instance(400, 2.0, seed=0, max_draws=5000)


def test_world_sampler_surface_and_refusals():
    from mmd_amd.multi_robot import MultiRobotSampler, PlanResult
    from mmd_amd.world import WorldRobotSampler
    assert issubclass(WorldRobotSampler, MultiRobotSampler)
    p = inspect.signature(WorldRobotSampler.__init__).parameters
    base = inspect.signature(MultiRobotSampler.__init__).parameters
    assert list(p)[:5] == ["self", "model", "starts", "goals", "offsets"] and list(p)[-1] == "neighbor_slots"
    assert p["neighbor_slots"].default is None
    assert [(k, p[k].default is base[k].default or p[k].default == base[k].default) for k in list(base)[4:]] == [(k, True) for k in list(base)[4:]]
    # refused before any device work: a stand-in object is enough to meet them
    fake = types.SimpleNamespace(constraint_table="dense", inter_robot=True)
    with pytest.raises(ValueError, match="repair"):
        WorldRobotSampler.plan_rounds_subset(fake, repair=True)
    with pytest.raises(ValueError, match="repair"):
        WorldRobotSampler.plan_rounds(fake, repair=True)
    for mode in ("conflicted", "independent"):
        with pytest.raises(ValueError, match="replan"):
            WorldRobotSampler.plan_rounds_subset(fake, replan=mode)
    starts = np.array([[0.2, 0.2], [6.5, 0.0]], np.float32)
    goals = np.array([[-0.5, 0.1], [5.5, 0.5]], np.float32)
    offsets = np.array([[0.0, 0.0], [6.0, 0.0]], np.float32)
    for bad_starts, bad_goals, word in ((starts + np.float32([[0, 0], [0.6, 0]]), goals, "start"),
                                        (starts, goals - np.float32([[0.6, 0], [0, 0]]), "goal")):
        with pytest.raises(ValueError, match=word):
            WorldRobotSampler.__init__(types.SimpleNamespace(), None, bad_starts, bad_goals, offsets, device="cpu")
    with pytest.raises(ValueError, match="offsets"):
        WorldRobotSampler.__init__(types.SimpleNamespace(), None, starts, goals, offsets[:1], device="cpu")
    with pytest.raises(ValueError, match="neighbor_slots"):
        WorldRobotSampler.__init__(types.SimpleNamespace(), None, starts, goals, offsets, device="cpu", neighbor_slots=2)
    assert PlanResult(1, 2, 3, 4, 5, 6, 7).dropped_constraints is None


def test_base_class_is_untouched():
    from mmd_amd.multi_robot import MultiRobotSampler
    p = inspect.signature(MultiRobotSampler.__init__).parameters
    assert list(p) == ["self", "model", "starts", "goals", "env_id", "n_samples", "rank", "world_size", "norm_mins", "norm_maxs",
                       "n_guide_steps", "start_guide_steps_fraction", "n_diffusion_steps_without_noise",
                       "weight_grad_cost_soft_constraints", "radius", "device", "group", "n_streams", "inter_robot", "constraint_table"]
    assert list(inspect.signature(MultiRobotSampler.plan).parameters) == ["self", "paths_local", "max_rounds", "seed", "list_cap"]
    assert list(inspect.signature(MultiRobotSampler.plan_round).parameters) == ["self", "paths_local", "seed"]
    assert list(inspect.signature(MultiRobotSampler.set_other_paths).parameters) == ["self", "paths_all"]
    assert list(inspect.signature(MultiRobotSampler._pick).parameters) == ["self", "trajs_normalized", "guide", "robot0", "n_robots",
                                                                           "paths_all", "collision_table"]
    assert list(inspect.signature(MultiRobotSampler._collision_table).parameters) == ["self", "paths_all"]
    sub = inspect.signature(MultiRobotSampler.plan_rounds_subset).parameters
    assert list(sub)[-2:] == ["replan", "independent_iters"] and sub["replan"].default == "all"
    # the default round's report still builds its own default table
    assert MultiRobotSampler._report_on_own_table(types.SimpleNamespace()) is False
