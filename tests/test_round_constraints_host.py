"""CPU: the host side of the round table (mmd_round_constraints_init, mmd_round_soft_from_paths, mmd_conflict_constraints_append;
constraints.RoundConstraints; MultiRobotSampler.plan_rounds(repair=, local_rounds=)) -- the numpy model of the hard block's slot rule pinned to
mmd_pack_constraints word for word, the error paths decided before any launch, the signatures and the ops' meta shapes."""
import ctypes as C
import inspect

import numpy as np
import pytest

import round_model as M
from mmd_amd import _lib

H = 64
FAKE = 0x1000                                                # a non-NULL "device pointer": every call below returns before its launch


def _pack_one_group(tc, mid, t_pad, radius=M.RADIUS):
    """mmd_pack_constraints on ONE group: the points (mid, range (tc - t_pad, tc + t_pad), radius) in the order given -> ell [slots, H, 4]"""
    lib = _lib.load()
    n = len(tc)
    q = np.ascontiguousarray(mid, np.float32).reshape(n, 2)
    tr = np.stack([np.asarray(tc) - t_pad, np.asarray(tc) + t_pad], 1).astype(np.float32)
    rad = np.full(n, radius, np.float32)
    n_pts = (C.c_int32 * 1)(n)
    ptrs = [(C.c_void_p * 1)(a.ctypes.data) for a in (q, tr, rad)]
    slots = (C.c_int32 * 1)()
    _lib.check(lib.mmd_pack_constraints(1, n_pts, ptrs[0], ptrs[1], ptrs[2], H, None, 0, slots))
    ell = np.zeros((max(slots[0], 1), H, 4), np.float32)
    _lib.check(lib.mmd_pack_constraints(1, n_pts, ptrs[0], ptrs[1], ptrs[2], H, ell.ctypes.data, max(slots[0], 1), slots))
    return ell[:slots[0]], int(slots[0])


def _record_list(rng, n, edge_heavy):
    """a robot's records of one round as the report orders them: tc ascending, several partners per tc (repeated pairs: the same
    partner, hence nearly the same midpoint, at successive tc); tc in {0, 1, H - 2, H - 1} always present when edge_heavy"""
    tc = np.sort(rng.integers(0, H, n))
    if edge_heavy:
        tc = np.sort(np.concatenate([tc, [0, 0, 1, H - 2, H - 1, H - 1, H - 1]]))
    base = rng.uniform(-1, 1, (5, 2))                                             # five partners' meeting points
    who = rng.integers(0, 5, len(tc))
    mid = (base[who] + 0.01 * tc[:, None] / H).astype(np.float32)
    return tc, mid


@pytest.mark.parametrize("t_pad", [2, 1, 3])
def test_slot_model_is_pack_constraints_word_for_word(t_pad):
    rng = np.random.default_rng(700 + t_pad)
    seen_edges = set()
    for case in range(40):
        rounds = [_record_list(rng, int(rng.integers(0, 60)), case % 2 == 0) for _ in range(1 + case % 3)]     # 1-3 concatenated rounds
        tc = np.concatenate([r[0] for r in rounds])
        mid = np.concatenate([r[1] for r in rounds])
        seen_edges |= set(tc.tolist()) & {0, 1, H - 2, H - 1}
        want, slots = _pack_one_group(tc, mid, t_pad)
        if slots == 0:
            assert len(tc) == 0
            continue
        blk = M.HardBlock(slots)
        for r in rounds:                                                          # round after round: the state persists
            blk.append(*r, t_pad=t_pad)
        assert blk.dropped == 0 and int(blk.fill.max()) == slots
        assert np.array_equal(blk.ell.view(np.int32), want.view(np.int32)), case
        assert np.array_equal(blk.fill, (want[..., 2] >= 0).sum(0)), case
        # the cap: the first cap slots of the same pack, the rest counted
        for cap in {1, max(slots - 1, 1)}:
            cut = M.HardBlock(cap)
            for r in rounds:
                cut.append(*r, t_pad=t_pad)
            assert np.array_equal(cut.ell.view(np.int32), want[:cap].view(np.int32)), (case, cap)
            assert np.array_equal(cut.fill, np.minimum(blk.fill, cap))
            assert cut.dropped == int(np.maximum(blk.fill - cap, 0).sum())
    assert seen_edges == {0, 1, H - 2, H - 1}


def test_report_model_orders_a_robots_records_by_time_then_partner():
    """what the kernel's walk relies on: in the (t, a, b), a < b row-major report, the records naming robot r are in ascending
    (t, other robot) order, and the midpoint does not depend on which of the two is named first"""
    p = M.instance_b()
    rep = M.report(p)
    t, a, b, mid = rep
    assert len(t) > 200
    for r in (0, 7, 8, 20, 21, 47):
        m = (a == r) | (b == r)
        other = np.where(a[m] == r, b[m], a[m])
        key = t[m] * 1000 + other
        assert (np.diff(key) > 0).all(), r
        assert np.array_equal(((p[r, t[m]] + p[other, t[m]]) / np.float32(2)).view(np.int32), mid[m].view(np.int32))
    assert M.max_fill([rep], 48) >= 4 and M.max_fill([M.report(M.instance_a()[2])], 6) >= 4


def _bins(**kw):
    b = _lib.ConsBins()
    b.lo[:] = [-1.0, -1.0]
    b.inv_cell[:] = [7.5, 7.5]
    b.nx, b.ny, b.n_all, b.robot0 = 15, 15, 8, 2
    b.radius, b.weight = 0.12, 0.0
    b.cell_off_dev, b.entries_dev = FAKE, FAKE
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_abi_stays_9_and_has_the_entry_points():
    assert _lib.ABI_VERSION == 9 and _lib.load().mmd_abi_version() == 9
    for name, n_args in (("mmd_round_constraints_init", 13), ("mmd_round_soft_from_paths", 9), ("mmd_conflict_constraints_append", 12)):
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == n_args
    assert C.sizeof(_lib.ConsBins) == 56 and C.sizeof(_lib.Conflict) == 48


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()

    def init(n_all=8, n_local=3, horizon=64, hs=4, ell=FAKE, gso=FAKE, gw=FAKE, rgo=FAKE, fill=FAKE, dropped=FAKE):
        rc = lib.mmd_round_constraints_init(n_all, n_local, horizon, hs, 0.2, 0.02, ell, gso, gw, rgo, fill, dropped, None)
        return rc, lib.mmd_last_error().decode()

    def soft(paths=FAKE, n_all=8, robot0=2, n_local=3, horizon=64, hs=4, ell=FAKE):
        rc = lib.mmd_round_soft_from_paths(paths, n_all, robot0, n_local, horizon, hs, 0.12, ell, None)
        return rc, lib.mmd_last_error().decode()

    def append(bins="default", paths=FAKE, n_local=3, horizon=64, hs=4, t_pad=2, margin=0.105, ell=FAKE, fill=FAKE, dropped=FAKE):
        bins = _bins() if isinstance(bins, str) else bins
        rc = lib.mmd_conflict_constraints_append(paths, C.byref(bins) if bins is not None else None, n_local, horizon, hs, t_pad, margin,
                                                 0.12, ell, fill, dropped, None)
        return rc, lib.mmd_last_error().decode()

    for call, name, cases in (
        (init, "mmd_round_constraints_init",
         [({k: None}, "NULL") for k in ("ell", "gso", "gw", "rgo", "fill", "dropped")] +
         [({"horizon": 63}, "horizon"), ({"hs": 0}, "hard_slots"), ({"hs": -3}, "hard_slots"), ({"n_local": 0}, "robot range"),
          ({"n_local": 9}, "robot range"), ({"n_all": 1, "n_local": 1}, "robot range")]),
        (soft, "mmd_round_soft_from_paths",
         [({"paths": None}, "NULL"), ({"ell": None}, "NULL"), ({"horizon": 32}, "horizon"), ({"hs": 0}, "hard_slots"),
          ({"robot0": -1}, "robot range"), ({"robot0": 6}, "robot range"), ({"robot0": 8}, "robot range"), ({"n_local": 0}, "robot range"),
          ({"n_all": 1, "robot0": 0, "n_local": 1}, "robot range")]),
        (append, "mmd_conflict_constraints_append",
         [({k: None}, "NULL") for k in ("paths", "ell", "fill", "dropped", "bins")] +
         [({"horizon": 65}, "horizon"), ({"hs": 0}, "hard_slots"), ({"t_pad": 0}, "t_pad"), ({"t_pad": -2}, "t_pad"),
          ({"margin": 0.1201}, "margin"), ({"bins": _bins(radius=0.1)}, "margin"), ({"n_local": 0}, "robot range"),
          ({"n_local": 7}, "robot range"), ({"bins": _bins(robot0=8)}, "robot"), ({"bins": _bins(n_all=1, robot0=0)}, "robot"),
          ({"bins": _bins(cell_off_dev=None)}, "NULL"), ({"bins": _bins(entries_dev=None)}, "NULL"), ({"bins": _bins(nx=0)}, "grid"),
          ({"bins": _bins(radius=0.0)}, "radius"), ({"bins": _bins(inv_cell=(C.c_float * 2)(8.0, 7.5))}, "cells smaller")])):
        for kw, text in cases:
            rc, err = call(**kw)
            assert rc != 0 and text in err, (name, kw, rc, err)
            if text not in ("NULL", "grid", "radius", "cells smaller", "robot"):
                assert name in err, (name, kw, err)
    # a table too large for the guided step's int index
    rc, err = init(n_all=4096, n_local=4096, hs=1 << 20)                        # 4096 x (2^20 + 4095) x 64 points
    assert rc != 0 and "2^31" in err


def test_plan_rounds_has_the_new_parameters_and_refuses_repair_next_to_a_cell_table():
    """plan() keeps its four parameters; plan_rounds is the same loop and carries the opt-in ones behind them"""
    import types
    from mmd_amd.multi_robot import MultiRobotSampler, PlanResult
    p = inspect.signature(MultiRobotSampler.plan_rounds).parameters
    assert [(k, p[k].default) for k in list(p)[1:]] == [
        ("paths_local", None), ("max_rounds", 8), ("seed", 0), ("list_cap", 0), ("repair", False), ("hard_slots", 32),
        ("weight_grad_cost_constraints", 2e-1), ("t_pad", 2), ("local_rounds", False), ("n_noising_steps", 3), ("n_denoising_steps", 3)]
    q = inspect.signature(MultiRobotSampler.plan).parameters
    assert [(k, q[k].default) for k in q] == [(k, p[k].default) for k in list(p)[:5]]
    seen = []
    fake = types.SimpleNamespace(plan_rounds=lambda *a: seen.append(a) or "result")                 # plan() is plan_rounds with both off
    assert MultiRobotSampler.plan(fake, "paths", 3, 7, 5) == "result" and seen == [("paths", 3, 7, 5)]
    sig = inspect.signature(MultiRobotSampler.plan_round)
    assert list(sig.parameters) == ["self", "paths_local", "seed"]
    assert inspect.signature(MultiRobotSampler.best_paths).parameters["collision_table"].default is None
    # a new trailing field with a default: the old positional construction still works
    f = list(PlanResult.__dataclass_fields__)
    assert f[-1] == "dropped_constraints" and f[:7] == ["paths_local", "trajs", "n_rounds", "conflict_counts", "robot_counts", "conflict_free",
                                                        "first_conflict"]
    assert PlanResult(1, 2, 3, 4, 5, 6, 7).dropped_constraints is None
    # refused before anything is launched or gathered
    for kw in ({"constraint_table": "binned", "inter_robot": True}, {"constraint_table": "dense", "inter_robot": False}):
        fake = types.SimpleNamespace(**kw)
        with pytest.raises(ValueError, match="repair"):
            MultiRobotSampler.plan_rounds(fake, repair=True)


def test_round_constraints_class_and_q_sample_index_base():
    from mmd_amd import constraints as K
    from mmd_amd.diffusion_model import GaussianDiffusionModel
    from mmd_amd.multi_agent import RR_MARGIN
    for name in ("reset", "set_soft", "append_conflicts", "tensors"):
        assert callable(getattr(K.RoundConstraints, name))
    p = inspect.signature(K.RoundConstraints.append_conflicts).parameters
    assert p["margin"].default == RR_MARGIN and p["t_pad"].default == 2
    p = inspect.signature(K.RoundConstraints.__init__).parameters
    assert p["hard_slots"].default == 32 and p["w_hard"].default == 2e-1 and p["w_soft"].default == 2e-2
    for bad in (dict(n_all=1, robot0=0, n_local=1), dict(n_all=8, robot0=6, n_local=3), dict(n_all=8, robot0=0, n_local=8, hard_slots=0)):
        with pytest.raises(ValueError):
            K.RoundConstraints(device="cpu", **bad)
    # run_local_inference hands traj_index_base to q_sample (a sharded rank draws its own rows' noise), 0 by default
    seen = []

    class Probe:
        def q_sample(self, x, t, noise=None, traj_index_base=0, seed=None):
            seen.append((t, traj_index_base, seed))
            return x

        def conditional_sample(self, hard_conds, **kw):
            import torch
            return None, torch.zeros(1, 2, 3, 4)

    run = GaussianDiffusionModel.run_local_inference.__wrapped__ if hasattr(GaussianDiffusionModel.run_local_inference, "__wrapped__") \
        else GaussianDiffusionModel.run_local_inference
    run(Probe(), "x", 3, 3, hard_conds={}, seed=5, traj_index_base=64)
    run(Probe(), "x", 3, 3, hard_conds={}, seed=6)
    assert seen == [(3, 64, 5), (3, 0, 6)]


def test_op_meta_shapes():
    import torch
    import mmd_amd.ops  # noqa: F401
    like = torch.zeros(1, device="meta")
    ell, gso, gw, rgo, fill, dropped = torch.ops.mmd_amd.round_constraints_init(like, 37, 3, 5, 0.2, 0.02)
    assert ell.shape == (3 * (5 + 36), 64, 4) and ell.dtype == torch.float32
    assert gso.shape == (7,) and gso.dtype == torch.int32 and gw.shape == (6,) and gw.dtype == torch.float32
    assert rgo.shape == (4,) and rgo.dtype == torch.int32
    assert fill.shape == (3, 64) and fill.dtype == torch.int32 and dropped.shape == (3,) and dropped.dtype == torch.int32
    paths = torch.zeros(37, 64, 2, device="meta")
    assert torch.ops.mmd_amd.round_soft_from_paths(ell, paths, 5, 3, 5, 0.12) is None
    assert torch.ops.mmd_amd.conflict_constraints_append(ell, fill, dropped, paths, 5, 3, 5, 2, 0.105, 0.12) is None
