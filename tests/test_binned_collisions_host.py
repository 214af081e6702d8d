"""CPU: the host side of the collision kernels on a cell table (mmd_bin_paths, mmd_count_collisions_binned, mmd_path_conflicts_binned;
MultiRobotSampler.plan) -- the signatures, the error paths decided before any launch, and the cover property the kernels rest on.

Cover property: a point p collides with a table point q iff sqrt(fma(dy, dy, dx * dx)) < margin in fp32 (rr_hit, csrc/collision_dev.h),
and p's lane reads only the list of its own cell, which holds the points of the 3 x 3 cells around it.  So every colliding pair must have
cell indices at most 1 apart on both axes whenever margin <= the table's radius (the entry points refuse a larger margin).  Checked here
at the robot-robot margin and at the extreme the entry points admit, margin == radius."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import fp32_forms as F
from mmd_amd import _lib
from mmd_amd import constraints as K
from test_binned_host import R, cell_index, planted_pairs

FAKE = 0x1000                                                # a non-NULL "device pointer": every call below returns before its launch


def _bins(**kw):
    b = _lib.ConsBins()
    b.lo[:] = [-1.0, -1.0]
    b.inv_cell[:] = [7.5, 7.5]
    b.nx, b.ny, b.n_all, b.robot0 = 15, 15, 8, 2
    b.radius, b.weight = 0.12, 0.0
    b.cell_off_dev, b.entries_dev = FAKE, FAKE               # never read on the host
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_abi_has_the_three_entry_points_and_stays_9():
    assert _lib.ABI_VERSION == 9
    for name in ("mmd_bin_paths", "mmd_count_collisions_binned", "mmd_path_conflicts_binned"):
        assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.mmd_abi_version() == 9
    assert len(_lib._SIGNATURES["mmd_bin_paths"][1]) == 12
    assert len(_lib._SIGNATURES["mmd_count_collisions_binned"][1]) == 7
    assert len(_lib._SIGNATURES["mmd_path_conflicts_binned"][1]) == 11
    assert C.sizeof(_lib.ConsBins) == 56                      # the struct keeps its layout


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    lo, hi = (C.c_float * 2)(-1, -1), (C.c_float * 2)(1, 1)
    good = dict(paths=FAKE, n_all=5, horizon=64, reach=0.12, lo=lo, hi=hi, nx=15, ny=15, first=0, off=FAKE, ent=FAKE)

    def bin_paths(**kw):
        a = dict(good, **kw)
        rc = lib.mmd_bin_paths(a["paths"], a["n_all"], a["horizon"], a["reach"], a["lo"], a["hi"], a["nx"], a["ny"], a["first"], a["off"],
                               a["ent"], None)
        return rc, lib.mmd_last_error().decode()

    for kw, text in (({"first": 2}, "first_step"), ({"first": -1}, "first_step"), ({"first": 64}, "first_step"), ({"paths": None}, "NULL"),
                     ({"off": None}, "NULL"), ({"ent": None}, "NULL"), ({"hi": None}, "NULL"), ({"n_all": 1}, "n_all"),
                     ({"reach": 0.0}, "radius"), ({"nx": 16}, "cells smaller"), ({"reach": 0.126}, "cells smaller"), ({"ny": 0}, "grid"),
                     ({"horizon": 63}, "horizon")):
        rc, err = bin_paths(**kw)
        assert rc != 0 and text in err and "mmd_bin_paths" in err, (kw, rc, err)

    def count(bins, trajs=FAKE, n_local=3, spr=4, margin=0.105, counts=FAKE):
        rc = lib.mmd_count_collisions_binned(trajs, C.byref(bins) if bins is not None else None, n_local, spr, margin, counts, None)
        return rc, lib.mmd_last_error().decode()

    def conflicts(bins, paths=FAKE, horizon=64, margin=0.105, rows=FAKE, robots=None, cnt=FAKE, first=None, lst=None, cap=0):
        rc = lib.mmd_path_conflicts_binned(paths, C.byref(bins) if bins is not None else None, horizon, margin, rows, robots, cnt, first,
                                           lst, cap, None)
        return rc, lib.mmd_last_error().decode()

    table_faults = ((None, "NULL"), (_bins(cell_off_dev=None), "NULL"), (_bins(entries_dev=None), "NULL"), (_bins(robot0=8), "robot"),
                    (_bins(n_all=1, robot0=0), "robot"), (_bins(nx=0), "grid"), (_bins(ny=65), "grid"), (_bins(radius=0.0), "radius"),
                    (_bins(inv_cell=(C.c_float * 2)(8.0, 7.5)), "cells smaller"))
    for call in (count, conflicts):
        for bins, text in table_faults:
            rc, err = call(bins)
            assert rc != 0 and text in err, (call.__name__, text, rc, err)
        rc, err = call(_bins(), margin=0.1201)                                    # above the table's radius: a list could miss a hit
        assert rc != 0 and "margin" in err, (rc, err)
        rc, err = call(_bins(radius=0.1), margin=0.105)
        assert rc != 0 and "margin" in err, (rc, err)
    for kw, text in (({"trajs": None}, "NULL"), ({"counts": None}, "NULL"), ({"n_local": 0}, "robot range"), ({"n_local": 7}, "robot range"),
                     ({"spr": 0}, "robot range")):
        rc, err = count(_bins(), **kw)
        assert rc != 0 and text in err, (kw, rc, err)
    for kw, text in (({"paths": None}, "NULL"), ({"rows": None}, "NULL"), ({"cnt": None}, "NULL"), ({"horizon": 32}, "horizon"),
                     ({"cap": 4}, "list_cap"), ({"cap": -1}, "list_cap")):
        rc, err = conflicts(_bins(), **kw)
        assert rc != 0 and text in err, (kw, rc, err)


def test_guide_refuses_a_collision_table_and_the_python_layer_records_first_step():
    import torch
    from mmd_amd.guides import GuideManagerTrajectoriesWithVelocity as G
    from mmd_amd.environments import LIMITS
    from mmd_amd import multi_agent as MA
    off, ent = torch.zeros((64, 226), dtype=torch.int32), torch.zeros((64, 45, 4))
    tabs = {f: K.BinnedConstraints(off, ent, LIMITS, (15, 15), 5, 0, 2, 0.12, 2e-2, first_step=f) for f in (0, 1)}
    assert K.BinnedConstraints(off, ent, LIMITS, (15, 15), 5, 0, 2, 0.12, 2e-2).first_step == 1      # the default: a constraint table
    guide = types.SimpleNamespace(n_robots=2, _binned=None)
    G.set_binned_constraints(guide, tabs[1])
    assert guide._binned is tabs[1]
    with pytest.raises(ValueError, match="time step"):
        G.set_binned_constraints(guide, tabs[0])
    assert guide._binned is tabs[1]
    # and the collision calls refuse a constraint table (it has no lists at t = 0, where collisions count)
    with pytest.raises(ValueError, match="time step 0"):
        MA.count_collisions_binned(torch.zeros(8, 64, 4), tabs[1], 2)
    with pytest.raises(ValueError, match="time step 0"):
        MA.path_conflicts(torch.zeros(5, 64, 2), table=tabs[1])
    summ, robots, lst = MA.path_conflicts(torch.zeros(1, 64, 2))                   # one robot: no table, no launch, nothing collides
    assert MA.read_summary(summ) == (0, None) and summ[4:7].tolist() == [-1, -1, -1] and robots.tolist() == [0] and lst is None
    for fn in (K.bin_constraints_table, K.binned_constraints_from_paths):
        assert inspect.signature(fn).parameters["first_step"].default == 1
    p = inspect.signature(K.binned_collision_table).parameters
    assert p["reach"].default == K.VERTEX_CONSTRAINT_RADIUS and K.bin_grid(LIMITS, p["reach"].default) == (15, 15)
    with pytest.raises(ValueError, match="first_step"):
        K.binned_constraints_from_paths(torch.zeros(5, 64, 2), 0, 5, first_step=2)


def test_sampler_has_plan_and_plan_round_is_unchanged():
    import torch
    import mmd_amd.ops  # noqa: F401
    from mmd_amd.multi_robot import MultiRobotSampler, PlanResult
    sig = inspect.signature(MultiRobotSampler.plan_round)
    assert list(sig.parameters) == ["self", "paths_local", "seed"] and sig.parameters["seed"].default is None
    p = inspect.signature(MultiRobotSampler.plan).parameters
    assert [(k, p[k].default) for k in list(p)[1:]] == [("paths_local", None), ("max_rounds", 8), ("seed", 0), ("list_cap", 0)]
    assert inspect.signature(MultiRobotSampler.__init__).parameters["constraint_table"].default == "dense"
    assert {"paths_local", "trajs", "n_rounds", "conflict_counts", "robot_counts", "conflict_free", "first_conflict"} <= \
        set(PlanResult.__dataclass_fields__)
    counts = torch.ops.mmd_amd.count_collisions_binned(torch.zeros(21, 64, 4, device="meta"), torch.zeros(37, 64, 2, device="meta"), 5, 3, 0.105)
    assert counts.shape == (3, 7) and counts.dtype == torch.int32
    summ, robots, lst = torch.ops.mmd_amd.path_conflicts(torch.zeros(37, 64, 2, device="meta"), 0.105, 10)
    assert summ.shape == (16,) and robots.shape == (37,) and lst.shape == (10, 12) and lst.dtype == torch.int32


def _hit(p, q, margin):
    return F.pos_norm(p, q) < np.float32(margin)


@pytest.mark.parametrize("margin", [F.MARGIN, R], ids=["rr_margin", "margin_eq_radius"])
def test_colliding_pairs_are_in_neighbouring_cells(margin):
    """every pair the collision test accepts has q in the list of p's own cell: the count over that list is the brute-force count"""
    pp, pq = planted_pairs()                                                      # at R (1 +- a few ulp): the margin == radius extreme
    mp, mq = F.margin_pairs(31, 20_000, margin=margin)                            # |p - q| = margin (1 +- 4e-7): both sides of the test
    rng = np.random.default_rng(32)
    c = rng.uniform(-1.4, 1.4, (50_000, 2))
    phi = rng.uniform(0, 2 * np.pi, 50_000)
    d = np.stack([np.cos(phi), np.sin(phi)], 1) * (float(margin) * rng.uniform(0.0, 1.2, 50_000))[:, None]
    rp, rq = (c + d / 2).astype(np.float32), (c - d / 2).astype(np.float32)
    for name, a, b in (("planted", pp, pq), ("margin", mp, mq), ("random", rp, rq)):
        hit = _hit(a, b, margin)
        in_list = (np.abs(cell_index(a) - cell_index(b)) <= 1).all(1)
        if name != "planted" or margin == R:
            assert hit.sum() > len(a) // 10 and (~hit).sum() > len(a) // 20, (name, int(hit.sum()))     # the cases sit on both sides
        assert int((hit & in_list).sum()) == int(hit.sum()), (name, a[hit & ~in_list][:4], b[hit & ~in_list][:4])
    # not vacuous: with cells narrower than the margin, colliding pairs do skip a cell
    ca, cb = cell_index(rp, grid=(32, 32)), cell_index(rq, grid=(32, 32))
    assert np.abs(ca - cb)[_hit(rp, rq, margin)].max() >= 2


def test_numpy_model_of_the_own_cell_walk_has_the_brute_force_counts():
    """one time step of count_collisions_binned_kernel in numpy fp32: per sample point, the hits among the robots of its own cell's list
    (the robot itself skipped by id) against the hits among all robots"""
    rng = np.random.default_rng(33)
    n, lanes = 48, 6000
    q = rng.uniform(-1.1, 1.1, (n, 2)).astype(np.float32)
    q[7] = q[8]                                                                    # coincident robots
    q[20], q[21] = (1.3, -1.2), (-1.0, 1.0)                                        # outside the limits, a corner
    anchor = rng.integers(0, n, lanes)
    p = F.near_points(rng, q[anchor], float(F.MARGIN))                             # within a few ulp of the margin, both sides
    p[:200] = F.near_points(rng, q[anchor[:200]], float(F.MARGIN) * rng.uniform(0, 2, 200), rel=0.0)
    cq, cp = cell_index(q), cell_index(p)
    for self_id in (0, 7, 47):
        brute = np.zeros(lanes, np.int64)
        walked = np.zeros(lanes, np.int64)
        for rid in range(n):
            if rid == self_id:
                continue
            hit = _hit(p, q[rid], F.MARGIN)
            brute += hit
            walked += hit & (np.abs(cq[rid] - cp) <= 1).all(1)
        assert np.array_equal(walked, brute), self_id
        assert brute.max() >= 2 and (brute == 0).sum() > 0 and (brute > 0).sum() > lanes // 4
