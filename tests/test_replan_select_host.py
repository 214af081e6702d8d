"""CPU: the selection of the robots a many-robot round re-plans (mmd_round_select; multi_agent.select_replan;
MultiRobotSampler.replan_round / plan_rounds_subset) -- the numpy model of the two rules (tests/replan_model.py) on hand cases and on the
round instances, its properties for every iteration count, the error paths decided before any launch, the signatures and the op's meta
shapes.  The GPU tests compare the kernels with this model word for word."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import replan_model as S
import round_model as M
from mmd_amd import _lib

H = 64
FAKE = 0x1000                                                # a non-NULL "device pointer": every call below returns before its launch
ITERS = (1, 3, 5, 8)


def _sel(paths, mode, iters=8, **kw):
    selected, perm, header = S.select(paths, mode, iters, **kw)
    return selected.tolist(), perm.tolist(), header.tolist()


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    cases = S.hand_cases()
    assert all(len(p) <= 8 for p in cases.values())
    # one pair, equal counts: the lower id
    assert _sel(cases["pair"], S.INDEPENDENT) == ([0, 1, 0, 0], [1, 0, 2, 3], [1, 0, 1, 0])
    assert _sel(cases["pair"], S.CONFLICTED) == ([0, 1, 1, 0], [1, 2, 0, 3], [2, 0, 2, 0])
    # a chain 1 - 2 - 3: the middle robot alone (twice the count of its neighbours); "conflicted" gives all three
    assert _sel(cases["chain"], S.INDEPENDENT, 1) == ([0, 0, 1, 0, 0], [2, 0, 1, 3, 4], [1, 0, 1, 2])     # the ends: undecided once
    assert _sel(cases["chain"], S.INDEPENDENT, 8) == ([0, 0, 1, 0, 0], [2, 0, 1, 3, 4], [1, 0, 1, 0])
    assert _sel(cases["chain"], S.CONFLICTED) == ([0, 1, 1, 1, 0], [1, 2, 3, 0, 4], [3, 0, 3, 0])
    # a triangle: one of three, the lowest id; the other two are still undecided after one iteration
    assert _sel(cases["triangle"], S.INDEPENDENT, 1) == ([0, 1, 0, 0, 0, 0], [1, 0, 2, 3, 4, 5], [1, 0, 1, 2])
    assert _sel(cases["triangle"], S.INDEPENDENT, 2) == ([0, 1, 0, 0, 0, 0], [1, 0, 2, 3, 4, 5], [1, 0, 1, 0])
    assert _sel(cases["triangle"], S.CONFLICTED)[0] == [0, 1, 0, 1, 1, 0]
    # a star: the centre
    assert _sel(cases["star"], S.INDEPENDENT) == ([0, 0, 0, 0, 0, 1, 0, 0], [5, 0, 1, 2, 3, 4, 6, 7], [1, 0, 1, 0])
    assert _sel(cases["star"], S.CONFLICTED) == ([1, 0, 1, 0, 0, 1, 1, 1], [0, 2, 5, 6, 7, 1, 3, 4], [5, 0, 5, 0])
    # conflicts only at t = 0 and only at t = 63 are conflicts
    p = cases["first_and_last_step"]
    t, a, b, _ = M.report(p)
    assert sorted(zip(t.tolist(), a.tolist(), b.tolist())) == [(0, 0, 4), (H - 1, 3, 5)]
    assert _sel(p, S.INDEPENDENT) == ([1, 0, 0, 1, 0, 0], [0, 3, 1, 2, 4, 5], [2, 0, 2, 0])
    assert _sel(p, S.CONFLICTED) == ([1, 0, 0, 1, 1, 1], [0, 3, 4, 5, 1, 2], [4, 0, 4, 0])
    # no conflict at all: nothing selected, the identity, a zero header
    for mode in (S.CONFLICTED, S.INDEPENDENT):
        assert _sel(cases["none"], mode) == ([0] * 8, list(range(8)), [0, 0, 0, 0])
    assert _sel(cases["two"], S.INDEPENDENT) == ([1, 0], [0, 1], [1, 0, 1, 0]) and _sel(cases["two"], S.CONFLICTED)[0] == [1, 1]
    # the header's shard words
    assert _sel(cases["star"], S.CONFLICTED, robot0=2, n_local=4)[2] == [5, 1, 2, 0]


# ---- model properties ------------------------------------------------------------------------------------------------------------------
def _properties(paths, iters):
    n = len(paths)
    rep = M.report(paths)
    counts, nb = S.counts_of(rep, n), S.neighbours_of(rep, n)
    selected, perm, header = S.select(paths, S.INDEPENDENT, iters, rep=rep)
    assert S.is_independent(selected, nb)
    assert selected.sum() > 0 and header[0] == selected.sum()                      # there is a conflict in every instance used here
    assert all(counts[r] > 0 for r in np.nonzero(selected)[0])
    assert sorted(perm.tolist()) == list(range(n))
    k = int(header[0])
    assert (np.diff(perm[:k]) > 0).all() and (np.diff(perm[k:]) > 0).all() and selected[perm[:k]].all() and not selected[perm[k:]].any()
    if iters == 1:                                                                 # the strict local maxima of the priority
        want = [int(counts[r] > 0 and all(S.beats(counts, r, j) for j in nb[r])) for r in range(n)]
        assert selected.tolist() == want
    return int(header[0]), int(header[3]), int((counts > 0).sum())


def test_model_properties_on_the_round_instances():
    a, b, b_next = M.instance_a()[2], M.instance_b(), M.instance_b_next()
    got = {name: [_properties(p, it) for it in ITERS] for name, p in (("A", a), ("B", b), ("B_next", b_next))}
    assert [g[0] for g in got["A"]] == [1, 1, 1, 1] and got["A"][0][2] == 6       # 1 of 6
    assert [g[:2] for g in got["B"]] == [(9, 37), (15, 4), (15, 0), (15, 0)] and got["B"][0][2] == 46
    assert S.select(b, S.INDEPENDENT, 4)[2].tolist() == [15, 0, 15, 0]            # nobody undecided from 4 on
    assert [g[0] for g in got["B_next"]][:3] == [9, 18, 19]
    # the fixed point is maximal: every conflicted robot is selected or has a selected neighbour
    rep = M.report(b)
    nb = S.neighbours_of(rep, 48)
    selected = S.select(b, S.INDEPENDENT, 8, rep=rep)[0]
    assert all(selected[r] or any(selected[j] for j in nb[r]) for r in np.nonzero(S.counts_of(rep, 48))[0])
    # the counts are the report's row sums, both robots of a pair: what mmd_path_conflicts_binned's robot_counts hold
    assert int(S.counts_of(rep, 48).sum()) == 2 * len(rep[0])


def test_lattice_crosses_the_partition_chunk():
    p = S.lattice()
    n = len(p)
    assert n == 306 and np.abs(p).max() < 1.0
    rep = M.report(p)
    t, a, b, _ = rep
    counts = S.counts_of(rep, n)
    conflicted = int((counts > 0).sum())
    assert ((a <= 255) & (b >= 256)).any()                                        # a record across the chunk border
    for it in ITERS:
        n_sel, _, _ = _properties(p, it)
        assert 0 < n_sel < conflicted < n
    selected = S.select(p, S.INDEPENDENT, 8, rep=rep)[0]
    assert selected[:256].any() and selected[256:].any()
    header = S.select(p, S.INDEPENDENT, 8, robot0=200, n_local=100, rep=rep)[2]
    assert header[1] == selected[:200].sum() > 0 and header[2] == selected[200:300].sum() > 0


# ---- the API surface -------------------------------------------------------------------------------------------------------------------
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


def test_abi_stays_9_and_exports_round_select():
    assert _lib.ABI_VERSION == 9 and _lib.load().mmd_abi_version() == 9
    assert "mmd_round_select" in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES["mmd_round_select"][1]) == 13
    assert hasattr(_lib.load(), "mmd_round_select")
    assert (_lib.REPLAN_CONFLICTED, _lib.REPLAN_INDEPENDENT) == (0, 1) == (S.CONFLICTED, S.INDEPENDENT)
    assert C.sizeof(_lib.ConsBins) == 56


def test_round_select_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()

    def call(bins="default", paths=FAKE, counts=FAKE, n_local=3, horizon=64, margin=0.105, mode=1, iters=8, state=FAKE, selected=FAKE,
             perm=FAKE, header=FAKE):
        bins = _bins() if isinstance(bins, str) else bins
        rc = lib.mmd_round_select(paths, C.byref(bins) if bins is not None else None, counts, n_local, horizon, margin, mode, iters, state,
                                  selected, perm, header, None)
        return rc, lib.mmd_last_error().decode()

    cases = [({k: None}, "NULL") for k in ("paths", "counts", "state", "selected", "perm", "header", "bins")] + [
        ({"mode": 2}, "mode"), ({"mode": -1}, "mode"), ({"iters": 0}, "iters"), ({"iters": -4}, "iters"), ({"horizon": 63}, "horizon"),
        ({"margin": 0.1201}, "margin"), ({"bins": _bins(radius=0.1)}, "margin"), ({"n_local": 0}, "robot range"),
        ({"n_local": 7}, "robot range"), ({"bins": _bins(robot0=8)}, "robot"), ({"bins": _bins(n_all=1, robot0=0)}, "robot"),
        ({"bins": _bins(cell_off_dev=None)}, "NULL"), ({"bins": _bins(nx=0)}, "grid"),
        ({"bins": _bins(inv_cell=(C.c_float * 2)(8.0, 7.5))}, "cells smaller")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc != 0 and text in err, (kw, rc, err)
        if text in ("mode", "iters", "horizon", "margin", "robot range"):
            assert "mmd_round_select" in err, (kw, err)
    # mode CONFLICTED ignores iters: nothing to refuse there (checked up to the table, which is refused next)
    rc, err = call(mode=0, iters=0, bins=_bins(nx=0))
    assert rc != 0 and "grid" in err


def test_sampler_surface():
    from mmd_amd import multi_agent as ma
    from mmd_amd.multi_robot import MultiRobotSampler, PlanResult
    rounds = inspect.signature(MultiRobotSampler.plan_rounds).parameters
    sub = inspect.signature(MultiRobotSampler.plan_rounds_subset).parameters
    # plan_rounds_subset is plan_rounds with the two new arguments behind its own; plan_rounds calls it with replan="all"
    assert [(k, sub[k].default) for k in list(sub)[:len(rounds)]] == [(k, rounds[k].default) for k in rounds]
    assert [(k, sub[k].default) for k in list(sub)[len(rounds):]] == [("replan", "all"), ("independent_iters", 8)]
    p = inspect.signature(MultiRobotSampler.replan_round).parameters
    assert [(k, p[k].default) for k in list(p)[1:]] == [("paths_all", inspect.Parameter.empty), ("selection", inspect.Parameter.empty),
                                                        ("seed", inspect.Parameter.empty), ("prev_trajs", None), ("n_noising_steps", 3),
                                                        ("n_denoising_steps", 3)]
    assert PlanResult.replanned_counts is None and PlanResult(1, 2, 3, 4, 5, 6, 7).replanned_counts is None
    q = inspect.signature(ma.select_replan).parameters
    assert [(k, q[k].default) for k in list(q)[3:6]] == [("mode", "conflicted"), ("iters", 8), ("n_local", None)]
    assert list(ma.ReplanSelection.__dataclass_fields__) == ["selected", "perm", "header"] and callable(ma.ReplanSelection.read_header)
    assert ma.REPLAN_MODES == {"conflicted": 0, "independent": 1}
    # the three refusals come before any device work: a sampler of two attributes is enough to meet them
    fake = types.SimpleNamespace(constraint_table="dense", inter_robot=True)
    with pytest.raises(ValueError, match="replan"):
        MultiRobotSampler.plan_rounds_subset(fake, replan="some")
    for mode in ("conflicted", "independent"):
        with pytest.raises(ValueError, match="inter_robot"):
            MultiRobotSampler.plan_rounds_subset(types.SimpleNamespace(constraint_table="dense", inter_robot=False), replan=mode)
        with pytest.raises(ValueError, match="repair"):
            MultiRobotSampler.plan_rounds_subset(fake, replan=mode, repair=True)
    # and so do select_replan's: an unknown mode, a table that does not list time step 0
    with pytest.raises(ValueError, match="mode"):
        ma.select_replan(None, None, None, mode="some")
    with pytest.raises(ValueError, match="time step 0"):
        ma.select_replan(None, types.SimpleNamespace(first_step=1), None)


def test_op_meta_shapes():
    import torch
    import mmd_amd.ops  # noqa: F401
    paths = torch.zeros(37, 64, 2, device="meta")
    counts = torch.zeros(37, dtype=torch.int32, device="meta")
    selected, perm, header = torch.ops.mmd_amd.round_select(paths, counts, 5, 3, 0.105, 1, 8)
    assert selected.shape == (37,) and perm.shape == (37,) and header.shape == (4,)
    assert selected.dtype == perm.dtype == header.dtype == torch.int32
