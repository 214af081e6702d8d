"""-m gpu: the selection of the robots a round re-plans (mmd_round_select through multi_agent.select_replan and
torch.ops.mmd_amd.round_select) against the numpy model of tests/replan_model.py, word for word: selected, perm and header, both modes, the
hand cases, the round instances, the 306-robot lattice that crosses the partition kernel's chunk, shards, and the smallest table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import multi_agent as ma                                            # noqa: E402
from mmd_amd.constraints import binned_collision_table                           # noqa: E402
import replan_model as S                                                         # noqa: E402
import round_model as M                                                          # noqa: E402

_CACHE = {}


def _instance(name):
    """(paths [N, H, 2] float32, its report), computed once and left unchanged"""
    if name not in _CACHE:
        hand = S.hand_cases()
        if name in hand:
            p = hand[name]
        else:
            p = {"A": lambda: M.instance_a()[2], "B": lambda: M.instance_b(meet_outside=True), "lattice": S.lattice}[name]()
        p = np.ascontiguousarray(p, np.float32)
        p.setflags(write=False)
        _CACHE[name] = (p, M.report(p))
    return _CACHE[name]


def _device(p_np, mode, iters, robot0=0, n_local=None):
    """(ReplanSelection, robot_counts) of the device path on a shard"""
    paths = torch.from_numpy(np.array(p_np)).cuda()
    n_local = len(p_np) - robot0 if n_local is None else n_local
    table = binned_collision_table(paths, robot0, n_local)
    _, robots, _ = ma.path_conflicts(paths, table=table)
    return ma.select_replan(paths, table, robots, mode, iters), robots


def _assert_is_model(name, mode, iters, robot0=0, n_local=None):
    p, rep = _instance(name)
    sel, robots = _device(p, mode, iters, robot0, n_local)
    want = S.select(p, ma.REPLAN_MODES[mode], iters, robot0, n_local, rep=rep)
    assert np.array_equal(robots.cpu().numpy(), S.counts_of(rep, len(p))), name   # what the priorities are made of
    got = (sel.selected.cpu().numpy(), sel.perm.cpu().numpy(), sel.header.cpu().numpy())
    for what, g, w in zip(("selected", "perm", "header"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, mode, iters, robot0, what, g.tolist(), w.tolist())
    assert sel.read_header() == tuple(int(v) for v in want[2])
    return want


@pytest.mark.parametrize("name", ["pair", "chain", "triangle", "star", "first_and_last_step", "none", "two"])
def test_hand_cases_are_the_model(name):
    for iters in (1, 2, 8):
        _assert_is_model(name, "independent", iters)
    _assert_is_model(name, "conflicted", 8)
    if name == "none":
        sel, _ = _device(_instance(name)[0], "independent", 8)
        assert sel.perm.tolist() == list(range(8)) and sel.header.tolist() == [0, 0, 0, 0] and not sel.selected.any()
    if name == "pair":
        assert _device(_instance(name)[0], "independent", 8)[0].selected.tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("iters", [1, 3, 8])
@pytest.mark.parametrize("name,robot0,n_local", [("A", 0, 6), ("B", 0, 48), ("B", 16, 16), ("lattice", 0, 306), ("lattice", 200, 100)],
                         ids=["A", "B", "B_16_16", "lattice", "lattice_200_100"])
def test_instances_are_the_model(name, robot0, n_local, iters):
    selected, perm, header = _assert_is_model(name, "independent", iters, robot0, n_local)
    assert header[0] > 0
    if name == "B" and robot0 == 16:
        assert header[1] > 0 and header[2] > 0 and header[1] + header[2] < header[0]        # selected robots on all three sides
    if name == "lattice":
        assert selected[:256].any() and selected[256:].any()                                # both chunks of the partition
    if iters == 8:
        want = _assert_is_model(name, "conflicted", 8, robot0, n_local)
        assert want[2][3] == 0 and want[2][0] > header[0]
        # mode CONFLICTED ignores iters
        p, _ = _instance(name)
        assert torch.equal(_device(p, "conflicted", 0, robot0, n_local)[0].perm, _device(p, "conflicted", 8, robot0, n_local)[0].perm)


def test_the_selection_is_the_same_on_every_run_and_leaves_its_inputs():
    p, _ = _instance("B")
    paths = torch.from_numpy(np.array(p)).cuda()
    table = binned_collision_table(paths)
    _, robots, _ = ma.path_conflicts(paths, table=table)
    keep = (paths.clone(), robots.clone(), table.entries.clone(), table.cell_off.clone())
    runs = [ma.select_replan(paths, table, robots, "independent", 5) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r.selected, runs[0].selected) and torch.equal(r.perm, runs[0].perm) and torch.equal(r.header, runs[0].header)
    assert all(torch.equal(a, b) for a, b in zip(keep, (paths, robots, table.entries, table.cell_off)))
    header = runs[0].read_header()                                                # one copy: the first call's result is kept
    assert header == tuple(runs[1].header.tolist()) and header[0] == 15
    runs[0].header.zero_()
    assert runs[0].read_header() == header
    with pytest.raises(ValueError, match="time step 0"):
        from mmd_amd.constraints import binned_constraints_from_paths
        ma.select_replan(paths, binned_constraints_from_paths(paths, 0, 48), robots)
    with pytest.raises(RuntimeError, match="iters"):
        ma.select_replan(paths, table, robots, "independent", 0)


def test_torch_op_is_the_ctypes_path():
    import mmd_amd.ops  # noqa: F401
    p, _ = _instance("B")
    paths = torch.from_numpy(np.array(p)).cuda()
    for mode, iters, robot0, n_local in (("independent", 3, 16, 16), ("conflicted", 8, 0, 48)):
        sel, robots = _device(p, mode, iters, robot0, n_local)
        selected, perm, header = torch.ops.mmd_amd.round_select(paths, robots, robot0, n_local, ma.RR_MARGIN, ma.REPLAN_MODES[mode], iters)
        assert torch.equal(selected, sel.selected) and torch.equal(perm, sel.perm) and torch.equal(header, sel.header)
        assert int(header[0]) > 0
