"""-m gpu: the fragments the ELL table builders share (csrc/cons_table_dev.h), at the smallest shapes where they can go wrong: the one
all-pairs kernel behind soft_constraints_from_paths and RoundConstraints.set_soft, and the "one group of S slots per robot" writer of the
all-pairs, the framed and the path-constraints builders.  The yardstick is the rule restated in numpy -- copies of the paths' words and
the one float32 product r * |r| -- and, for the columns t >= 1, the host pack (mmd_pack_constraints) of the per-robot point lists.  No
tolerances: every comparison is of int32 words."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases                                                                      # noqa: E402
import gpu_common                                                                 # noqa: E402
from cases import H                                                               # noqa: E402
from mmd_amd import multi_agent as ma                                             # noqa: E402
from mmd_amd.constraints import (RoundConstraints, framed_constraints_from_paths, pack_constraints,   # noqa: E402
                                 soft_constraints_from_paths)

RADIUS, WEIGHT = cases.RADIUS_SOFT, 2e-2
# (n_all, robot0, n_local): one slot; one local robot; the skip rule at the last robot; more than four local robots; a shard in the middle
SHAPES = [(2, 0, 2), (2, 1, 1), (5, 4, 1), (5, 0, 5), (7, 2, 3)]
SENTINEL = 0x7FC0BEEF                                                             # (a NaN no builder writes)

_PATHS = {}


def _paths(n_all):
    """seeded float32 paths [n_all, H, 2] in [-1, 1], made once per size and never written"""
    if n_all not in _PATHS:
        p = np.random.default_rng(100 + n_all).uniform(-1.0, 1.0, (n_all, H, 2)).astype(np.float32)
        p.setflags(write=False)
        _PATHS[n_all] = p
    return _PATHS[n_all]


def _words(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _restated(paths, robot0, n_local, radius):
    """float32 [n_local, n_all - 1, H, 4]: slot j of local robot i = the j-th other robot, (x, y, r, r |r|) with r = radius at t >= 1, -1 at 0"""
    n_all = paths.shape[0]
    out = np.empty((n_local, n_all - 1, H, 4), dtype=np.float32)
    r = np.where(np.arange(H) >= 1, np.float32(radius), np.float32(-1.0)).astype(np.float32)
    for i in range(n_local):
        for j in range(n_all - 1):
            other = j + (1 if j >= robot0 + i else 0)
            out[i, j, :, :2] = paths[other]
            out[i, j, :, 2] = r
            out[i, j, :, 3] = r * np.abs(r)
    return out


@pytest.mark.parametrize("n_all,robot0,n_local", SHAPES)
def test_all_pairs_table(n_all, robot0, n_local):
    paths = _paths(n_all)
    ell, gso, gw, rgo, radius = soft_constraints_from_paths(torch.from_numpy(np.array(paths)).cuda(), robot0, n_local, RADIUS, WEIGHT)
    slots = n_all - 1
    assert radius == float(RADIUS) and ell.shape == (n_local * slots, H, 4)
    want = _restated(paths, robot0, n_local, RADIUS)
    got = _words(ell).reshape(n_local, slots, H, 4)
    assert np.array_equal(got, want.view(np.int32))
    assert gso.dtype == torch.int32 and gso.cpu().tolist() == [i * slots for i in range(n_local + 1)]
    assert rgo.dtype == torch.int32 and rgo.cpu().tolist() == list(range(n_local + 1))
    assert np.array_equal(_words(gw), np.full(n_local, WEIGHT, dtype=np.float32).view(np.int32))
    # columns t >= 1 are the host pack of the per-robot point lists (column 0: the pack leaves the empty word, the device the point with R = -1)
    groups = [[gpu_common.to_cost_constraint(cases.soft_group(np.array(paths), robot0 + i, WEIGHT))] for i in range(n_local)]
    p_ell, p_gso, p_gw, p_rgo = pack_constraints(groups, "cuda")
    assert np.array_equal(got[:, :, 1:], _words(p_ell).reshape(n_local, slots, H, 4)[:, :, 1:])
    assert torch.equal(p_gso, gso) and torch.equal(p_rgo, rgo) and np.array_equal(_words(p_gw), _words(gw))


@pytest.mark.parametrize("hard_slots", [1, 3])
@pytest.mark.parametrize("n_all,robot0,n_local", SHAPES)
def test_round_table_soft_block(n_all, robot0, n_local, hard_slots):
    paths = _paths(n_all)
    rc = RoundConstraints(n_all, robot0, n_local, hard_slots, radius=RADIUS, w_hard=2e-1, w_soft=WEIGHT)
    before = [_words(t).copy() for t in (rc.gso, rc.gw, rc.rgo, rc.fill, rc.dropped)]
    rc.ell.view(torch.int32).fill_(SENTINEL)
    rc.set_soft(torch.from_numpy(np.array(paths)).cuda())
    S = hard_slots + n_all - 1
    got = _words(rc.ell).reshape(n_local, S, H, 4)
    assert np.array_equal(got[:, hard_slots:], _restated(paths, robot0, n_local, RADIUS).view(np.int32))
    assert (got[:, :hard_slots] == np.int32(SENTINEL)).all()
    after = [_words(t) for t in (rc.gso, rc.gw, rc.rgo, rc.fill, rc.dropped)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("n_all,robot0,n_local", [(5, 0, 5), (7, 2, 3)])
def test_one_group_per_robot(n_all, robot0, n_local):
    slots = 2
    paths = torch.from_numpy(np.array(_paths(n_all))).cuda()
    _, s_gso, s_gw, s_rgo, _ = soft_constraints_from_paths(paths, robot0, n_local, RADIUS, WEIGHT)
    out = framed_constraints_from_paths(paths, torch.zeros((n_all, 2), device="cuda"), robot0, n_local, slots, RADIUS, WEIGHT)
    f_gso, f_gw, f_rgo = out[1], out[2], out[3]
    # the same arrays up to the slot count: i * slots against i * (n_all - 1)
    assert f_gso.dtype == torch.int32 and f_gso.cpu().tolist() == [i * slots for i in range(n_local + 1)]
    assert np.array_equal(_words(f_gso) * (n_all - 1), _words(s_gso) * slots)
    assert np.array_equal(_words(f_gw), _words(s_gw)) and torch.equal(f_rgo, s_rgo)
    # one robot, one group: mmd_path_constraints
    batches = [torch.cat((paths[k:k + 1], torch.zeros((1, H, 2), device="cuda")), -1).contiguous() for k in range(n_all)]
    _, gso, gw, rgo = ma.PathConstraints(batches, [0] * n_all, robot0, radius=RADIUS).build(WEIGHT, n_slots=slots)
    assert gso.dtype == torch.int32 and gso.cpu().tolist() == [0, slots]
    assert rgo.dtype == torch.int32 and rgo.cpu().tolist() == [0, 1]
    assert np.array_equal(_words(gw), np.float32([WEIGHT]).view(np.int32))
