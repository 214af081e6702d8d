"""Host checks of tests/round_pick_cases.py: on the model alone (tests/round_pick_model.py: the oracle, fp32_forms and float64), every family
of inputs reaches the edge it is built around, so that no test of tests/test_gpu_round_pick_edges.py can pass by missing it.  A ladder
counts only if both verdicts occur on it; at least 90 % of a family's ladders must count, and each verdict must make up at least 10 % of the
family's samples.  No GPU."""
import numpy as np
import pytest
import torch

import fp32_forms as F
import post_edge_cases as E
import round_pick_cases as K
import round_pick_model as M
from oracle import mmd_oracle as O

H = K.H


def _assert_reaches_its_edge(verdict, ladders, tag):
    counted, share = K.ladder_stats(verdict, ladders)
    assert counted >= 0.9, (tag, counted)
    assert 0.1 <= share <= 0.9, (tag, share)


def test_model_unnormalise_is_the_torch_form_with_the_clip_on_every_element():
    x = torch.tensor([[-1.5, -1.0, 0.0, float("nan")], [0.3, 1.0, 1.00005, 7.0]])
    mins, maxs = torch.from_numpy(K.WIDE_MIN), torch.from_numpy(K.WIDE_MAX)
    want = (torch.clip(x, -1, 1) + 1) / 2.0 * (maxs - mins) + mins
    got = M.unnormalise(x.numpy(), K.WIDE_MIN, K.WIDE_MAX)
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32)) and np.isnan(got[0, 3]) and got[1, 2] == 1.5 and got[0, 0] == -1.25
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(-1.1, 1.1, (4096, 4)).astype(np.float32))
    want = (torch.clip(x, -1, 1) + 1) / 2.0 * (maxs - mins) + mins
    assert np.array_equal(M.unnormalise(x.numpy(), K.WIDE_MIN, K.WIDE_MAX).view(np.int32), want.numpy().view(np.int32))


def test_a_ladder_in_ulps_of_v_plus_1_moves_the_value_and_one_in_ulps_of_v_does_not():
    lo, hi = K.NORM_MIN[0], K.NORM_MAX[0]
    v = K.ladder(1e-3, lo, hi)
    assert len(np.unique(M.unnormalise(v, [lo], [hi]))) == len(v)
    tiny = (np.float64(v[4]) + K.STEPS * np.float64(np.spacing(v[4]))).astype(np.float32)            # ulps of v itself
    assert len(np.unique(tiny)) == len(tiny) and len(np.unique(M.unnormalise(tiny, [lo], [hi]))) == 1
    v = K.ladder(-0.995, lo, hi)                                       # next to the minimum: v + 1 is small, the rungs still move u
    assert len(np.unique(M.unnormalise(v, [lo], [hi]))) == len(v)


@pytest.mark.parametrize("ni", [0, 1, 5, 16])
def test_map_cell_edges_hold_both_verdicts(ni):
    c = K.map_edge_case(ni)
    free = K.model(c)[0][0]
    _assert_reaches_its_edge(free, c.ladders, c.name)
    at = np.array([int(np.nonzero((c.x[s, :, :2] != c.x[s, 10, :2]).any(-1))[0][0]) for s in c.ladders[:, 0]])
    for s in ([0, 31, 62, H - 1] if ni == 0 else [0, 31, 62]):         # at every place of the embedding
        v = free[c.ladders[at == s]]
        assert v.size and v.any() and not v.all(), (ni, s)
    # nothing but the embedded points decides: the base trajectory alone is free
    base = c.x[c.ladders[:, 0]].copy()
    base[:] = base[:, 10:11]
    assert M.free_flags(M.unnormalise(base, c.norm_min, c.norm_max), K.guide_params(c)[0], ni, c.margin, c.q_min, c.q_max).all()


@pytest.mark.parametrize("ni", [0, 5])
def test_workspace_walls_hold_both_verdicts(ni):
    c = K.wall_case(ni)
    free = K.model(c)[0][0]
    _assert_reaches_its_edge(free, c.ladders, c.name)
    v = free[c.ladders]
    assert (v.any(1) & ~v.all(1)).all()                                 # every wall at every place
    # the wall alone decides: with the walls far away every sample is free
    gp = K.guide_params(c)[0]
    gp.ws_min, gp.ws_max = torch.tensor([-9.0, -9.0]), torch.tensor([9.0, 9.0])
    assert M.free_flags(M.unnormalise(c.x, c.norm_min, c.norm_max), gp, ni, c.margin, c.q_min, c.q_max).all()
    assert not c.default_settings


def test_joint_limits_hold_on_inside_and_outside():
    c = K.limit_case()
    free = K.model(c)[0][0]
    _assert_reaches_its_edge(free, c.ladders, c.name)
    u = M.unnormalise(c.x, c.norm_min, c.norm_max)
    for ladder in c.ladders:
        off = np.abs(u[ladder, :, :2]).max(axis=(1, 2))                # the one coordinate at the limit is the largest
        assert (off == 1).any() and (off < 1).any() and (off > 1).any()
        assert np.array_equal(free[ladder], off <= 1)                   # the bounds are included, and nothing else decides
    places = sorted({int(np.nonzero(np.abs(u[l[0], :, :2]).max(-1) > 0.9)[0][0]) for l in c.ladders})
    assert places == [0, 31, H - 1]


def test_robot_robot_margin_holds_both_verdicts_an_exact_pair_and_the_own_path():
    c = K.margin_case()
    free, key, idx, n_free, _ = K.model(c)
    R, B, m = c.R, c.B, np.float32(c.rr_margin)
    assert (c.paths_all.shape[0], c.robot0, R) == (7, 2, 3)
    d = K.planted_distance(c)
    _assert_reaches_its_edge(d < m, c.ladders, c.name)
    assert {int(t) for j, t in c.note["planted"] if j >= 0} == {0, 31, H - 1}
    exact = np.nonzero(d == m)[0]
    assert len(exact) >= 4                                              # exactly at the margin: not a hit ('<')
    u = M.unnormalise(c.x, c.norm_min, c.norm_max)
    for r in range(R):
        own = c.paths_all[c.robot0 + r]
        assert np.array_equal(u[r * B + 1, :, :2].view(np.int32), own.view(np.int32))             # its own path, bit for bit
        assert F.pos_norm(u[r * B + 1, :, :2], own).max() == 0
        nxt = c.robot0 + (r + 1) % R
        alone = M.collision_counts(u[r * B:r * B + 1, :, :2], c.paths_all[[c.robot0 + r, nxt]], 0, m)
        assert int(alone[0]) == H and key[r, 0] >= H                    # 64 hits from the next robot's row alone
        # a self that is not skipped (or a skip of the wrong row) changes the counts
        wrong = M.collision_counts(u[r * B:(r + 1) * B, :, :2], c.paths_all, r, m)
        assert (wrong != key[r]).any() and wrong[1] >= H
    for n in exact:                                                     # the exact pairs count nothing at their planted step
        j, t = c.note["planted"][n]
        others = [k for k in range(7) if k != c.robot0 + n // B]
        assert not (F.pos_norm(u[n, t, :2], c.paths_all[others, t]) < m).any()


def test_phantom_segment_cases_would_change_with_a_segment_to_the_origin():
    c = K.phantom_cost_case()
    free, key, idx, n_free, _ = K.model(c)
    assert free.all() and idx.tolist() == [0] and key[0, 0] < key[0, 1] and K.cost_gap_ok(c)
    u = M.unnormalise(c.x, c.norm_min, c.norm_max).astype(np.float64)
    phantom = np.linalg.norm(u[:, -1, :2], axis=-1) + np.linalg.norm(u[:, -1, 2:], axis=-1)
    assert key[0, 0] + phantom[0] > (key[0, 1] + phantom[1]) * (1 + 1e-3)
    c = K.phantom_map_case()
    free, key, idx, n_free, _ = K.model(c)
    assert free.all() and idx.tolist() == [0] and K.cost_gap_ok(c)
    u = M.unnormalise(c.x, c.norm_min, c.norm_max)
    gp = K.guide_params(c)[0]
    seg = torch.from_numpy(np.stack([u[0, -1], np.zeros(4, np.float32)])[None])                    # last point -> (0, 0, 0, 0)
    hit = O.compute_collision(O.interpolate_traj_via_points(seg, c.ni)[..., :2], gp, c.margin)
    assert bool(hit.any())
    assert float(gp.sdf_grids[0][0][200, 200]) < 0                      # the origin lies inside an obstacle of the map


@pytest.mark.parametrize("kind", K.PICK_KINDS)
def test_pick_size_cases_cover_what_they_name(kind):
    cs = K.pick_size_cases(kind)
    assert [(c.B, c.R) for c in cs[::3]] == [(B, R) for B in E.PICK_B for R in E.PICK_R]
    assert any(c.x.shape[0] % 4 for c in cs)
    beyond = 0
    for c in cs:
        free, key, idx, n_free, _ = K.model(c)
        B, R, share = c.B, c.R, c.note["share"]
        assert np.array_equal(free, c.note["free"]), c.name           # free exactly the samples built to be
        assert (n_free == 0).all() if share == 0 else (n_free == B).all() if share == 1 and kind != "nan" else (n_free >= 1).all()
        assert K.cost_gap_ok(c) is (None if kind == "counts" else True), c.name
        assert (c.paths_all is not None) == (kind == "counts")
        beyond += int((idx >= 64).sum())
        for r in range(R):
            cand = free[r] if free[r].any() else np.ones(B, bool)
            assert cand[idx[r]]
            if kind == "counts":
                assert np.array_equal(key[r], c.note["hits"][r])       # the counts are the planted ones
                tie = c.note["ties"][r]
                if tie:
                    assert 0 not in tie and idx[r] == tie[0] and (key[r, tie] == key[r, cand].min()).all() and key[r, 0] > key[r, tie[0]]
                if B > 64 and r == 0:
                    assert tie[:2] == [63, 64]
            if kind == "ties":
                tie = c.note["ties"][r]
                assert idx[r] == tie[0] and all(np.array_equal(c.x[r * B + i].view(np.int32), c.x[r * B + tie[0]].view(np.int32)) for i in tie)
                assert len(tie) > 1 or B == 1
            if kind == "nan":
                assert np.isnan(key[r, idx[r]]) and np.isnan(key[r, cand]).sum() >= (2 if B > 65 else 1)
                if share == 0 and B > 1:
                    assert idx[r] == 1 and np.isnan(c.x[r * B + 1, :, :2]).any()      # a NaN position among the only candidates
                if share > 0:
                    assert idx[r] == c.note["nan_free"][0] and not np.isnan(c.x[r * B + idx[r], :, :2]).any()
                    assert B == 1 or (np.isnan(key[r, 1]) and not free[r, 1])          # the NaN that is no candidate does not win
        assert not np.isinf(key).any()
    assert beyond >= 4                                                  # picks the scan finds in its second or third trip


def test_two_maps_decide_differently():
    c = K.two_map_case()
    free = K.model(c)[0]
    B = c.B
    assert np.array_equal(c.x[:B], c.x[B:2 * B]) and np.array_equal(c.x[:B], c.x[2 * B:])
    assert np.array_equal(free[0], free[2]) and (free[0] != free[1]).sum() >= 8
    assert free[0].any() and not free[0].all()


def test_extra_objects_hold_both_verdicts_on_an_empty_fixed_map():
    c = K.extra_object_case()
    free = K.model(c)[0][0]
    _assert_reaches_its_edge(free, c.ladders, c.name)
    assert len(c.ladders) >= 40
    bare = K.Case("extra_objects_without", c.x, c.maps)
    assert M.free_flags(M.unnormalise(c.x, c.norm_min, c.norm_max), K.guide_params(bare)[0], c.ni, c.margin, c.q_min, c.q_max).all()
    # spheres and boxes both decide: without either kind some verdicts change
    for kind in ("spheres", "boxes"):
        gp = K.guide_params(c)[0]
        if kind == "spheres":
            gp.extra_spheres = gp.extra_spheres[:0]
        else:
            gp.extra_boxes = gp.extra_boxes[:0]
        other = M.free_flags(M.unnormalise(c.x, c.norm_min, c.norm_max), gp, c.ni, c.margin, c.q_min, c.q_max)
        assert (other != free).sum() >= 20, kind
