"""Host checks of tests/post_edge_cases.py: on the ORACLE alone, every builder holds both sides of the decision it is built around, so that
no test of tests/test_gpu_post_edges.py can pass by missing its edge.  No GPU; numpy, torch, scipy and oracle.mmd_oracle."""
import numpy as np
import pytest
import torch

import cases
import post_edge_cases as E
from oracle import mmd_oracle as O

MIN_SIDE = 300


@pytest.fixture(scope="module")
def gp():
    return cases.guide_params(E.MAP)


def _margins(gp):
    return (gp.robot_radius, gp.margin)


def test_cell_edge_points_hold_both_sides_and_flip_inside_the_window(gp):
    for margin in _margins(gp):
        pts, axis = E.cell_edge_points(gp, margin, 3)
        assert pts.dtype == np.float32 and pts.shape[1:] == (5, 2) and set(axis.tolist()) == {0, 1}
        assert np.array_equal(pts, E.cell_edge_points(gp, margin, 3)[0])                # seeded
        coll = O.compute_collision(torch.from_numpy(pts), gp, margin).numpy()
        below, above = int(coll.sum()), int((~coll).sum())
        flips = int((coll.any(1) & ~coll.all(1)).sum())
        assert below >= MIN_SIDE and above >= MIN_SIDE, (margin, below, above)
        assert flips >= MIN_SIDE, (margin, flips, len(pts))
    # the count the builder rests on: x-pairs whose decisions differ at the robot radius
    dec = E.decisions(gp, gp.robot_radius)
    assert dec.shape == (400, 400) and int((dec[:-1] != dec[1:]).sum()) == 972


def test_cell_edge_segments_hold_both_sides_and_both_outcomes(gp):
    trajs = E.cell_edge_segments(gp, gp.robot_radius, 5)
    assert trajs.shape == (400, E.H, E.D)
    pairs = E.flip_pairs(gp, gp.robot_radius)
    # every support point within 8 ulps of an edge
    along = np.where(np.ptp(trajs[..., 0], axis=1)[:, None] > 0, trajs[..., 0], trajs[..., 1])
    cell = np.round((along.astype(np.float64) - E.LO) / E.CELL)
    e = E.edge(cell)
    assert np.all(np.abs(along - e) <= 8 * np.spacing(np.abs(e))) and len(pairs[0]) > 0
    t = torch.from_numpy(trajs)
    for ni in (1, 5, 16):
        pts = O.interpolate_traj_via_points(t, ni)[..., :2]
        coll = O.compute_collision(pts, gp, gp.robot_radius)
        assert int(coll.sum()) >= MIN_SIDE and int((~coll).sum()) >= MIN_SIDE, ni
        _, coll_idxs, _, free_idxs, _ = O.get_trajs_collision_and_free(t, gp, num_interpolation=ni)
        assert len(free_idxs) >= 100 and len(coll_idxs) >= 100, (ni, len(free_idxs), len(coll_idxs))


def test_workspace_boundary_points_hold_both_sides(gp):
    for margin in _margins(gp):
        pts = E.ws_boundary_points(gp, margin)
        coll = O.compute_collision(torch.from_numpy(pts), gp, margin).numpy().reshape(4, 5)
        assert coll.any(1).all() and (~coll).any(1).all(), coll                          # each wall: both outcomes
        # the wall alone decides: without the walls every point is free
        far = O.GuideParams(norm_mins=gp.norm_mins, norm_maxs=gp.norm_maxs, sdf_grids=gp.sdf_grids, ws_min=torch.tensor([-9.0, -9.0]),
                            ws_max=torch.tensor([9.0, 9.0]))
        assert not O.compute_collision(torch.from_numpy(pts), far, margin).any()
        d = np.concatenate([np.float32(1.08) - pts[:5, 0], pts[5:10, 0] + np.float32(1.08)])
        assert np.all(np.abs(d - np.float32(margin)) <= 3 * np.spacing(np.float32(1.03)))


def test_limit_trajs_are_free_iff_every_support_point_is_inside_bounds_included(gp):
    trajs, free = E.limit_trajs(gp)
    assert free.sum() == 24 and (~free).sum() == 12
    for ni in (0, 1, 5, 16):
        _, _, _, free_idxs, wp = O.get_trajs_collision_and_free(torch.from_numpy(trajs), gp, num_interpolation=ni)
        assert not wp.any()                                            # the limits alone decide
        assert free_idxs.reshape(-1).tolist() == np.nonzero(free)[0].tolist(), ni
    on = trajs[np.arange(len(trajs)), np.tile(np.repeat([0, 31, E.H - 1], 3), 4)][1::3, :2]                     # the k = 0 rows
    assert np.all(np.abs(on).max(1) == 1.0)


@pytest.mark.parametrize("K", [2, 3, 16])
def test_seam_trajs_are_free_or_colliding_as_designed(gp, K):
    trajs, free, seg = E.seam_trajs(K, gp)
    L = K * E.H
    assert trajs.shape == (2 * (K - 1) + 2 * (K + 1), L, E.D) and free.sum() * 2 == len(free)
    t = torch.from_numpy(trajs)
    for ni in (1, 5, 16):
        _, _, _, free_idxs, wp = O.get_trajs_collision_and_free(t, gp, num_interpolation=ni)
        assert free_idxs.reshape(-1).tolist() == np.nonzero(free)[0].tolist(), ni
        wp = wp.numpy().reshape(len(trajs), L - 1, ni).any(-1)
        for n in range(len(trajs)):                                    # the colliding interpolants lie on the seam segment only
            assert np.nonzero(wp[n])[0].tolist() == ([seg[n]] if seg[n] >= 0 else []), (ni, n)
    assert set(seg[seg >= 0].tolist()) == {E.H * k - 1 for k in range(1, K)}
    # the limit variants: the one offending support point is p = 64 k or p = L - 1
    out = np.nonzero((np.abs(trajs[..., :2]) > 1).any(-1))
    assert sorted(out[1].tolist()) == sorted([E.H * k for k in range(K)] + [L - 1])


def test_expected_pick_rule():
    nan, inf = float("nan"), float("inf")
    a = np.array([5, 4, 6, nan, 7, 8, 9, 1], np.float32)
    one = np.ones(8, np.uint8)
    assert E.expected_pick(one, 8, 1, a)[0].tolist() == [3]            # torch.argmin: a NaN is the smallest
    f = one.copy(); f[3] = 0
    assert E.expected_pick(f, 8, 1, a)[0].tolist() == [7]              # ... unless its sample is no candidate
    idx, n_free, summary = E.expected_pick(np.zeros(8, np.uint8), 8, 1, a)
    assert idx.tolist() == [3] and n_free.tolist() == [0] and summary.tolist() == [0.0] * 8 + [3.0]
    assert E.expected_pick(one, 8, 1, np.full(8, inf, np.float32))[0].tolist() == [0]
    assert E.expected_pick(one, 4, 2, np.array([2, 1, 1, 3, nan, nan, 0, 0], np.float32))[0].tolist() == [1, 0]
    assert E.expected_pick(one, 8, 1, counts=np.array([3, 1, 2, 1, 0, 0, 5, 0], np.int32))[0].tolist() == [4]


@pytest.mark.parametrize("kind", E.PICK_KINDS)
def test_pick_cases_cover_what_they_name(kind):
    cs = E.pick_cases(kind)
    assert len(cs) == len(E.PICK_B) * len(E.PICK_R) * len(E.PICK_SHARES)
    assert {c["n_free"].min() for c in cs if c["share"] == 0.0} == {0} and all((c["n_free"] == c["B"]).all() for c in cs if c["share"] == 1.0)
    assert any(0 < c["n_free"].max() < c["B"] for c in cs if c["share"] == 0.1)
    again = E.pick_cases(kind)
    assert all(np.array_equal(c["free"], d["free"]) and np.array_equal(c["idx"], d["idx"]) for c, d in zip(cs, again))
    for c in cs:
        B, R = c["B"], c["R"]
        assert len(c["free"]) == R * B and c["summary"].shape == (R * B + R,) and ((0 <= c["idx"]) & (c["idx"] < B)).all()
        for r in range(R):
            f = c["free"][r * B:(r + 1) * B].astype(bool)
            cand = f if f.any() else np.ones(B, bool)
            assert cand[c["idx"][r]]
            a = None if c["cost_a"] is None else c["cost_a"][r * B:(r + 1) * B]
            if kind == "nan":
                assert np.isnan(a[cand]).any() and np.isnan(a[c["idx"][r]])
            if kind == "nan_on_non_free" and f.any():
                assert not np.isnan(a[cand]).any() and (np.isnan(a[~f]).any() or f.all())
            if kind == "all_inf":
                assert c["idx"][r] == np.nonzero(cand)[0][0]
            if kind == "ties" and B > 64 and cand[5]:
                assert c["idx"][r] == 5 and a[64] == a[5] == a[cand].min()
    if kind == "counts":
        assert all(c["counts"] is not None and c["cost_a"] is None for c in cs)
    if kind == "inf":
        assert any(np.isinf(c["cost_a"]).any() for c in cs)


def test_metric_reference_and_inputs():
    for K in (1, 2, 16):
        t = E.metric_trajs(K, 7 + K)
        pl, sm, bpl, bsm = E.metric_reference(t)
        assert t.shape == (6, K * E.H, E.D) and pl[4] == 0 and sm[4] == 0 and bpl[4] == 0
        d = np.linalg.norm(np.diff(t[3, :, :2].astype(np.float64), axis=0), axis=1)
        assert d.max() > 500 and np.median(d) < 1e-3                   # one huge segment among tiny ones
        assert int(np.argmax(d)) == (E.H - 1 if K > 1 else 30)
        # the oracle's own fp32 sum obeys the derived bound
        assert np.all(np.abs(O.compute_path_length(torch.from_numpy(t)).numpy() - pl) <= bpl)
        assert np.all(np.abs(O.compute_smoothness(torch.from_numpy(t)).numpy() - sm) <= bsm)


@pytest.mark.parametrize("L,window,order", E.SAVGOL_CONFIGS)
def test_savgol_operator_is_banded_within_the_window(L, window, order):
    """postprocess_batch passes window_size as the band of the operator: every non-zero must lie within it."""
    S = E.savgol_operator64(L, window, order)
    r, c = np.nonzero(S)
    reach = int(np.abs(r - c).max())
    assert reach < window, (reach, window)
    assert reach == {10: 9, 5: 4, 31: 30}[window]
    t = E.savgol_trajs(L, 9)
    ref, bound = E.savgol_reference(t, window, order)
    assert np.abs(S @ t[0].astype(np.float64) - ref[0]).max() < 1e-12                    # the operator IS the filter
    assert bound.shape == ref.shape and (bound[:5] > 0).all()
    if L == 2 * E.H:
        assert [np.nonzero(np.abs(x).sum(-1))[0].tolist() for x in t[5:]] == [[E.H - 1], [E.H]]


def test_variance_reference_and_inputs():
    assert np.isnan(E.variance_reference(E.variance_trajs(1, 64, 1)))
    t = E.variance_trajs(17, 65, 2)
    want = float(O.compute_variance_waypoints(torch.from_numpy(t).double()))
    assert abs(E.variance_reference(t) - want) <= 1e-12 * want
    tight = E.variance_trajs(100, 64, 3, tight=True)
    assert np.abs(tight[..., :2] - 0.5).max() <= 1.1e-6 and len(np.unique(tight[..., 0])) > 8


def test_unnormalize_cases_separate_the_two_readings_of_a_nan():
    """The CPU form (the reference's) leaves a tensor with a NaN unclipped; a clip that ignores the NaN would change these cases."""
    mins, maxs = torch.from_numpy(E.UNNORM_MINS), torch.from_numpy(E.UNNORM_MAXS)
    names = []
    for name, x, n_tensors in E.unnorm_cases():
        names.append(name)
        chunks = x.chunk(n_tensors, dim=1)
        ref = torch.cat([O.unnormalize(c, mins, maxs) for c in chunks], 1)
        forced = torch.cat([O.unnormalize(torch.nan_to_num(c, nan=0.0), mins, maxs) for c in chunks], 1)
        has_nan = [bool(torch.isnan(c).any()) for c in chunks]
        assert (any(has_nan) or name == "infinities") and torch.equal(torch.isnan(ref), torch.isnan(x))       # a NaN stays a NaN, nothing else becomes one
        finite = ~torch.isnan(x)
        differs = bool((ref[finite] != forced[finite]).any())
        assert differs == any(h and bool((c[~torch.isnan(c)].abs() > 1 + 1e-4).any()) for h, c in zip(has_nan, chunks)), name
    assert sum(n.startswith("nan_and_above") for n in names) >= 4
    for n_tensors in (1, 4):
        x = E.unnorm_chain_case(n_tensors)
        assert x.numel() // 4 == 552960 > 2048 * 256
        out = torch.nonzero((x.abs() > 1 + 1e-4).reshape(-1, 4).any(-1)).reshape(-1)
        assert len(out) == 1 and int(out) >= 552960 - 20000
        assert all(((c.abs() > 1) & (c.abs() <= 1 + 1e-4)).any() for c in x.chunk(n_tensors, dim=1))
