"""-m gpu: the post-sampling kernels of mmd_amd/csrc/postprocess.hip at their edges, on the inputs of tests/post_edge_cases.py (whose both
sides tests/test_post_edges_host.py asserts on the oracle alone).  Occupancy decisions, free / colliding splits and picks must EQUAL the
oracle's; path length, smoothness, the Savitzky-Golay output and the waypoint variance are held to bounds derived from fp32 rounding against
float64 references; the un-normalisation must equal the CPU form of LimitsNormalizer.unnormalize, NaN positions included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases                             # noqa: E402
import parity_log                        # noqa: E402
import post_edge_cases as E              # noqa: E402
from oracle import mmd_oracle as O       # noqa: E402

_CACHE = {}


def _gp(map_name=E.MAP):
    return cases.guide_params(map_name)


def _guide():
    if "guide" not in _CACHE:
        import gpu_common
        _CACHE["guide"] = gpu_common.hip_guide(E.MAP, [[]])
    return _CACHE["guide"]


def _assert_split_equals_oracle(trajs, guide, gp, ni, tag):
    """waypoint_collisions and free_idxs of post.get_trajs_collision_and_free equal the oracle's; -> the oracle's (free_idxs, waypoints)."""
    from mmd_amd import postprocess as post
    t = torch.from_numpy(trajs)
    _, _, _, want_free, want_wp = O.get_trajs_collision_and_free(t, gp, num_interpolation=ni)
    _, _, _, got_free, got_wp = post.get_trajs_collision_and_free(t.cuda(), guide, num_interpolation=ni)
    assert got_wp.shape == want_wp.shape, (tag, got_wp.shape, want_wp.shape)
    bad = int((got_wp.cpu() != want_wp).sum())
    assert bad == 0, f"{tag}: {bad} of {want_wp.numel()} waypoint decisions differ"
    assert torch.equal(got_free.cpu(), want_free), tag
    return want_free, want_wp


# ---- occupancy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["robot_radius", "guide_margin"])
def test_compute_collision_at_cell_edges_and_workspace_walls(which):
    """mmd_points_collision on points -2 .. +2 ulps around SDF cell edges whose cells decide differently, and around the four workspace
    walls: every decision equals O.compute_collision.  A grid index computed with a reciprocal or an FMA would move the flip."""
    from mmd_amd import postprocess as post
    gp = _gp()
    margin = gp.robot_radius if which == "robot_radius" else gp.margin
    pts = np.concatenate([E.cell_edge_points(gp, margin, 3)[0].reshape(-1, 2), E.ws_boundary_points(gp, margin)])
    want = O.compute_collision(torch.from_numpy(pts), gp, margin)
    assert int(want.sum()) >= 300 and int((~want).sum()) >= 300
    got = post.compute_collision(torch.from_numpy(pts).cuda(), _guide(), margin=margin).cpu()
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {len(pts)} decisions differ"
    if which == "guide_margin":                                        # the default margin is the guide's
        assert torch.equal(post.compute_collision(torch.from_numpy(pts).cuda(), _guide()).cpu(), want)


@pytest.mark.parametrize("ni", [1, 5, 16])
def test_split_at_cell_edges_limits_and_block_seams(ni):
    """mmd_postprocess_trajs with 1, 5 and 16 (= MAX_INTERP) interpolants: segments whose ends lie within 8 ulps of a cell edge, support points
    on / 1 ulp off the joint limits, and K-block trajectories whose only offending point sits at a seam of the 64-point blocks (the segment of
    lane 63, the support point of lane 0, the last point)."""
    gp, guide = _gp(), _guide()
    free, _ = _assert_split_equals_oracle(E.cell_edge_segments(gp, gp.robot_radius, 5), guide, gp, ni, "cell_edge_segments")
    assert 100 <= len(free) <= 300
    trajs, want = E.limit_trajs(gp)
    free, _ = _assert_split_equals_oracle(trajs, guide, gp, ni, "limit_trajs")
    assert free.reshape(-1).tolist() == np.nonzero(want)[0].tolist()
    for K in (2, 3, 16):
        trajs, want, _ = E.seam_trajs(K, gp)
        free, _ = _assert_split_equals_oracle(trajs, guide, gp, ni, f"seam_trajs({K})")
        assert free.reshape(-1).tolist() == np.nonzero(want)[0].tolist()


def test_split_and_points_with_two_robots_on_two_maps():
    """robot_map: each robot's rows are decided against its own map, in mmd_postprocess_trajs and (map_index) in mmd_points_collision."""
    import gpu_common
    from mmd_amd import postprocess as post
    maps = [E.MAP, "EnvConveyor2D"]
    gps = [_gp(m) for m in maps]
    guide = gpu_common.hip_guide(E.MAP, [[], []], n_robots=2, robot_env_ids=maps)
    rng = np.random.default_rng(17)
    ends = rng.uniform(-0.95, 0.95, (60, 2, 1, 2))
    w = np.linspace(0, 1, E.H)[None, :, None]
    lines = np.zeros((60, E.H, E.D), np.float32)
    lines[..., :2] = ends[:, 0] * (1 - w) + ends[:, 1] * w
    batch = np.concatenate([E.cell_edge_segments(gps[0], gps[0].robot_radius, 6, n=60), lines])
    B = len(batch)
    r = post.postprocess_batch(guide, torch.from_numpy(np.concatenate([batch, batch])).cuda(), n_robots=2, smooth=False, want_waypoints=True)
    want = [O.get_trajs_collision_and_free(torch.from_numpy(batch), gp) for gp in gps]
    assert not torch.equal(want[0][4], want[1][4]) and not torch.equal(want[0][3], want[1][3])           # the maps decide differently
    for k in range(2):
        assert torch.equal(r.waypoint_collisions[k * B:(k + 1) * B].bool().cpu(), want[k][4]), maps[k]
        assert torch.equal(torch.argwhere(r.free_mask[k * B:(k + 1) * B].bool()).cpu(), want[k][3]), maps[k]
    pts = torch.from_numpy(np.concatenate([batch[:, :, :2].reshape(-1, 2), E.cell_edge_points(gps[0], gps[0].margin, 4)[0].reshape(-1, 2)]))
    env_ids = sorted(maps)                                             # the guide's map order
    cw = [O.compute_collision(pts, gps[maps.index(e)]) for e in env_ids]
    assert int((cw[0] != cw[1]).sum()) >= 300
    for m in range(2):
        assert torch.equal(post.compute_collision(pts.cuda(), guide, map_index=m).cpu(), cw[m]), env_ids[m]


def test_all_free_reports_nothing_even_on_colliding_input():
    """all_free (PlanningTaskEnsemble): no waypoint is marked and every sample is free, whatever the input."""
    from mmd_amd import postprocess as post
    gp = _gp()
    trajs, free, _ = E.seam_trajs(2, gp)
    assert (~free).sum() >= 4
    t = torch.from_numpy(trajs).cuda()
    coll, coll_idxs, got_free, free_idxs, wp = post.get_trajs_collision_and_free(t, _guide(), all_free=True)
    assert coll is None and coll_idxs.numel() == 0 and torch.equal(got_free, t)
    assert free_idxs.reshape(-1).tolist() == list(range(len(trajs)))
    assert wp.shape == (len(trajs), (2 * E.H - 1) * 5) and not wp.any()
    want = O.get_trajs_collision_and_free(torch.from_numpy(trajs), gp, all_free=True)
    assert torch.equal(free_idxs.cpu(), want[3]) and not want[4].any()


def test_num_interpolation_zero_tests_the_support_points():
    """num_interpolation = 0: interpolate_traj_via_points returns the trajectory itself, so the SUPPORT points are tested for occupancy (the
    last included) and waypoint_collisions is [B, L]: equal to the oracle on support points either side of cell edges, on the joint limits and
    on K-block trajectories with one support point inside an obstacle."""
    gp, guide = _gp(), _guide()
    free, wp = _assert_split_equals_oracle(E.cell_edge_segments(gp, gp.robot_radius, 5), guide, gp, 0, "cell_edge_segments")
    assert wp.shape == (400, E.H) and int(wp.sum()) >= 300 and int((~wp).sum()) >= 300 and len(free) < 400
    assert int(wp[:, E.H - 1].sum()) >= 30                                # the last support point is tested too
    trajs, want = E.limit_trajs(gp)
    free, _ = _assert_split_equals_oracle(trajs, guide, gp, 0, "limit_trajs")
    assert free.reshape(-1).tolist() == np.nonzero(want)[0].tolist()
    for K in (2, 16):
        trajs, want, seg = E.seam_trajs(K, gp)
        free, wp = _assert_split_equals_oracle(trajs, guide, gp, 0, f"seam_trajs({K})")
        assert free.reshape(-1).tolist() == np.nonzero(want)[0].tolist()
        assert wp.shape == (len(trajs), K * E.H) and [int(torch.nonzero(w)[0]) for w in wp[seg >= 0]] == seg[seg >= 0].tolist()


# ---- path length and smoothness ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 16])
def test_path_length_and_smoothness_within_the_derived_bound(K):
    """Against float64, per trajectory within (L + 2) 2^-24 sum ||diff|| (post_edge_cases.metric_reference): holds for any summation order of
    L - 1 correctly rounded terms; a constant trajectory gives exactly 0."""
    from mmd_amd import postprocess as post
    t = E.metric_trajs(K, 7 + K)
    pl, sm, bpl, bsm = E.metric_reference(t)
    r = post.postprocess_batch(_guide(), torch.from_numpy(t).cuda(), smooth=False)
    for name, got, ref, bound in (("path_length", r.path_length, pl, bpl), ("smoothness", r.smoothness, sm, bsm)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        parity_log.record("post_edges_metrics", f"{name}_K{K}", None, worst, bound=1.0, note="max error / derived bound")
        assert np.all(err <= bound), (name, err.tolist(), bound.tolist())
        assert float(got[4]) == 0.0


# ---- Savitzky-Golay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,window,order", E.SAVGOL_CONFIGS)
def test_savgol_within_the_derived_bound(L, window, order):
    """smooth_trajs and postprocess_batch(smooth=True) against scipy.signal.savgol_filter in float64: per element within
    (2 window + 3) 2^-24 sum_j |S_pj| |v_j|; for L = 128 two signals whose only non-zero sits at the block seam."""
    from mmd_amd import postprocess as post
    t = E.savgol_trajs(L, 9)
    ref, bound = E.savgol_reference(t, window, order)
    x = torch.from_numpy(t).cuda()
    got = post.smooth_trajs(x, _guide(), window_size=window, poly_order=order)
    both = post.postprocess_batch(_guide(), x, smooth=True, window_size=window, poly_order=order).smoothed
    assert torch.equal(got, both)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    parity_log.record("post_edges_savgol", f"L{L}_w{window}_o{order}", None, worst, bound=1.0, note="max error / derived bound")
    assert np.all(err <= bound), (worst, np.unravel_index(np.argmax(err - bound), err.shape))


# ---- waypoint variance -------------------------------------------------------------------------------------------------------------
def _variance_inputs():
    out = [(f"B{B}_L{L}", E.variance_trajs(B, L, 100 * B + L)) for B in E.VAR_B for L in E.VAR_L]
    return out + [(f"tight_B{B}", E.variance_trajs(B, E.H, 50 + B, tight=True)) for B in (17, 100)]


def test_variance_waypoints_against_float64():
    """mmd_variance_waypoints against the float64 form over all B^2 entries of triu(cdist): B = 1 is NaN (torch.var of one element), B = 100
    needs more than one 256-thread pass, and near-identical trajectories (spread 1e-6 around 0.5).  Tolerance: twice the error of the
    oracle's own fp32 form against the same reference on the same input, or 1e-6 relative, whichever is larger."""
    from mmd_amd import postprocess as post
    for tag, t in _variance_inputs():
        ref = E.variance_reference(t)
        got = float(post.compute_variance_waypoints(torch.from_numpy(t).cuda()))
        if t.shape[0] == 1:
            assert np.isnan(ref) and np.isnan(got), tag
            continue
        err_oracle = abs(float(O.compute_variance_waypoints(torch.from_numpy(t))) - ref) / ref
        err = abs(got - ref) / ref
        tol = max(2 * err_oracle, 1e-6)
        parity_log.record("post_edges_variance", tag, None, err, bound=tol, oracle_fp32_err=err_oracle)
        print(f"variance {tag}: kernel {err:.3e} oracle fp32 {err_oracle:.3e} (relative, against float64)")
        assert err <= tol, (tag, err, err_oracle)


# ---- the pick ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.PICK_KINDS)
def test_select_best_equals_the_host_rule(kind):
    """mmd_select_best: idx, n_free and the summary buffer (free flags as floats, then the picks at [R B + r]) equal the host rule -- torch.argmin
    over the candidates' keys (a NaN is the smallest, the first index wins among equals), the first minimum in counts mode."""
    from mmd_amd import postprocess as post
    bad = []
    for c in E.pick_cases(kind):
        dev = lambda v: None if v is None else torch.from_numpy(v).cuda()            # noqa: E731
        summary = torch.full((c["R"] * c["B"] + c["R"],), -7.0, dtype=torch.float32, device="cuda")
        idx, n_free = post.select_best(dev(c["free"]), c["R"], cost_a=dev(c["cost_a"]), cost_b=dev(c["cost_b"]), counts=dev(c["counts"]),
                                       summary=summary)
        if idx.cpu().tolist() != c["idx"].tolist() or n_free.cpu().tolist() != c["n_free"].tolist() or \
                summary.cpu().tolist() != c["summary"].tolist():
            bad.append((c["B"], c["R"], c["share"], idx.cpu().tolist(), c["idx"].tolist()))
    assert not bad, f"{len(bad)} cases differ (B, R, free share, got, want): {bad[:8]}"


def test_select_best_hand_case_with_a_nan_key():
    from mmd_amd import postprocess as post
    a = torch.tensor([5, 4, 6, float("nan"), 7, 8, 9, 1], dtype=torch.float32)
    free = torch.ones(8, dtype=torch.uint8)
    idx, n_free = post.select_best(free.cuda(), 1, cost_a=a.cuda())
    assert int(idx) == int(torch.argmin(a)) == 3 and int(n_free) == 8
    free[3] = 0                                                        # the NaN's sample is no candidate: the smallest number wins
    idx, n_free = post.select_best(free.cuda(), 1, cost_a=a.cuda())
    assert int(idx) == 7 and int(n_free) == 7


# ---- un-normalisation --------------------------------------------------------------------------------------------------------------
def _assert_unnormalize_equals_cpu_form(ds, x, n_tensors, name):
    ref = ds.unnormalize_trajectories(x.clone(), n_tensors=n_tensors)                    # the torch form on the CPU
    got = ds.unnormalize_trajectories(x.cuda(), n_tensors=n_tensors).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), name
    assert torch.allclose(got, ref, rtol=0, atol=0, equal_nan=True), (name, int((~torch.isclose(got, ref, rtol=0, atol=0, equal_nan=True)).sum()))
    return got


def test_unnormalize_with_non_finite_elements_equals_the_cpu_form():
    """mmd_unnormalize_trajs against the CPU form of LimitsNormalizer.unnormalize: with a NaN in a tensor x.max() and x.min() are NaN, so that
    tensor is NOT clipped whatever else it holds, and the NaN stays a NaN; infinities alone are out of range and are clipped."""
    from mmd_amd.normalization import TrajectoryDatasetFacade
    ds = TrajectoryDatasetFacade(E.UNNORM_MINS, E.UNNORM_MAXS)
    for name, x, n_tensors in E.unnorm_cases():
        got = _assert_unnormalize_equals_cpu_form(ds, x, n_tensors, name)
        assert torch.equal(torch.isnan(got), torch.isnan(x)), name
    name, x, _ = next(c for c in E.unnorm_cases() if c[0] == "nan_and_above_0")
    got = ds.unnormalize_trajectories(x.cuda()).cpu()
    assert float(got[7, 6, 40, 1]) > float(E.UNNORM_MAXS[1]) and float(got[1, 0, 3, 0]) > float(E.UNNORM_MAXS[0])       # nothing was clipped


@pytest.mark.parametrize("n_tensors", [1, 4])
def test_unnormalize_chain_with_the_only_outlier_in_the_grid_stride_tail(n_tensors):
    """552,960 points; the only element out of range lies in the last 20,000, which the range kernel reaches only in a later grid-stride
    iteration: the tensor that holds it is clipped (its elements in (1, 1 + eps] come down to the limit), the other tensors of the call not."""
    from mmd_amd.normalization import TrajectoryDatasetFacade
    ds = TrajectoryDatasetFacade(E.UNNORM_MINS, E.UNNORM_MAXS)
    x = E.unnorm_chain_case(n_tensors)
    got = _assert_unnormalize_equals_cpu_form(ds, x, n_tensors, f"chain_{n_tensors}")
    per = x.shape[1] // n_tensors
    above = [float(got[1, c * per, 3, c % 4]) > float(E.UNNORM_MAXS[c % 4]) for c in range(n_tensors)]
    assert above == ([False] if n_tensors == 1 else [True, True, False, True])
