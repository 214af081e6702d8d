"""-m gpu: every collision decision at its margin.  Pairs (and points next to extra objects) a few ulps either side of the margin, so
that the order of the fp32 operations of the distance decides; each kernel is asserted bitwise against the oracle's own torch expression
run on the CPU in fp32 (the form the goldens were made with): check_rr_collisions, count_collisions, find_conflicts in both modes,
scan_candidates, and the extra-object occupancy of compute_collision / get_trajs_collision_and_free."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp32_forms as F                   # noqa: E402
import parity_log                        # noqa: E402
from oracle import mmd_oracle as O       # noqa: E402

H = 64
MIN_SIDE = 300                           # pairs each kernel sees on each side of the margin


def _both_sides(d, margin=F.MARGIN):
    below, above = F.sides(d, margin)
    assert below >= MIN_SIDE and above >= MIN_SIDE, (below, above)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _record_gpu_torch(case, pa, pb, margin=F.MARGIN):
    """The same torch expression on the device: its decisions against the CPU's, recorded only (the reference really runs on a device)."""
    d = torch.from_numpy(np.asarray(pa, np.float32) - np.asarray(pb, np.float32))
    cpu = torch.norm(d, dim=-1) < float(margin)
    gpu = (torch.norm(d.cuda(), dim=-1) < float(margin)).cpu()
    parity_log.record("margin_gpu_torch", case, None, int((cpu != gpu).sum()), note=f"of {cpu.numel()} near-margin pairs")


def _pair_paths(seed, n_pairs):
    """[4, T, 2]: robots 0 / 1 and 2 / 3 hold near-margin pairs at every t."""
    pa, pb = F.margin_pairs(seed, n_pairs)
    qa, qb = F.margin_pairs(seed + 1, n_pairs)
    m = min(len(pa), len(qa))
    return np.stack([pa[:m], pb[:m], qa[:m], qb[:m]])


def test_rr_collisions_at_the_margin():
    """mmd_rr_collisions: the mask, the NaN pattern and the midpoint values bitwise O.check_rr_collisions."""
    from mmd_amd import multi_agent as ma
    paths = _pair_paths(11, 2048)
    _both_sides(F.pos_norm(paths[0], paths[1]))
    _record_gpu_torch("rr_collisions", paths[0], paths[1])
    coll, mid = ma.check_rr_collisions(torch.from_numpy(paths).cuda())
    wc, wm = O.check_rr_collisions(torch.from_numpy(paths).permute(1, 0, 2))
    assert coll.shape == wc.shape
    bad = int((coll.cpu() != wc).sum())
    assert bad == 0, f"{bad} of {wc.numel()} decisions differ"
    got, want = mid.cpu().numpy(), wm.numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(_bits(got[keep]), _bits(want[keep]))


def test_count_collisions_at_the_margin():
    """mmd_count_collisions: every sample's count bitwise O.count_collisions_with_others; samples near some other robot at every t."""
    from mmd_amd import multi_agent as ma
    rng = np.random.default_rng(21)
    N, B, robot0, n_local = 4, 24, 1, 2
    paths = rng.uniform(-0.9, 0.9, (N, H, 2)).astype(np.float32)
    trajs = np.zeros((n_local * B, H, 4), np.float32)
    d = []
    for r in range(n_local):
        self_idx = robot0 + r
        others = np.array([j for j in range(N) if j != self_idx])
        j = others[rng.integers(0, len(others), (B, H))]
        anchor = paths[j, np.arange(H)[None, :]]                        # [B, H, 2]
        trajs[r * B:(r + 1) * B, :, :2] = F.near_points(rng, anchor, F.MARGIN)
        d.append(F.pos_norm(trajs[r * B:(r + 1) * B, :, :2], anchor))
    _both_sides(np.concatenate(d))
    got = ma.count_collisions(torch.from_numpy(trajs).cuda(), torch.from_numpy(paths).cuda(), robot0, n_local).cpu()
    for r in range(n_local):
        want = O.count_collisions_with_others(torch.from_numpy(trajs[r * B:(r + 1) * B, :, :2]), torch.from_numpy(paths), robot0 + r)
        assert got[r].tolist() == want.tolist(), r


def _want_conflicts(pos, ordered):
    """get_conflicts on the padded positions pos [Tg, n, 2]: (t, a, b) row-major, a != b (CBS) or a < b (PP); words as mmd_conflict."""
    coll, mid = O.check_rr_collisions(torch.from_numpy(pos))
    nz = torch.nonzero(coll).numpy()
    if not ordered:
        nz = nz[nz[:, 1] < nz[:, 2]]
    t, a, b = nz[:, 0], nz[:, 1], nz[:, 2]
    w = np.zeros((len(nz), 12), np.int32)
    w[:, 0], w[:, 1], w[:, 2] = t, a, b
    w[:, 4:6] = _bits(pos[t, a])
    w[:, 6:8] = _bits(pos[t, b])
    w[:, 8:10] = _bits(mid.numpy()[t, a, b])
    return w


@pytest.mark.parametrize("ordered", [True, False])
def test_find_conflicts_at_the_margin(ordered):
    """mmd_find_conflicts, both modes: the count, every record and the first record bitwise get_conflicts on the padded paths."""
    from mmd_amd import multi_agent as ma
    paths = _pair_paths(31, 1536)                                      # [4, T, 2]
    n, T = paths.shape[:2]
    _both_sides(F.pos_norm(paths[0], paths[1]))
    batches = []
    for k in range(n):
        b = np.random.default_rng(40 + k).uniform(-1, 1, (2, T, 4)).astype(np.float32)
        b[1, :, :2] = paths[k]
        batches.append(torch.from_numpy(b).cuda())
    table = ma.agent_table(batches, [1] * n, [0] * n)
    want = _want_conflicts(np.ascontiguousarray(paths.transpose(1, 0, 2)), ordered)
    mode = ma.ORDERED if ordered else ma.PAIRS
    summ, lst = ma.find_conflicts(table, n, T, mode, list_cap=len(want) + 4)
    h = summ.cpu().numpy()
    assert int(h[0]) == len(want)
    got = lst.cpu().numpy()[:len(want)]
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f"{bad.size} of {len(want)} records differ, first at {bad[:1]}"
    np.testing.assert_array_equal(h[4:16], want[0])


def test_scan_candidates_at_the_margin():
    """mmd_scan_candidates: every candidate's count (with_counts) and the CBS / PP picks, both modes, against the counts of
    O.check_rr_collisions on the state with that candidate put in."""
    from mmd_amd import multi_agent as ma
    rng = np.random.default_rng(51)
    L, Bc, n = 64, 80, 3
    other = np.zeros((n, L, 2), np.float32)
    other[1] = rng.uniform(-0.9, 0.9, (L, 2))
    other[2] = F.near_points(rng, other[1], F.MARGIN)                  # the base rows hold near-margin pairs too
    j = rng.integers(1, n, (Bc, L))
    anchor = other[j, np.arange(L)[None, :]]
    cand = np.zeros((Bc, L, 4), np.float32)
    cand[..., :2] = F.near_points(rng, anchor, F.MARGIN)
    _both_sides(F.pos_norm(cand[..., :2], anchor))
    # reference: the ordered count of the whole state per candidate
    pos = np.broadcast_to(other.transpose(1, 0, 2)[None], (Bc, L, n, 2)).copy()
    pos[:, :, 0] = cand[..., :2]
    coll, _ = O.check_rr_collisions(torch.from_numpy(pos))
    ordered_counts = coll.sum(dim=(1, 2, 3)).numpy()
    pairs_counts = torch.triu(coll.to(torch.int64), diagonal=1).sum(dim=(1, 2, 3)).numpy()
    batches = [torch.from_numpy(cand).cuda()] + [torch.from_numpy(np.concatenate([other[k], np.zeros((L, 2), np.float32)], -1)[None]).cuda()
                                                  for k in (1, 2)]
    table = ma.agent_table(batches, [0, 0, 0], [0, 0, 0])
    init = int(rng.integers(0, Bc))
    free = rng.permutation(np.array([c for c in range(Bc) if c != init]))[:Bc - 8]
    for mode, want_all in ((ma.ORDERED, ordered_counts), (ma.PAIRS, pairs_counts)):
        res, counts = ma.scan_candidates(table, n, L, 0, batches[0], torch.from_numpy(free).cuda(), mode, ma.SELECT_CBS, with_counts=True)
        want = want_all[free]
        bad = int((counts.cpu().numpy() != want).sum())
        assert bad == 0, f"{bad} of {len(free)} counts differ"
        k = int(np.argmin(want))
        assert res.cpu().tolist() == [int(free[k]), int(want[k])]
        res = ma.scan_candidates(table, n, L, 0, batches[0], torch.from_numpy(free).cuda(), mode, ma.SELECT_PP, init_idx=init)
        pick = [int(free[k]), int(want[k])] if want[k] < want_all[init] else [init, int(want_all[init])]
        assert res.cpu().tolist() == pick


def _extra_objects():
    spheres = np.array([[-0.4, 0.3, 0.12], [0.35, -0.25, 0.071], [0.05, 0.55, 0.2]], np.float32)
    boxes = np.array([[0.3, 0.35, 0.3, 0.18], [-0.35, -0.4, 0.22, 0.34]], np.float32)       # (cx, cy, sx, sy)
    return spheres, boxes


def _points_at(rng, spheres, boxes, margin, n_per):
    """Points whose extra-object sdf is margin (1 + delta): around the spheres, on the flat sides of the rounded boxes and around their
    corners.  -> (points float32 [m, 2], number of corner / sphere points, whose distance is a 2-D norm)."""
    pts, n_norm = [], 0
    for cx, cy, r in spheres:
        c = np.broadcast_to(np.array([cx, cy], np.float32), (n_per, 2))
        pts.append(F.near_points(rng, c, float(r) + float(margin)))
        n_norm += n_per
    for cx, cy, sx, sy in boxes:
        half = np.array([sx, sy], np.float64) / 2
        rad = 0.15 * min(float(sx), float(sy))
        e = half - rad                                                  # the inner box
        s = rng.choice([-1.0, 1.0], (n_per, 2))
        # corners: inner corner + (rad + margin) in a direction of the corner's quadrant
        phi = rng.uniform(0.02, np.pi / 2 - 0.02, n_per)
        r = (rad + float(margin)) * (1 + rng.uniform(-4e-7, 4e-7, n_per))
        p = np.array([cx, cy]) + s * (e + r[:, None] * np.stack([np.cos(phi), np.sin(phi)], 1))
        pts.append(p.astype(np.float32))
        n_norm += n_per
        # flat sides: x or y beyond the side by margin (1 + delta), the other coordinate inside the inner box
        u = rng.uniform(-1, 1, n_per) * e[1]
        v = rng.uniform(-1, 1, n_per) * e[0]
        w = half + float(margin) * (1 + rng.uniform(-4e-7, 4e-7, (n_per, 2)))
        side = np.where(rng.integers(0, 2, n_per)[:, None] == 0, np.stack([w[:, 0], u], 1), np.stack([v, w[:, 1]], 1))
        pts.append((np.array([cx, cy]) + s * side).astype(np.float32))
    return np.concatenate(pts), n_norm


def test_extra_object_occupancy_at_the_margin():
    """compute_collision (margin = collision margin + cutoff) and get_trajs_collision_and_free (margin = robot radius) with extra spheres
    and rounded boxes, on points a few ulps either side of the margin: bitwise O.compute_collision / O.get_trajs_collision_and_free."""
    import cases
    import gpu_common
    from mmd_amd import postprocess as post
    from mmd_amd.guides import GuideManagerTrajectoriesWithVelocity
    from mmd_amd.planners import PlanningTaskFacade, RobotPlanarDiskFacade
    spheres, boxes = _extra_objects()
    xo = {"spheres": spheres.tolist(), "boxes": boxes.tolist()}
    guide = GuideManagerTrajectoriesWithVelocity(gpu_common.dataset(), env_id="EnvEmpty2D", extra_objects=xo, device="cuda")
    gp = cases.guide_params("EnvEmpty2D")
    gp.extra_spheres, gp.extra_boxes = torch.from_numpy(spheres), torch.from_numpy(boxes)
    rng = np.random.default_rng(61)
    # (a) the task's occupancy at the guide margin
    pts, _ = _points_at(rng, spheres, boxes, gp.margin, 600)
    sdf = O.extra_objects_sdf(torch.from_numpy(pts), gp)[0].numpy()
    _both_sides(sdf, np.float32(gp.margin))
    want = O.compute_collision(torch.from_numpy(pts), gp)
    got = PlanningTaskFacade(guide, RobotPlanarDiskFacade(torch.device("cuda"))).compute_collision(torch.from_numpy(pts)).cpu().reshape(-1)
    bad = int((got != want).sum())
    assert bad == 0, f"compute_collision: {bad} of {len(pts)} decisions differ"
    # (b) the free / colliding split at the robot radius: one constant trajectory per point
    pts, _ = _points_at(rng, spheres, boxes, gp.robot_radius, 120)
    sdf = O.extra_objects_sdf(torch.from_numpy(pts), gp)[0].numpy()
    _both_sides(sdf, np.float32(gp.robot_radius))
    trajs = np.zeros((len(pts), H, 4), np.float32)
    trajs[..., :2] = pts[:, None]
    _, _, _, want_free, want_wp = O.get_trajs_collision_and_free(torch.from_numpy(trajs), gp)
    _, _, _, got_free, got_wp = post.get_trajs_collision_and_free(torch.from_numpy(trajs).cuda(), guide)
    assert torch.equal(got_wp.cpu().reshape(want_wp.shape), want_wp)
    assert torch.equal(got_free.cpu(), want_free)
