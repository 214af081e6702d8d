"""-m gpu: the cell-binned inter-robot constraint table (mmd_bin_constraints_from_paths) against a numpy brute force, and the guided step
on it (ddpm_guide_binned_kernel) against the step on the all-pairs table of the same paths.  The yardstick is exact: a slot of the dense
table that does not act adds nothing to its accumulator, the cell lists are in ascending robot id, so the binned step must return the
SAME BITS (csrc/guide.hip, the comment above bin_cell) -- at every launch size, through every entry point, sharded or not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                                                        # noqa: E402
from mmd_amd.constraints import binned_constraints_from_paths, soft_constraints_from_paths   # noqa: E402
import cases                                                                     # noqa: E402
from cases import H, D                                                           # noqa: E402
from test_binned_host import cell_index, ulps, R                                 # noqa: E402

T, I, T_START_GUIDE = 25, 9, 13


def test_table_is_the_brute_force_lists():
    n = 37
    starts, goals = synth.start_goal_circle(n, 0.45)
    paths = synth.straight_line_paths(starts, goals, H)
    # planted points: outside the limits, the corners, on cell edges (and an ulp either side), pairs at the acceptance radius
    edge = np.float32(-1.0) + np.float32(7) * np.float32(2.0 / 15)
    planted = [(1.3, -1.2), (-1.3, 1.2), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (edge, edge), (ulps(edge, 1), ulps(edge, -1)),
               (ulps(edge, -1), edge), (0.0, 0.0), (float(R), 0.0), (ulps(R, 1), 0.0), (0.0, ulps(R, -1)), (-1.0, edge), (edge, 1.0)]
    for k, p in enumerate(planted):
        paths[(5 * k + 2) % n, 1 + (11 * k) % (H - 1)] = p
        paths[(5 * k + 3) % n, H - 1 - (7 * k) % 20] = p
    paths[4, 30] = paths[9, 30] = paths[20, 30] = (0.4, -0.4)                     # coincident points of three robots
    tab = binned_constraints_from_paths(torch.from_numpy(paths).cuda(), 0, n)
    assert tab.grid == (15, 15)
    off, ent, ids = tab.lists()
    ncell = 225
    assert off.shape == (H, ncell + 1) and ent.shape == (H, 9 * n, 4)
    assert (off[:, 0] == 0).all() and (np.diff(off, axis=1) >= 0).all() and (off[:, -1] <= 9 * n).all()
    assert (off[0] == 0).all()                                                    # time step 0: empty lists
    cells = cell_index(paths)                                                     # [n, H, 2]
    cx, cy = np.divmod(np.arange(ncell), 15)
    n_entries = 0
    for t in range(1, H):
        near = (np.abs(cells[None, :, t, 0] - cx[:, None]) <= 1) & (np.abs(cells[None, :, t, 1] - cy[:, None]) <= 1)   # [cell, robot]
        for c in range(ncell):
            want = np.flatnonzero(near[c])                                        # ascending robot id
            got = ids[t, off[t, c]:off[t, c + 1]]
            assert got.tolist() == want.tolist(), (t, c)
            assert np.array_equal(ent[t, off[t, c]:off[t, c + 1], :2].view(np.int32), paths[want, t].view(np.int32)), (t, c)
        assert off[t, -1] == near.sum()
        n_entries += int(near.sum())
    assert n_entries > 4 * n * (H - 1)                                            # (a point is in 4 to 9 lists)


def _instance(kind, n_agents):
    if kind == "random":
        from mmd_amd import trials
        starts, goals = trials.get_start_goal_pos_random_in_env(n_agents, "EnvHighways2D", seed=0)
        starts, goals = np.asarray(starts, np.float32), np.asarray(goals, np.float32)
    else:
        starts, goals = synth.start_goal_circle(n_agents, 0.45)
    return starts, goals, synth.straight_line_paths(starts, goals, H)


def _guides(paths, robot0, n_local):
    """(dense, binned, unconstrained) guides of the local robots over the same best paths"""
    import gpu_common as gc
    p = torch.from_numpy(paths).cuda()
    out = []
    for table in ("dense", "binned", None):
        g = gc.hip_guide("EnvHighways2D", [[] for _ in range(n_local)], n_robots=n_local)
        if table == "dense":
            g.set_packed_constraints(soft_constraints_from_paths(p, robot0, n_local))
        elif table == "binned":
            g.set_binned_constraints(binned_constraints_from_paths(p, robot0, n_local))
        out.append(g)
    return out


def _hard(starts, goals, robot0, n_local):
    rows = [cases.hard_conds_for(starts[r], goals[r]) for r in range(robot0, robot0 + n_local)]
    return {0: torch.stack([h[0] for h in rows]), H - 1: torch.stack([h[H - 1] for h in rows])}


@pytest.mark.parametrize("n_agents,robot0,n_local,B,kind", [
    (10, 0, 2, 8, "circle"),        # baseline
    (10, 0, 2, 5, "circle"),        # a workgroup straddles two robots, idle waves at the end
    (48, 46, 2, 4, "circle"),       # self exclusion and the id > self shift at the top end; N - 1 not a multiple of 4
    (300, 0, 2, 8, "circle"),       # every path crosses the centre: one cell's list holds ~299 entries, lanes near the ends none
    (20, 0, 2, 4, "random"),        # empty cells and short lists
    (10, 0, 10, 64, "circle"),      # 640 trajectories: past the cooperative kernel's launch size
], ids=["10_2x8", "10_2x5_straddle", "48_top_2x4", "300_2x8_centre", "20_random_2x4", "10_10x64"])
def test_binned_step_is_bitwise_the_dense_step(n_agents, robot0, n_local, B, kind):
    import gpu_common as gc
    model = gc.hip_model(T)
    starts, goals, paths = _instance(kind, n_agents)
    hc = _hard(starts, goals, robot0, n_local)
    n = n_local * B
    x = torch.from_numpy(synth.synth_noise(420, (n, H, D))) * 0.5
    nz = torch.from_numpy(synth.synth_noise(421, (n, H, D))).cuda()

    def step(guide):
        y = x.clone().cuda()
        model.sample_step(y, hc, I, guide=guide, n_guide_steps=20, t_start_guide=T_START_GUIDE, noise_std_extra_schedule_fn=lambda t: 0.5,
                          n_robots=n_local, noise=nz)
        return y.cpu()
    dense, binned, free = (step(g) for g in _guides(paths, robot0, n_local))
    assert torch.isfinite(dense).all() and torch.isfinite(binned).all()
    assert torch.equal(binned, dense), float((binned - dense).abs().max())
    assert not torch.equal(dense, free)                                           # the constraints acted


def test_binned_guide_steps_chain_is_bitwise_the_dense_one():
    """mmd_guide_steps, the guide-only launch: every row of the chain"""
    n_agents, n_local, B, n_steps = 24, 3, 4, 6
    starts, goals, paths = _instance("circle", n_agents)
    hc = _hard(starts, goals, 5, n_local)
    hard = torch.stack([hc[0], hc[H - 1]], 1).contiguous().cuda()
    from mmd_amd import _lib
    x = torch.from_numpy(synth.synth_noise(430, (n_local * B, H, D))) * 0.4
    rows = []
    for g in _guides(paths, 5, n_local):
        y, chain = x.clone().cuda(), torch.empty((n_steps, n_local * B, H, D), device="cuda")
        g.guide_steps(y, hard, _lib.HARD_ROWS_START_GOAL, n_steps, chain=chain)
        assert torch.equal(chain[-1], y)
        rows.append(chain.cpu())
    dense, binned, free = rows
    assert torch.isfinite(dense).all()
    for k in range(n_steps):
        assert torch.equal(binned[k], dense[k]), k
    assert not torch.equal(dense[0], free[0])


def test_round_with_the_binned_table_is_the_dense_round():
    """MultiRobotSampler(constraint_table="binned"): plan_round (mmd_p_sample_loop, in-kernel noise) gives the dense round's trajectories and
    best paths; rank 1 of a world of 2, played on this GPU, gives rows 3-5 of the unsharded run"""
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    model = gc.hip_model(T)
    Rn, B = 6, 8
    starts, goals = synth.start_goal_circle(Rn, 0.45)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    dense = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B)
    binned = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, constraint_table="binned")
    td, bd = dense.plan_round(paths, seed=31)
    tb, bb = binned.plan_round(paths, seed=31)
    assert binned.guide._binned is not None and binned.guide._external_cons is None
    assert torch.isfinite(td).all() and torch.equal(tb, td) and torch.equal(bb, bd)
    free = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, inter_robot=False)
    assert not torch.equal(free.plan_round(paths, seed=31)[0], td)
    part = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=B, rank=1, world_size=2, constraint_table="binned")
    assert part.robot0 == 3
    part.set_other_paths(paths)
    tp = part.sample(seed=31)
    assert torch.equal(tp, td[3 * B:6 * B])
    assert torch.equal(part.best_paths(tp, paths), bd[3:6])
    binned.set_other_paths(None)                                                  # reset_extra_costs clears the table
    assert binned.guide._binned is None


def test_two_chunk_loop_with_the_binned_table():
    """mmd_p_sample_loop above 512 trajectories: two stream chunks, each launching the binned kernel on its own trajectory range"""
    import gpu_common as gc
    from mmd_amd.multi_robot import MultiRobotSampler
    model = gc.hip_model(T)
    starts, goals = synth.start_goal_circle(10, 0.45)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    out = []
    for table in ("dense", "binned"):
        s = MultiRobotSampler(model, starts, goals, env_id="EnvEmpty2D", n_samples=64, constraint_table=table)
        s.set_other_paths(paths)
        out.append(s.sample(seed=8).cpu())
    assert torch.isfinite(out[0]).all() and torch.equal(out[1], out[0])
