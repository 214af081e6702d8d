"""-m gpu: every instantiation of the guided step kernel past its LDS staging.  A constraint group's slots come from two places: the part of
the robot's table that the workgroup staged into LDS and, past the staged slot count, the L2-resident table itself (guide.hip: group_slots).
The slot sum is defined as one fixed tree, so a guided step gives the SAME BITS whichever kernel runs it and wherever the split falls:
the cooperative kernel (guide_coop_max = 0: these launches are <= 512 trajectories), a one-wave kernel (guide_coop_max = -1) and the trace
instantiation (every slot from L2).  Each case is the smallest launch that reaches its split in the one-wave kernel named beside it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                # noqa: E402
import cases                             # noqa: E402
from cases import H, D                   # noqa: E402

T, I, T_START_GUIDE = 25, 9, 13


def _problem(n_agents):
    starts, goals = synth.start_goal_circle(n_agents, 0.45)
    hc = {0: torch.stack([cases.hard_conds_for(starts[r], goals[r])[0] for r in range(2)]),
          H - 1: torch.stack([cases.hard_conds_for(starts[r], goals[r])[H - 1] for r in range(2)])}
    return synth.straight_line_paths(starts, goals, H), hc


def _host_packed(n_agents, hard_on_both):
    """two robots of n_agents on the circle: soft constraints from the n_agents - 1 others (one slot each), robot 0 (or both) + a hard group"""
    import gpu_common as gc
    paths, hc = _problem(n_agents)
    hard = cases.hard_group([[0.1, 0.2]], [[20, 27]])
    groups = [[cases.soft_group(paths, r)] + ([hard] if r == 0 or hard_on_both else []) for r in range(2)]
    return [gc.hip_guide("EnvHighways2D", groups, n_robots=2)], hc


def _device_built(n_agents):
    """the same soft constraints built on the device: with their one radius (compact LDS staging) and without it (general staging)"""
    import gpu_common as gc
    from mmd_amd.constraints import soft_constraints_from_paths
    paths, hc = _problem(n_agents)
    cons = soft_constraints_from_paths(torch.from_numpy(paths).cuda(), 0, 2)
    guides = []
    for c in (cons, cons[:4]):
        g = gc.hip_guide("EnvHighways2D", [[], []], n_robots=2)
        g.set_packed_constraints(c)
        guides.append(g)
    return guides, hc


def _step(model, guide, x, hc, nz, coop_max):
    y = x.clone().cuda()
    model.guide_coop_max = coop_max
    model.sample_step(y, hc, I, guide=guide, n_guide_steps=20, t_start_guide=T_START_GUIDE, noise_std_extra_schedule_fn=lambda t: 0.5,
                      n_robots=2, noise=nz.cuda())
    return y.cpu()


@pytest.mark.parametrize("B,build", [
    (8, lambda: _host_packed(10, False)),    # <4, general>: 9 + 1 and 9 slots, the whole table in LDS
    (5, lambda: _host_packed(10, False)),    # <4, general>: the middle workgroup straddles the robots (stages nothing), the last has two idle waves
    (4, lambda: _host_packed(48, True)),     # <4, general>: 47 + 1 slots, overflow past 40
    (8, lambda: _host_packed(160, True)),    # <8, general>: 159 + 1 slots, overflow past 144; cooperative: past 60
    (4, lambda: _device_built(100)),         # <4, compact>: 99 slots, overflow past 80; cooperative compact holds all (120)
    (8, lambda: _device_built(300)),         # <8, compact>: 299 slots, overflow past 288; cooperative compact: past 120
], ids=["2x8_lds", "2x5_straddle", "2x4_over40", "2x8_over144", "2x4_compact_over80", "2x8_compact_over288"])
def test_guided_step_is_bitwise_the_same_in_every_kernel(B, build):
    import gpu_common as gc
    model = gc.hip_model(T)
    guides, hc = build()
    x = torch.from_numpy(synth.synth_noise(320, (2 * B, H, D))) * 0.5
    nz = torch.from_numpy(synth.synth_noise(321, (2 * B, H, D)))
    keep = model.guide_coop_max
    try:
        unconstrained = _step(model, gc.hip_guide("EnvHighways2D", [[], []], n_robots=2), x, hc, nz, 0)
        ref = None
        for guide in guides:             # (device-built: compact, then general staging of the same table)
            coop = _step(model, guide, x, hc, nz, 0)
            one_wave = _step(model, guide, x, hc, nz, -1)
            traced = gc.hip_step_with_trace(model, x, hc, I, guide, T_START_GUIDE, 2, nz)[0]
            ref = coop if ref is None else ref
            for name, y in (("cooperative", coop), ("one wave", one_wave), ("trace", traced)):
                assert torch.isfinite(y).all(), name
                assert torch.equal(y, ref), (name, float((y - ref).abs().max()))
    finally:
        model.guide_coop_max = keep
    assert not torch.equal(ref, unconstrained)          # the slots acted
