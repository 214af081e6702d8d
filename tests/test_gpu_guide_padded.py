"""-m gpu: the one-wave guided step kernel's padded slot pass and its map-free branch (guide.hip: stage_cons<.., PAD>, PaddedSum, MapFree).
A robot whose ONE constraint group fits the workgroup's LDS staging is summed in trips of eight slots over a table padded with entries that
cannot act; the cooperative kernel never sees the padding and sums the same group through cons_accumulate1.  The slot sum is one fixed
tree, so the two kernels must return the SAME BITS for every slot count around the trip size and the staging size, for two groups per
robot, on rows at the edge of the radius, on rows that are not finite, and on a map without grids as on a map whose grid never acts.
2 robots x 4 samples throughout: one workgroup per robot in the one-wave kernel.  Bits are compared as int32 words (NaN == NaN, +0 != -0)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                # noqa: E402
import cases                             # noqa: E402
import guide_edge_cases as E             # noqa: E402
import test_gpu_guide_edges as TE        # noqa: E402  (its launch helper and its float64 bound; its tests are not collected through this name)
from cases import H, D                   # noqa: E402
from oracle import mmd_oracle as O       # noqa: E402

T, I, T_START_GUIDE = 25, 9, 13
B = 4
TILE = 260                               # 2 x 260 = 520 trajectories, a multiple of 4 per robot: a guide-only launch past the cooperative 512
SLOT_COUNTS = (1, 7, 8, 9, 31, 32, 33, 40, 41)
RADIUS = 0.4                             # wide enough that slots act on a handful of random trajectories


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hard_conds():
    starts, goals = synth.start_goal_circle(6, 0.45)
    return {k: torch.stack([cases.hard_conds_for(starts[r], goals[r])[k] for r in range(2)]) for k in (0, H - 1)}


def _inputs():
    x = torch.from_numpy(synth.synth_noise(330, (2 * B, H, D))) * 0.5
    nz = torch.from_numpy(synth.synth_noise(331, (2 * B, H, D)))
    return x, nz


def _step(model, guide, x, hc, nz, coop_max):
    """one guided ddpm step of the 8 trajectories: guide_coop_max = 0 runs the cooperative kernel, -1 the one-wave kernel"""
    y = x.clone().cuda()
    keep = model.guide_coop_max
    try:
        model.guide_coop_max = coop_max
        model.sample_step(y, hc, I, guide=guide, n_guide_steps=20, t_start_guide=T_START_GUIDE, noise_std_extra_schedule_fn=lambda t: 0.5,
                          n_robots=2, noise=nz.cuda())
    finally:
        model.guide_coop_max = keep
    return y.cpu()


_UNCONSTRAINED = {}


def _unconstrained(model, env, x, hc, nz):
    """the same step without any constraint group, once per map: what a table must differ from if its slots act"""
    import gpu_common as gc
    if env not in _UNCONSTRAINED:
        _UNCONSTRAINED[env] = _step(model, gc.hip_guide(env, [[], []], n_robots=2), x, hc, nz, 0)
    return _UNCONSTRAINED[env]


def _slot_table(n_slots, table):
    """(ell, grp_slot_off, grp_weight, robot_grp_off[, radius]) of 2 robots with ONE group of n_slots slots each: the all-pairs table of
    n_slots + 1 robots on a circle.  compact: as built, one radius (the 5-tuple: (qx, qy) staged).  general: a radius of its own per slot
    and a fifth of the entries emptied (R < 0), without the radius (the (qx, qy, R, R|R|) staging)."""
    from mmd_amd.constraints import soft_constraints_from_paths
    starts, goals = synth.start_goal_circle(n_slots + 1, 0.8)
    paths = torch.from_numpy(synth.straight_line_paths(starts, goals, H)).cuda()
    cons = soft_constraints_from_paths(paths, 0, 2, radius=RADIUS, weight=2e-2)
    if table == "compact":
        return cons
    rng = np.random.default_rng(1000 + n_slots)
    ell = cons[0].clone().view(2, n_slots, H, 4)
    r = torch.from_numpy(rng.uniform(0.5 * RADIUS, 1.5 * RADIUS, (2, n_slots, 1)).astype(np.float32)).cuda().expand(2, n_slots, H - 1)
    ell[:, :, 1:, 2] = r
    ell[:, :, 1:, 3] = r * r.abs()                                     # (R|R|: one fp32 product, as the builders write it)
    hole = torch.from_numpy(rng.uniform(size=(2, n_slots, H)) < 0.2).cuda()
    ell[hole] = torch.tensor([0.0, 0.0, -1.0, -1.0], device="cuda")
    return (ell.view(2 * n_slots, H, 4),) + tuple(cons[1:4])


@pytest.mark.parametrize("table", ["compact", "general"])
@pytest.mark.parametrize("n_slots", SLOT_COUNTS)
def test_padded_pass_equals_the_cooperative_kernel_bitwise(n_slots, table):
    """1, 7, 8, 9, 31, 32, 33, 40 and 41 slots per robot: below, at and above a trip of eight, the headline's 31, and the 40 slots the
    general staging holds (41 general slots leave one in the L2-resident table: that group takes the general path; 41 compact slots are
    padded to 48).  The one-wave kernel pads and runs trips of eight; the cooperative kernel stages the bare table."""
    import gpu_common as gc
    model = gc.hip_model(T)
    hc = _hard_conds()
    x, nz = _inputs()
    guide = gc.hip_guide("EnvEmpty2D", [[], []], n_robots=2)
    guide.set_packed_constraints(_slot_table(n_slots, table))
    coop = _step(model, guide, x, hc, nz, 0)
    one_wave = _step(model, guide, x, hc, nz, -1)
    assert torch.isfinite(coop).all() and torch.isfinite(one_wave).all()
    diff = (_bits(coop) != _bits(one_wave)).any(-1)
    assert not diff.any(), (n_slots, table, int(diff.sum()), torch.nonzero(diff)[:4].tolist(), float((coop - one_wave).abs().max()))
    assert not torch.equal(coop, _unconstrained(model, "EnvEmpty2D", x, hc, nz))        # the slots acted


@pytest.mark.parametrize("n_slots,table", [(41, "general"), (81, "compact")])
def test_eight_wave_kernel_pads_inside_its_lds(n_slots, table):
    """2 robots x 8 samples with one slot more than the four-wave staging holds: the launch takes the eight-wave kernel, whose LDS is sized
    to the table (41 / 81 slots) rounded up to the padded 48 / 88.  Same bits as the cooperative kernel."""
    import gpu_common as gc
    model = gc.hip_model(T)
    hc = _hard_conds()
    x = torch.from_numpy(synth.synth_noise(332, (2 * 8, H, D))) * 0.5
    nz = torch.from_numpy(synth.synth_noise(333, (2 * 8, H, D)))
    guide = gc.hip_guide("EnvEmpty2D", [[], []], n_robots=2)
    guide.set_packed_constraints(_slot_table(n_slots, table))
    coop = _step(model, guide, x, hc, nz, 0)
    one_wave = _step(model, guide, x, hc, nz, -1)
    assert torch.isfinite(coop).all()
    assert _same_bits(coop, one_wave), float((coop - one_wave).abs().max())
    assert not torch.equal(coop, _step(model, gc.hip_guide("EnvEmpty2D", [[], []], n_robots=2), x, hc, nz, 0))


def test_two_groups_per_robot_equal_the_cooperative_kernel_bitwise():
    """soft (5 slots) + hard (2 points) per robot on a map with a grid: the second group starts at slot 5 of the staged table, off any trip
    boundary, and neither group is the whole table: both go through group_slots next to the padding.  Cooperative, one-wave and trace
    instantiation (every slot from L2), same bits."""
    import gpu_common as gc
    model = gc.hip_model(T)
    hc = _hard_conds()
    x, nz = _inputs()
    starts, goals = synth.start_goal_circle(6, 0.45)
    paths = synth.straight_line_paths(starts, goals, H)
    hard = cases.hard_group([[0.1, 0.2], [-0.2, 0.1]], [[20, 27], [30, 41]])
    guide = gc.hip_guide("EnvHighways2D", [[cases.soft_group(paths, r), hard] for r in range(2)], n_robots=2)
    coop = _step(model, guide, x, hc, nz, 0)
    one_wave = _step(model, guide, x, hc, nz, -1)
    traced = gc.hip_step_with_trace(model, x, hc, I, guide, T_START_GUIDE, 2, nz)[0]
    assert torch.isfinite(coop).all()
    assert _same_bits(coop, one_wave), float((coop - one_wave).abs().max())
    assert _same_bits(coop, traced), float((coop - traced).abs().max())
    assert not torch.equal(coop, _unconstrained(model, "EnvHighways2D", x, hc, nz))


class _Regridded:
    """a guide whose descriptor names one grid of the given texture instead of none"""

    def __init__(self, guide, tex):
        self.guide, self.tex = guide, tex

    def desc(self):
        d = self.guide.desc()
        d.n_grids, d.n_maps, d.grid_nx, d.grid_ny, d.sdf_grids_dev = 1, 1, self.tex.shape[2], self.tex.shape[3], self.tex.data_ptr()
        d.robot_map_dev = None
        return d


def test_map_without_grids_equals_a_grid_that_never_acts_bitwise():
    """The same trajectories and constraints on EnvEmpty2D as it is (n_grids == 0, no extra objects: the iterations skip the map term) and
    with one 8 x 8 grid whose sdf is 1 everywhere (the term is evaluated and is w_coll * 0): the same bits, in both kernels."""
    import gpu_common as gc
    model = gc.hip_model(T)
    hc = _hard_conds()
    x, nz = _inputs()
    guide = gc.hip_guide("EnvEmpty2D", [[], []], n_robots=2)
    guide.set_packed_constraints(_slot_table(31, "compact"))
    assert guide.desc().n_grids == 0 and guide.desc().n_extra_spheres + guide.desc().n_extra_boxes == 0
    tex = torch.zeros((1, 1, 8, 8, 4), device="cuda")
    tex[..., 0] = 1.0
    outs = {(name, coop_max): _step(model, g, x, hc, nz, coop_max)
            for name, g in (("no grid", guide), ("sdf = 1", _Regridded(guide, tex))) for coop_max in (0, -1)}
    first = outs[("no grid", 0)]
    assert torch.isfinite(first).all()
    for key, y in outs.items():
        assert _same_bits(y, first), (key, float((y - first).abs().max()))


# ---- rows at the edge: guide-only launches (mmd_guide_steps has no kernel switch: 2 x 4 trajectories run the cooperative kernel, the same
# ---- rows tiled to 2 x 260 the one-wave kernel), one iteration, the constraint term alone
N_FAR = 4


def _edge_case():
    """Robot 0: one group of five slots -- four that never act (points far outside the workspace, every time step) and a fifth that holds
    one planted point per time step and is empty elsewhere: a support point exactly on its constraint centre (d2 == 0), at
    fma(dx, dx, dy dy) == R|R| exactly and at the two fp32 neighbours of that value, and one well inside the radius.  Five slots: one
    trip of eight, three of them padding."""
    b = E._Batch(B, E.NEUTRAL, one_per_t=True)
    q = [np.full(2, 50.0, np.float32)] * N_FAR
    tr = [(0, H)] * N_FAR

    def add(p, qq, kind, side, dist, exact=True):
        _, t = b.plant(p, kind, side, dist, exact)
        q.append(np.asarray(qq, np.float32)); tr.append((t, t + 1))

    add(E._f32(0.25, -0.5), E._f32(0.25, -0.5), "d2_zero", 1, -float(E.R) / float(np.spacing(E.R)))
    for k in (-1, 0, 1):
        t2 = E.ulps(E.R2, k)
        dx, dy, miss = E._search_offset(1.1, lambda a, c: np.abs(E.F.fma_f32(a, a, c * c).astype(np.float64) - float(t2)))
        assert miss == 0.0
        qq = (-E._f32(dx, dy)).astype(np.float32)
        du = E.dist_ulps(E._f32(0, 0), qq)
        add(E._f32(0, 0), qq, f"d2_r2_{k:+d}", int(k <= 0), du, exact=abs(du) > E.K_BAND)
    add(E._f32(0, 0), E._f32(0.0625, 0), "inside", 1, E.dist_ulps(E._f32(0, 0), E._f32(0.0625, 0)))
    grp = O.ConstraintGroup(q=torch.from_numpy(np.stack(q)), t_range=torch.tensor(tr, dtype=torch.float32),
                            radius=torch.full((len(q),), float(E.R)), weight=1.0)
    gp = E._gp(weight_collision=0.0, weight_smoothness=0.0)
    return E.Case("padded_edges", b.x, gp, b.labels, cons=[grp], desc=dict(E.NO_BASE), term_roundings=13)


def _edge_guide(case, table):
    """robot 0 with the case's group, robot 1 with a group of ZERO slots (weight 1), in the general or the compact staging"""
    import gpu_common as gc
    from mmd_amd.constraints import pack_constraints
    cc, w = gc.to_cost_constraint(case.cons[0])
    ell, gso, gw, rgo = pack_constraints([[(cc, w)]], "cuda")
    n = ell.shape[0]
    assert n == N_FAR + 1 and gso.tolist() == [0, n]
    cons = (ell, torch.tensor([0, n, n], dtype=torch.int32, device="cuda"), torch.tensor([w, 1.0], device="cuda"),
            torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"))
    g = gc.hip_guide("EnvEmpty2D", [[], []], n_robots=2)
    g.set_packed_constraints(cons + ((float(E.R),) if table == "compact" else ()))
    return g


def _both_kernels(case, guide, x2):
    """one guide iteration on x2 [2 * 4, H, D] (robot-major) in the cooperative kernel, after asserting that the one-wave kernel returns
    the same bits on those rows of the batch tiled to 2 x 260"""
    xs = torch.from_numpy(x2).cuda()
    y = TE._steps(case, guide, xs, 2)
    xt = xs.view(2, B, H, D)[:, torch.arange(TILE, device="cuda") % B].reshape(2 * TILE, H, D)
    yt = TE._steps(case, guide, xt, 2).view(2, TILE, H, D)
    assert _same_bits(yt[:, :B].reshape(2 * B, H, D), y), "one-wave (2 x 260) differs from cooperative (2 x 4)"
    assert _same_bits(yt[:, B:2 * B], yt[:, :B])
    return y.cpu()


@pytest.mark.parametrize("table", ["general", "compact"])
def test_edge_rows_in_both_kernels_and_against_float64(table):
    """d2 == 0 (active, gradient 0), d2 == R|R| (active), the next float above (inactive), a robot whose group has no slots (nothing is
    staged or padded for it: its rows do not move, though they sit on robot 0's planted points), and a support point that is NaN / +inf:
    it comes back non-finite and the other three trajectories of its workgroup keep their bits.  Values: test_gpu_guide_edges' bound
    against the float64 oracle (a point inside the constraint band may take either of its two values)."""
    case = _edge_case()
    guide = _edge_guide(case, table)
    x2 = np.concatenate([case.x, case.x])
    y = _both_kernels(case, guide, x2)
    delta = (y - torch.from_numpy(x2)).numpy()
    assert np.all(delta[:, 0] == 0) and np.all(delta[:, H - 1] == 0)
    # the kernel's own decisions at the edge: not (d2 > R|R|) acts
    acts = E.decode_active(delta[:B])[..., 0]
    for lb in case.labels:
        want = {"d2_zero": 0, "d2_r2_-1": 1, "d2_r2_+0": 1, "d2_r2_+1": 0, "inside": 1}[lb.kind]      # (d2 == 0 acts with gradient 0)
        assert acts[lb.traj, lb.t] == want, (lb, delta[lb.traj, lb.t].tolist())
    TE._check_values(case, delta[:B], f"padded_{table}")
    assert _bits(torch.from_numpy(delta[B:])).eq(0).all(), "the robot without slots moved"       # (0 exactly, not -0)
    # a support point that is not finite
    for value, traj, t in ((np.nan, 2, 40), (np.inf, 3, 41)):
        bad = x2.copy()
        bad[traj, t] = value
        yb = _both_kernels(case, guide, bad)
        assert not torch.isfinite(yb[traj, t]).any(), (value, yb[traj, t].tolist())
        others = [k for k in range(2 * B) if k != traj]
        assert _same_bits(yb[others], y[others]), value
        assert torch.isfinite(yb[others]).all()
