"""-m gpu: every discrete decision of guide_grad (mmd_amd/csrc/guide.hip) at its edge, on the inputs of tests/guide_edge_cases.py (whose both
sides tests/test_guide_edges_host.py asserts on the oracle alone).  One guide iteration through mmd_guide_steps, hard_rows = 0, in the launch
shapes the product uses.  The cell index, the hinge, the winning grid, the wall and its arg max, the constraint's active set outside the band
and the zeroed rows 0 / 63 must EQUAL the fp32 oracle's -- read back from y - x, no attributed flip; the values are held against float64 to a
bound derived from fp32 rounding; the launch shapes and the three constraint tables must return the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guide_edge_cases as E             # noqa: E402
import parity_log                        # noqa: E402
from oracle import mmd_oracle as O       # noqa: E402

H, D = E.H, E.D
TILE = 320                               # 2 robots x 320 = 640 trajectories: past the cooperative kernel's 512
_CASES = {}


def _case(name):
    if not _CASES:
        _CASES.update({c.name: c for c in E.single_term_cases()})
    return _CASES[name]


def _guide(case, n_robots, binned=False):
    """the case's guide for n_robots robots with the same constraint groups each; binned: instead of the groups a cell table of three
    robots whose paths stay at the far group's point (the case's only group must be that one), so the step runs the binned kernel"""
    import gpu_common as gc
    from mmd_amd.constraints import binned_constraints_from_paths
    from mmd_amd.guides import GuideManagerTrajectoriesWithVelocity
    g = GuideManagerTrajectoriesWithVelocity(gc.dataset(), env_id=case.env, n_robots=n_robots, device="cuda", clip_grad=case.clip_rule is not None,
                                             clip_grad_rule=case.clip_rule or "norm", max_grad_value=case.max_grad_value,
                                             extra_objects=case.extra_objects)
    if binned:
        assert len(case.cons) == 1 and float(case.cons[0].q.min()) == 50.0
        far = torch.full((3, H, 2), 50.0, device="cuda")
        g.set_binned_constraints(binned_constraints_from_paths(far, 0, n_robots, radius=float(E.R), weight=1.0))
        return g
    for r in range(n_robots):
        pairs = [gc.to_cost_constraint(grp) for grp in case.cons]
        g.add_extra_costs([p[0] for p in pairs], [p[1] for p in pairs], robot=r)
    return g


def _steps(case, guide, x, n_robots, n_steps=1, chain=None):
    """x after n_steps guide iterations (hard_rows = 0) with the case's descriptor patch: one cost term, the synthetic texture"""
    from mmd_amd import _lib
    d = guide.desc()
    for k, v in case.desc.items():
        if isinstance(v, (list, tuple)):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    tex = None
    if case.tex is not None:
        tex = torch.from_numpy(np.ascontiguousarray(case.tex[None])).cuda()          # [n_maps = 1, n_grids, nx, ny, 4]
        d.n_grids, d.n_maps, d.grid_nx, d.grid_ny, d.sdf_grids_dev = tex.shape[1], 1, tex.shape[2], tex.shape[3], tex.data_ptr()
    y = x.contiguous().clone()
    assert y.shape[0] % n_robots == 0 and y.shape[1:] == (H, D)
    hard = torch.zeros(n_robots, 2, D, device="cuda")
    _lib.check(_lib.load().mmd_guide_steps(C.byref(d), y.data_ptr(), hard.data_ptr(), 0, n_robots, y.shape[0] // n_robots, n_steps,
                                           chain.data_ptr() if chain is not None else None, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    del tex
    return y


def _all_kernels(case):
    """y - x of the batch as it is, one robot with <= 16 trajectories: the cooperative kernel (every case carries guide_edge_cases.far_group,
    41 slots that never act, so the robot has a constraint table) -- after asserting that the same bits come back from the batch tiled to
    2 robots x 320 (the 8-wave kernel: more than 40 slots, samples a multiple of 8), to 2 x 324 (the 4-wave kernel, 40 slots staged in LDS,
    the rest from L2) and, where the far group is the case's only one, from the binned kernel on a cell table that never acts, at both sizes"""
    x = torch.from_numpy(case.x).cuda()
    B = x.shape[0]
    assert B <= 16 and sum(g.q.shape[0] for g in case.cons) > 40
    y1 = _steps(case, _guide(case, 1), x, 1)
    forms = [(TILE, False), (TILE + 4, False)] + ([(B, True), (TILE, True)] if len(case.cons) == 1 else [])
    for tile, binned in forms:
        n_robots = 1 if tile == B else 2
        xt = x[torch.arange(tile, device="cuda") % B].repeat(n_robots, 1, 1)
        yt = _steps(case, _guide(case, n_robots, binned), xt, n_robots).view(n_robots, tile, H, D)
        for r in range(n_robots):
            diff = (yt[r, :B] != y1).any(-1)
            assert not diff.any(), (case.name, f"{n_robots} x {tile}" + (" binned" if binned else ""), r, torch.nonzero(diff)[:4].tolist())
        assert tile == B or torch.equal(yt[:, B:2 * B], yt[:, :B])
    return (y1 - x).cpu().numpy()


def _banded_candidates(case, lb):
    """the two float64 values a banded constraint point may take: 0, or its clipped unit vector"""
    grp = case.cons[0]
    k = int(O.slot_table(grp)[:, lb.t].max())
    d = case.x[lb.traj, lb.t, :2].astype(np.float64) - grp.q[k].numpy().astype(np.float64)
    n = np.hypot(d[0], d[1])
    u = np.zeros(D)
    if n > 0:
        u[:2] = d / n
    u *= min(1.0, case.gp.max_grad_norm / np.linalg.norm(-u + 1e-6))         # (the term's gradient is -u: the clip sees -u + 1e-6)
    return np.zeros(D), u


def _check_values(case, delta, tag):
    """|(y - x) - float64 reference| <= the derived bound (guide_edge_cases.value_bound), or twice the fp32 oracle's own error against the same
    reference where that is larger; a banded point may take either of its two float64 values.  Both errors go to the parity log."""
    ref64 = case.ref64()
    bound = E.value_bound(case, ref64)
    ref64 = ref64.numpy()
    err = np.abs(delta.astype(np.float64) - ref64)
    err_o = np.abs(case.ref32().numpy().astype(np.float64) - ref64)
    for lb in case.labels:
        if not lb.exact:                                               # either decision: the nearer of the two values
            cands = _banded_candidates(case, lb)
            err[lb.traj, lb.t] = min((np.abs(delta[lb.traj, lb.t] - c) for c in cands), key=np.max)
            err_o[lb.traj, lb.t] = 0
            bound[lb.traj, lb.t] = E.U24 * (np.abs(case.x[lb.traj, lb.t]) + 2) + case.term_roundings * E.U24       # value_bound at |g| = 1
    tol = np.maximum(bound, 2 * float(err_o.max()))
    worst = float((err / np.maximum(tol, 1e-300)).max())
    parity_log.record(f"guide_edges/{tag}", "kernel_vs_float64", None, float(err.max()), bound=float(tol[np.unravel_index(np.argmax(err), err.shape)]),
                      oracle_fp32_err=float(err_o.max()), worst_err_over_bound=worst, note="max abs over the batch")
    print(f"guide_edges/{tag}: kernel {err.max():.3e} oracle fp32 {err_o.max():.3e} (max abs against float64), worst error / bound {worst:.3f}")
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, (tag, f"{len(bad)} values beyond the bound, first (traj, t, dim): {bad[:4].tolist()}",
                           [(float(err[tuple(i)]), float(tol[tuple(i)])) for i in bad[:4]])


def _check_decisions(case, delta, decode, tag):
    """the decision decoded from the kernel's y - x equals the one decoded from the fp32 oracle's gradient at every exact label"""
    got, want = decode(delta), decode(case.ref32().numpy())
    bad = [(lb, got[lb.traj, lb.t].tolist(), want[lb.traj, lb.t].tolist()) for lb in case.labels
           if lb.exact and not np.array_equal(got[lb.traj, lb.t], want[lb.traj, lb.t])]
    assert not bad, f"{tag}: {len(bad)} of {len(case.labels)} decisions differ from the fp32 oracle's (label, kernel, oracle): {bad[:6]}"
    assert np.all(delta[:, 0] == 0) and np.all(delta[:, H - 1] == 0), f"{tag}: rows 0 / 63 hold an active point and must come back exactly 0"
    # cell kinds: also the fp32 operation sequence replayed by the builder (the label's side32), which is the oracle's by the host test
    for lb in case.labels:
        if lb.side32 is not None:
            k = got[lb.traj, lb.t]
            mine = int(k[0 if lb.kind.endswith("_x") else 1]) if tag == "cell" else int(k[0])
            assert mine == lb.side32, f"{tag}: {lb} decoded {k.tolist()}"


@pytest.mark.parametrize("name,decoder", [("cell", E.decode_cell), ("cell_real", E.decode_active), ("hinge", E.decode_hinge),
                                          ("hinge_extra", E.decode_extra_win), ("walls", E.decode_wall), ("constraint", E.decode_active)])
def test_decisions_equal_the_fp32_oracle_at_the_edge(name, decoder):
    """SDF cell index on a 24 x 40 grid over [-1, 0.5] x [-0.75, 1] (every interior edge at 0, +-1, +-2 lattice steps, lo, hi, the clip at
    +-1, beyond the limits) and on the real 400 x 400 grid; hinge on / off at margin, margin +- 1, 2 ulps, the first-maximum rule over two
    grids and against an extra sphere one ulp deeper or shallower than the cell; the four walls at 0, +-1 steps, the corner ties and the later wall one step deeper; the constraint radius along the axes at R,
    R +- 1, 2 ulps (exact), at k ulps of R in general directions (exact beyond the band K = 2 ulps, either value inside), R = 0, d = 0 and
    the exclusive end of a time range.  Every kernel (_all_kernels), same bits."""
    case = _case(name)
    delta = _all_kernels(case)
    _check_decisions(case, delta, decoder, name)
    _check_values(case, delta, name)


@pytest.mark.parametrize("name", ["extras", "clip_value", "clip_norm", "clip_off"])
def test_values_at_the_ties_and_clip_thresholds(name):
    """extra_sdf<false> at its ties (sphere centre, two spheres at equal distance, max q == 0 and +-1 step, qx == qy, dx == 0) against
    O.extra_objects_sdf's autograd; clip by value with a component at max_grad_value +- 1 ulp; clip by norm with ||g + 1e-6|| at max_norm
    +- 1, 2 ulps (the 1-ulp v_rsq_f32 stays inside the bound); clip off on a sum of 40 coincident unit vectors (40, not 1)."""
    case = _case(name)
    delta = _all_kernels(case)
    assert np.all(delta[:, 0] == 0) and np.all(delta[:, H - 1] == 0), name
    _check_values(case, delta, name)
    if name == "clip_off":
        for lb in case.labels:
            assert abs(np.linalg.norm(delta[lb.traj, lb.t, :2]) - 40.0) < 1e-4, lb


def _tables_candidates(x, paths, lb):
    """the two float64 values of a sample point of the tables instance: its clipped slot sum with the planted carrier's point acting or not"""
    self_id = lb.traj // E.TABLES_B
    others = np.array([j for j in range(paths.shape[0]) if j != self_id])
    d = (x[lb.traj, lb.t, :2][None] - paths[others, lb.t]).astype(np.float64)          # the fp32 differences both sides compute
    dist = np.hypot(d[:, 0], d[:, 1])
    out = []
    for carrier_acts in (True, False):
        act = np.where(others == lb.carrier, carrier_acts, dist <= float(E.R)) & (dist > 0)
        u = np.zeros(D)
        u[:2] = (d[act] / dist[act, None]).sum(0)
        out.append(u * min(1.0, 1.0 / np.linalg.norm(-u + 1e-6)))
    return out


def test_three_tables_and_three_kernels_return_the_same_bits():
    """One instance -- 2 local robots x 8 samples among 90 robots, other robots' path points planted at a sample point's radius (along an axis
    at R, R +- 1 ulp; at fma(dx, dx, dy dy) == R|R| and its two fp32 neighbours; across a cell-table edge) in slots either side of what a
    kernel stages in LDS -- as soft_constraints_from_paths with the uniform radius (compact staging, R|R| from the host), the same table
    without it (general staging, R|R| from the table's slot word) and binned_constraints_from_paths; each as 2 x 8 (cooperative kernel),
    2 x 320 (8-wave kernel) and 2 x 324 (4-wave kernel: 89 slots overflow its 80 compact / 40 general LDS slots).  All nine results are
    bit-identical on the shared trajectories, and agree with the oracle on the all-pairs groups."""
    import gpu_common as gc
    from mmd_amd.constraints import binned_constraints_from_paths, soft_constraints_from_paths
    paths, x, labels = E.tables_instance()
    p = torch.from_numpy(paths).cuda()
    B, radius = E.TABLES_B, float(E.R)
    case = E.Case("tables", x, E._gp(weight_collision=0.0, weight_smoothness=0.0), labels, desc=dict(E.NO_BASE))
    dense = soft_constraints_from_paths(p, 0, 2, radius=radius, weight=1.0)
    out = {}
    for table in ("compact", "general", "binned"):
        g = gc.hip_guide("EnvEmpty2D", [[], []], n_robots=2)
        if table == "binned":
            g.set_binned_constraints(binned_constraints_from_paths(p, 0, 2, radius=radius, weight=1.0))
        else:
            g.set_packed_constraints(dense if table == "compact" else dense[:4])
        for spr in (B, 320, 324):
            xs = torch.from_numpy(x).cuda().view(2, B, H, D)[:, torch.arange(spr, device="cuda") % B].reshape(2 * spr, H, D)
            y = _steps(case, g, xs, 2).view(2, spr, H, D)
            assert torch.equal(y[:, B:2 * B], y[:, :B]) or spr == B
            out[(table, spr)] = y[:, :B].reshape(2 * B, H, D).cpu()
    first = out[("compact", B)]
    assert torch.isfinite(first).all()
    for key, y in out.items():
        diff = (y != first).any(-1)
        where = [(lb.kind, lb.traj, lb.t) for lb in labels if diff[lb.traj, lb.t]]
        assert not diff.any(), f"{key} differs from ('compact', {B}) at {int(diff.sum())} points; planted ones among them: {where[:6]}"
    delta = (first - torch.from_numpy(x)).numpy()
    assert np.all(delta[:, 0] == 0) and np.all(delta[:, H - 1] == 0)
    # values: per robot the oracle on the all-pairs group.  A sum of up to n acting unit vectors: T = 13 each and n u for the fma chain.
    err, err_o, n_act = [], [], 0
    for r in range(2):
        grp = O.soft_constraints_from_paths(torch.from_numpy(paths), r, radius, 1.0)
        xr = torch.from_numpy(x[r * B:(r + 1) * B])
        ref64 = O.guide_grad(xr.double(), case.gp, [grp], clip_mode="always").numpy()
        ref32 = O.guide_grad(xr, case.gp, [grp], clip_mode="always").numpy()
        n_act = max(n_act, int(O.guide_decisions(xr, case.gp, [grp]).cons[0].sum(-1).max()))
        e, eo = np.abs(delta[r * B:(r + 1) * B] - ref64), np.abs(ref32 - ref64)
        for lb in labels:                                              # planted points inside the band: either of the two float64 values
            if not lb.exact and lb.traj // B == r:
                e[lb.traj - r * B, lb.t] = min((np.abs(delta[lb.traj, lb.t] - c) for c in _tables_candidates(x, paths, lb)), key=np.max)
                eo[lb.traj - r * B, lb.t] = 0
        err.append(e)
        err_o.append(eo)
    worst = np.unravel_index(np.argmax(np.concatenate(err)), (2 * B, H, D))
    at = [lb for lb in labels if (lb.traj, lb.t) == worst[:2]] or "no planted point"
    err, err_o = float(np.max(err)), float(np.max(err_o))
    tol = max(2 * err_o, E.U24 * (1 + 2 * n_act) + 14 * n_act * E.U24)
    parity_log.record("guide_edges/tables", "kernel_vs_float64", None, err, bound=tol, oracle_fp32_err=err_o, note="max abs")
    print(f"guide_edges/tables: kernel {err:.3e} oracle fp32 {err_o:.3e} (max abs against float64), bound {tol:.3e}, up to {n_act} acting slots")
    assert 2 <= n_act <= 12 and err <= tol, (err, err_o, tol, n_act, f"worst at (traj, t, dim) {worst}: {at}, y - x = {delta[worst[:2]].tolist()}")


def test_twenty_iterations_walk_across_cell_edges():
    """One 20-iteration mmd_guide_steps call on the cell-encoding grid with chain=: row k equals k single launches, bitwise, and -- every
    operation of this term being exact but the one rounding of x + g -- the fp32 oracle's k-th iterate, bitwise; the points start next to
    cell edges and cross them mid-chain, so the cell changes between iterations."""
    case = E.walking_case()
    g = _guide(case, 1)
    x = torch.from_numpy(case.x).cuda()
    n = 20
    chain = torch.empty((n,) + tuple(x.shape), device="cuda")
    y = _steps(case, g, x, 1, n_steps=n, chain=chain)
    assert torch.equal(chain[-1], y)
    z, ref, cells = x.clone(), torch.from_numpy(case.x), []
    for k in range(n):
        z = _steps(case, g, z, 1)
        assert torch.equal(chain[k], z), k
        step = O.guide_grad(ref, case.gp, [], clip_mode="always")
        cells.append(E.decode_cell(step.numpy()))
        ref = ref + step
        bad = (chain[k].cpu() != ref).any(-1)
        assert not bad.any(), (k, torch.nonzero(bad)[:4].tolist(), E.decode_cell((chain[k].cpu() - (ref - step)).numpy())[bad.numpy()][:4].tolist(),
                               cells[-1][bad.numpy()][:4].tolist())
    cells = np.stack(cells)                                            # [n, B, H, 2]
    changes = [int((np.diff(cells[:, lb.traj, lb.t], axis=0) != 0).any(1).sum()) for lb in case.labels]
    assert min(changes) >= 1 and max(changes) >= 3, changes           # every planted point changes its cell mid-chain
