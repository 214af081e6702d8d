"""CPU: the host side of the cell-binned inter-robot constraint table (include/mmd_amd.h: mmd_cons_bins) -- the default grid, the cover
property the binned guided step rests on, and the error paths that are decided before any launch.

Cover property: the step kernel accepts a table point q at a lane's point p iff fma(dx, dx, dy * dy) <= R|R| in fp32 (cons_term,
csrc/guide.hip), and the lane reads only the list of its own cell, which holds the points of the 3 x 3 cells around it.  So every
accepted pair must have cell indices at most 1 apart on both axes.  The cell index is mirrored here in numpy fp32, operation for operation
(bin_cell: floor((p - lo) * inv_cell) clamped to [0, n - 1]; inv_cell the fp32 quotient n / (hi - lo))."""
import ctypes as C

import numpy as np
import pytest

import fp32_forms as F
from mmd_amd import _lib
from mmd_amd import constraints as K
from mmd_amd.environments import LIMITS

R = np.float32(K.VERTEX_CONSTRAINT_RADIUS)
R2 = np.float32(R * np.abs(R))


def cell_index(p, limits=LIMITS, grid=(15, 15)):
    """numpy fp32 mirror of bin_cell on float32 points [..., 2] -> int [..., 2]"""
    p = np.asarray(p, np.float32)
    out = np.empty(p.shape, np.int64)
    for k in range(2):
        lo, hi, n = np.float32(limits[0][k]), np.float32(limits[1][k]), np.float32(grid[k])
        inv = np.float32(n / (hi - lo))
        u = np.floor((p[..., k] - lo) * inv)
        out[..., k] = np.clip(u, np.float32(0), n - np.float32(1)).astype(np.int64)
    return out


def accepted(p, q):
    """the kernel's fp32 test of one slot: not (fma(dx, dx, dy * dy) > R|R|)"""
    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)
    return ~(F.fma_f32(d[..., 0], d[..., 0], d[..., 1] * d[..., 1]) > R2)


def ulps(v, k):
    v = np.asarray(v, np.float32).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def planted_pairs():
    """pairs at the acceptance boundary around anchors where the cell index is most exposed: cell edges, points outside the limits, the
    four corners; q at distance R (1 + a few ulp either way) from p along the axes and the diagonals, each coordinate also moved by ulps"""
    cell = 2.0 / 15
    edges = np.float32(-1.0) + np.arange(16, dtype=np.float32) * np.float32(cell)
    anchors = [(x, y) for x in edges for y in (edges[0], edges[7], edges[15])] + [(y, x) for x in edges for y in (edges[3], edges[8])]
    anchors += [(ulps(x, s), ulps(x, -s)) for x in edges for s in (1, 2)]
    anchors += [(1.3, -1.2), (-1.3, 1.2), (1.3, 1.3), (-1.25, -1.05), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (0.0, 0.0)]
    a = np.array(anchors, np.float32)
    dirs = np.array([(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0)], np.float64)
    dirs[4:8] /= np.sqrt(2.0)
    ps, qs = [], []
    for rel in (-3e-7, -1.2e-7, -6e-8, 0.0, 6e-8, 1.2e-7, 3e-7):
        off = (dirs * float(R) * (1 + rel)).astype(np.float64)
        for k in (-2, -1, 0, 1, 2):
            q = ulps((a[:, None, :].astype(np.float64) + off[None]).astype(np.float32), k)
            ps.append(np.broadcast_to(a[:, None, :], q.shape).reshape(-1, 2))
            qs.append(q.reshape(-1, 2))
    return np.concatenate(ps), np.concatenate(qs)


def test_bin_grid_default_and_too_small_cells():
    assert K.bin_grid(LIMITS, K.VERTEX_CONSTRAINT_RADIUS) == (15, 15)
    assert K.bin_grid(((-1, -1), (1, 3)), 0.12) == (15, 31)
    assert K.bin_grid(((-10, -10), (10, 10)), 0.12) == (32, 32)                   # capped
    assert K.bin_grid(((0, 0), (0.1275, 1)), 0.12)[0] == 1                        # exactly (1 + 1/16) R
    with pytest.raises(ValueError):
        K.bin_grid(((0, 0), (0.127, 1)), 0.12)                                    # not even one cell of 1.0625 R
    with pytest.raises(ValueError):
        K.bin_grid(LIMITS, 0.0)
    K.check_bin_grid(LIMITS, 0.12, (15, 15))
    with pytest.raises(ValueError):
        K.check_bin_grid(LIMITS, 0.12, (16, 15))                                  # 0.125 < 0.1275
    with pytest.raises(ValueError):
        K.check_bin_grid(LIMITS, 0.12, (15, 0))


def test_accepted_pairs_are_in_neighbouring_cells():
    rng = np.random.default_rng(20)
    n = 100_000
    c = rng.uniform(-1.4, 1.4, (n, 2))
    phi = rng.uniform(0, 2 * np.pi, n)
    r = float(R) * rng.uniform(0.0, 1.2, n)
    d = np.stack([np.cos(phi), np.sin(phi)], 1) * r[:, None]
    p, q = (c + d / 2).astype(np.float32), (c - d / 2).astype(np.float32)
    mp, mq = F.margin_pairs(21, 20_000, margin=R)                                 # |p - q| = R (1 +- 4e-7): both sides of the test
    pp, pq = planted_pairs()
    for name, a, b in (("random", p, q), ("margin", mp, mq), ("planted", pp, pq)):
        acc = accepted(a, b)
        n_acc, n_rej = int(acc.sum()), int((~acc).sum())
        assert n_acc > len(a) // 10 and n_rej > len(a) // 20, (name, n_acc, n_rej)            # the cases sit on both sides
        ca, cb = cell_index(a), cell_index(b)
        assert ca.min() >= 0 and ca.max() <= 14
        worst = np.abs(ca - cb)[acc].max()
        assert worst <= 1, (name, worst, a[acc][np.abs(ca - cb)[acc].max(1) > 1][:4], b[acc][np.abs(ca - cb)[acc].max(1) > 1][:4])
    # the property is not vacuous: with cells narrower than the radius, accepted pairs do skip a cell
    ca, cb = cell_index(p, grid=(32, 32)), cell_index(q, grid=(32, 32))
    assert np.abs(ca - cb)[accepted(p, q)].max() >= 2
    # points outside the limits land in the border cells
    assert cell_index(np.array([[1.3, -1.2], [-5.0, 7.0]], np.float32)).tolist() == [[14, 0], [0, 14]]


def _bins(**kw):
    b = _lib.ConsBins()
    b.lo[:] = [-1.0, -1.0]
    b.inv_cell[:] = [7.5, 7.5]
    b.nx, b.ny, b.n_all, b.robot0 = 15, 15, 4, 0
    b.radius, b.weight = 0.12, 2e-2
    b.cell_off_dev, b.entries_dev = 0x1000, 0x1000          # never read on the host
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    lo, hi = (C.c_float * 2)(-1, -1), (C.c_float * 2)(1, 1)
    fake = 0x1000                                            # a non-NULL "device pointer": every call below returns before its launch
    good = dict(paths=fake, n_all=5, horizon=64, radius=0.12, lo=lo, hi=hi, nx=15, ny=15, off=fake, ent=fake)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.mmd_bin_constraints_from_paths(a["paths"], a["n_all"], a["horizon"], a["radius"], a["lo"], a["hi"], a["nx"], a["ny"],
                                                a["off"], a["ent"], None)
        return rc, lib.mmd_last_error().decode()

    for kw, text in (({"paths": None}, "NULL"), ({"off": None}, "NULL"), ({"ent": None}, "NULL"), ({"lo": None}, "NULL"),
                     ({"n_all": 1}, "n_all"), ({"n_all": 0}, "n_all"), ({"radius": 0.0}, "radius"), ({"radius": -0.1}, "radius"),
                     ({"nx": 16}, "cells smaller"), ({"ny": 16}, "cells smaller"), ({"radius": 0.126}, "cells smaller"),
                     ({"nx": 0}, "grid"), ({"horizon": 32}, "horizon")):
        rc, err = call(**kw)
        assert rc != 0 and text in err, (kw, rc, err)
    ob, eb = C.c_size_t(), C.c_size_t()
    assert lib.mmd_cons_bins_bytes(300, 15, 15, C.byref(ob), C.byref(eb)) == ob.value + eb.value
    assert (ob.value, eb.value) == (64 * 226 * 4, 64 * 9 * 300 * 16)

    # mmd_guide_steps: a cell table together with ELL groups, and a malformed table
    d = _lib.GuideDesc()
    d.clip_grad_rule = 0
    for bins, ell, text in ((_bins(), fake, "ELL"), (_bins(radius=0.0), None, "radius"), (_bins(inv_cell=(C.c_float * 2)(8.0, 7.5)), None, "cells smaller"),
                            (_bins(cell_off_dev=None), None, "NULL"), (_bins(robot0=4), None, "robot")):
        d.cons_bins = C.pointer(bins)
        d.cons_ell_dev = ell
        rc = lib.mmd_guide_steps(C.byref(d), fake, fake, 0, 2, 2, 1, None, None)
        assert rc != 0 and text in lib.mmd_last_error().decode(), (text, rc, lib.mmd_last_error())


def test_host_layer_has_the_binned_path():
    from mmd_amd.guides import GuideManagerTrajectoriesWithVelocity as G
    from mmd_amd.multi_robot import MultiRobotSampler
    import inspect
    import torch
    import mmd_amd.ops  # noqa: F401
    assert callable(G.set_binned_constraints)
    assert inspect.signature(MultiRobotSampler.__init__).parameters["constraint_table"].default == "dense"
    off, ent = torch.ops.mmd_amd.bin_constraints_from_paths(torch.zeros(5, 64, 2, device="meta"), 0.12, -1.0, -1.0, 1.0, 1.0, 15, 15)
    assert off.shape == (64, 226) and off.dtype == torch.int32 and ent.shape == (64, 45, 4)
    assert C.sizeof(_lib.ConsBins) == 56 and _lib.GuideDesc.cons_bins.offset % 8 == 0


def test_numpy_model_of_the_list_sum_has_the_dense_sum_bits():
    """The argument the GPU test rests on, replayed in numpy fp32: the dense slot sum (four interleaved fma chains over all N - 1 slots,
    a slot that does not act contributing fma(-d, 0, a)) and the sum over the lane's cell list (ascending robot id, own robot skipped,
    entry -> chain rel & 3) are the same bits, for lanes near the other robots' points, at the top and bottom robot ids."""
    rng = np.random.default_rng(22)
    n, lanes = 48, 4000
    q = rng.uniform(-1.1, 1.1, (n, 2)).astype(np.float32)                          # the robots' points at one time step
    q[7] = q[8]                                                                    # coincident robots
    near = F.near_points(rng, q[rng.integers(0, n, lanes)], float(R) * rng.uniform(0.0, 1.3, lanes), rel=0.0)
    p = np.clip(near, -1.08, 1.08).astype(np.float32)                              # lanes: within the normaliser's limits
    p[:50] = q[rng.integers(0, n, 50)]                                             # d = 0
    cq, cp = cell_index(q), cell_index(p)
    zero = np.float32(0)

    def term(a, pp, qq, on):
        dx, dy = pp[:, 0] - qq[0], pp[:, 1] - qq[1]
        d2 = F.fma_f32(dx, dx, dy * dy)
        m = np.where((d2 > R2) | ~on, zero, np.float32(1) / np.sqrt(np.maximum(d2, np.float32(1e-30))))
        return np.stack([F.fma_f32(-dx, m, a[:, 0]), F.fma_f32(-dy, m, a[:, 1])], 1), (~(d2 > R2)) & on

    for self_id in (0, 1, 46, 47):
        dense = np.zeros((4, lanes, 2), np.float32)
        acting = np.zeros(lanes, np.int64)
        for rel in range(n - 1):
            other = rel + (1 if rel >= self_id else 0)
            dense[rel & 3], act = term(dense[rel & 3], p, q[other], np.ones(lanes, bool))
            acting += act
        binned = np.zeros((4, lanes, 2), np.float32)
        for rid in range(n):                                                       # a lane's list: the robots within one cell, ascending
            in_list = (np.abs(cq[rid] - cp) <= 1).all(1) & (rid != self_id)
            k = (rid - (1 if rid > self_id else 0)) & 3
            binned[k], _ = term(binned[k], p, q[rid], in_list)
        assert acting.max() >= 3 and (acting == 0).sum() > 0
        tot = lambda a: (a[0] + a[1]) + (a[2] + a[3])                              # noqa: E731
        assert np.array_equal(tot(dense).view(np.int32), tot(binned).view(np.int32)), self_id
        assert np.array_equal(dense.view(np.int32), binned.view(np.int32)), self_id
