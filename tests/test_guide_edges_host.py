"""Host checks of tests/guide_edge_cases.py: on the ORACLE alone, every builder holds both sides of the decision it is built around, its
labels (side and distance, computed in float64 from the fp32 operands) agree with the fp32 oracle outside the declared band, and the data that
encodes a decision decodes unambiguously -- so that no test of tests/test_gpu_guide_edges.py can pass by missing its edge.  No GPU."""
import numpy as np
import pytest
import torch

import fp32_forms as F
import guide_edge_cases as E
from oracle import mmd_oracle as O
from test_binned_host import accepted, cell_index

H = E.H


@pytest.fixture(scope="module")
def all_cases():
    return {c.name: c for c in E.single_term_cases()}


def _sets(c):
    return O.guide_decisions(torch.from_numpy(c.x), c.gp, c.cons)


def _by_kind(c):
    out = {}
    for lb in c.labels:
        out.setdefault(lb.kind, []).append(lb)
    return out


def test_builders_are_seeded_small_and_cover_the_end_rows(all_cases):
    again = {c.name: c for c in E.single_term_cases()}
    for name, c in all_cases.items():
        assert c.x.dtype == np.float32 and c.x.shape[1:] == (H, E.D) and c.x.shape[0] <= 16, name
        assert np.array_equal(c.x, again[name].x) and c.labels == again[name].labels, name
        ts = {lb.t for lb in c.labels}
        assert {1, H - 2} <= ts and not ({0, H - 1} & ts), (name, sorted(ts))
        assert len({(lb.traj, lb.t) for lb in c.labels}) == len(c.labels), name       # one label per planted point
        # rows 0 and 63 hold an ACTIVE point of the term: with the end-row zeroing taken away the oracle's gradient there is not 0
        mid = c.x.copy()                                               # (the end rows' points as rows 1 and 62, their constraints moved along)
        mid[:, 1], mid[:, H - 2] = c.x[:, 0], c.x[:, H - 1]
        cons = [O.ConstraintGroup(q=g.q, t_range=torch.where(g.t_range[:, :1] == 0, g.t_range + 1, torch.where(g.t_range[:, :1] == H - 1, g.t_range - 1, g.t_range)),
                                  radius=g.radius, weight=g.weight) for g in c.cons]
        moved = O.guide_grad(torch.from_numpy(mid), c.gp, cons, clip_mode="always", clip_rule=c.clip_rule, max_grad_value=c.max_grad_value)
        assert float(moved[:, 1].abs().max()) > 0 and float(moved[:, H - 2].abs().max()) > 0, name
        ref = c.ref32()
        assert float(ref[:, 0].abs().max()) == 0 and float(ref[:, H - 1].abs().max()) == 0, name


def test_position_exactness_of_every_planted_x(all_cases):
    """fl(fl((x + 1) / 2) * 2) - 1 == fma((x + 1) / 2, 2, -1) for every x of every builder: the un-normalised position has the same bits
    whether or not the kernel's multiply-add is contracted; and on the lattice it is x itself."""
    paths, xt, _ = E.tables_instance()
    for name, x in [(n, c.x) for n, c in all_cases.items()] + [("tables", xt), ("walk", E.walking_case().x)]:
        v = np.clip(x[..., :2], np.float32(-1), np.float32(1))
        a = ((v + np.float32(1)) / np.float32(2)).astype(np.float32)
        plain = ((a * np.float32(2)).astype(np.float32) + np.float32(-1)).astype(np.float32)
        fused = F.fma_f32(a, np.full_like(a, 2), np.full_like(a, -1))
        assert np.array_equal(plain.view(np.int32), fused.view(np.int32)), name
        assert np.array_equal(plain, E.unnorm32(x[..., :2])) and np.array_equal(plain, v), name


def test_cell_labels_against_the_fp32_oracle(all_cases):
    """The float64 side of every cell label is the fp32 oracle's cell, except where the exact (p - lo) / dim n lies within the two fp32
    roundings (the quotient, the product) of an integer: there the fp32 operation sequence IS the reference's decision, and the GPU test
    holds the kernel to it exactly (the label's side is kept for the record).  Both sides of every edge are present."""
    c = all_cases["cell"]
    cell = _sets(c).cell.numpy()
    rounding, edges = 0, {}
    for lb in c.labels:
        axis = 0 if lb.kind.endswith("_x") else 1
        got = divmod(int(cell[lb.traj, lb.t]), E.CELL_N[1])[axis]
        p = float(E.unnorm32(c.x[lb.traj, lb.t, axis]))
        _, u = E.cell_index64(p, axis)
        assert got == lb.side32, lb                                    # the builder's numpy replay of the fp32 sequence is the oracle's cell
        if lb.side32 != lb.side:
            assert abs(u - round(u)) <= 2 * E.U24 * abs(u) and abs(got - lb.side) == 1, (lb, got, u)
            rounding += 1
        if lb.kind.startswith("cell_edge"):
            assert abs(lb.ulps) <= 3.0
            edges.setdefault((axis, int(round(u))), set()).add(got)
    assert 0 < rounding <= len(c.labels) // 8                          # such points exist: they are what a reciprocal or an fma would move
    assert len(edges) == E.CELL_N[0] - 1 + E.CELL_N[1] - 1 and all(len(v) == 2 for v in edges.values())
    by = _by_kind(c)
    for a, n in (("x", E.CELL_N[0]), ("y", E.CELL_N[1])):
        assert [lb.side for lb in by[f"cell_lo_{a}"]] == [0] and [lb.side for lb in by[f"cell_hi_{a}"]] == [n - 1]
        assert {lb.side for lb in by[f"cell_clip_{a}"]} == {0, n - 1} and {lb.side for lb in by[f"cell_beyond_{a}"]} <= {0, n - 1}
    dec = E.decode_cell(c.ref32().numpy())
    assert np.array_equal(dec[..., 0] * E.CELL_N[1] + dec[..., 1], np.where(np.isin(np.arange(H), (0, H - 1))[None], 0, cell))


def test_cell_encoding_decodes_unambiguously():
    tex = E.cell_texture()
    g = tex[0, ..., 1:3].reshape(-1, 2).astype(np.float64)
    assert len(np.unique(g, axis=0)) == E.CELL_N[0] * E.CELL_N[1]
    assert np.all(np.sqrt(((g + 1e-6) ** 2).sum(1) + 2e-12) < 1)       # the clip factor is exactly 1
    assert np.array_equal(tex[0, ..., 1] * 1024, np.round(tex[0, ..., 1] * 1024))      # exact in fp32
    hinge = E.hinge_case(0.105).tex
    g = hinge[..., 1:3].reshape(-1, 2).astype(np.float64)
    assert len(np.unique(g, axis=0)) == len(g) and np.all(np.sqrt(((g + 1e-6) ** 2).sum(1) + 2e-12) < 1) and np.all(np.abs(g).max(1) > 0)


def test_real_grid_edges_hold_both_sides(all_cases):
    c = all_cases["cell_real"]
    act = _sets(c).obj_active.numpy()
    sides = [int(act[lb.traj, lb.t]) for lb in c.labels]
    for lb, side in zip(c.labels, sides):                               # float64 and fp32 pick the same cell unless the one rounding of
        assert side == lb.side32, lb                                    # (p + 1) / 2 * 400 reaches the integer: then fp32 (side32) is the
        if side != lb.side:                                             # reference, and what the device is held to
            u = (np.float64(np.abs(c.x[lb.traj, lb.t, :2])) + 1) * 200
            assert np.min(np.abs(u - np.rint(u)) / u) <= E.U24 and lb.ulps <= 0, lb
    for k in range(0, len(sides), 5):                                   # each edge: its five points take both decisions
        assert len(set(sides[k:k + 5])) == 2, k
    ref = c.ref32().numpy()
    assert all((np.abs(ref[lb.traj, lb.t]).max() > 0.5) == bool(side) for lb, side in zip(c.labels, sides))


def test_hinge_and_argmax_labels(all_cases):
    c = all_cases["hinge"]
    s = _sets(c)
    dec = E.decode_hinge(c.ref32().numpy())
    for lb in c.labels:
        active, win = bool(s.obj_active[lb.traj, lb.t]), int(s.obj_win[lb.traj, lb.t])
        if lb.kind.startswith("hinge"):
            assert active == bool(lb.side) == (lb.ulps < 0), lb        # margin - sdf > 0: sdf == margin is inactive
            assert win == (1 if lb.kind == "hinge_grid1" and active else 0), lb
        else:
            assert active and win == lb.side, lb
        assert dec[lb.traj, lb.t, 0] == int(active) and (not active or dec[lb.traj, lb.t, 2] == win), lb
        # float64 on the same fp32 table values decides the same
        cellv = [float(O.sdf_lookup(torch.from_numpy(c.x[lb.traj, lb.t, :2]), c.gp, k)[0]) for k in range(len(c.gp.sdf_grids))]
        v64 = [max(float(np.float32(c.gp.margin)) - v, 0.0) for v in cellv]
        assert (max(v64) > 0) == active and (not active or int(np.argmax(v64)) == win), lb
    kinds = _by_kind(c)
    assert {lb.side for lb in kinds["hinge"]} == {0, 1} and {lb.side for lb in kinds["hinge_grid1"]} == {0, 1}
    assert {"argmax_tie", "argmax_deeper0", "argmax_deeper1"} <= set(kinds)


def test_hinge_against_the_extra_objects(all_cases):
    """the sphere one or two ulps deeper than the cell wins, at a tie and shallower the grid does: the oracle's gradient and float64 agree"""
    c = all_cases["hinge_extra"]
    dec = E.decode_extra_win(c.ref32().numpy())
    sdf = c.gp.sdf_grids[0][0].numpy().astype(np.float64)
    for lb in c.labels:
        p = c.x[lb.traj, lb.t, :2].astype(np.float64)
        sph = c.gp.extra_spheres.numpy().astype(np.float64)
        extra = (np.hypot(*(p[None] - sph[:, :2]).T) - sph[:, 2]).min()
        cell = sdf[int((p[0] + 1) * 8), int((p[1] + 1) * 8)]
        assert (extra < cell) == bool(lb.side) == (lb.ulps > 0) and max(extra, cell) < c.gp.margin, lb
        assert dec[lb.traj, lb.t].tolist() == [1, lb.side], lb
    assert sorted({lb.ulps for lb in c.labels}) == [-2, -1, 0, 1, 2]


def test_wall_labels(all_cases):
    c = all_cases["walls"]
    s = _sets(c)
    for lb in c.labels:
        active, arg = bool(s.ws_active[lb.traj, lb.t]), int(s.ws_arg[lb.traj, lb.t])
        if lb.kind.startswith("wall_corner"):
            assert active and arg == lb.side, lb
        else:
            assert active == bool(lb.side) and (not active or arg == int(lb.kind[4])), lb
    kinds = _by_kind(c)
    for w in range(4):
        assert {lb.side for lb in kinds[f"wall{w}"]} == {0, 1} and sorted(round(lb.ulps) for lb in kinds[f"wall{w}"]) == [-1, 0, 1]
    assert sorted(lb.side for lb in kinds["wall_corner_tie"]) == [0, 0, 1, 2] and sorted(lb.side for lb in kinds["wall_corner_later"]) == [1, 2, 3, 3]
    dec = E.decode_wall(c.ref32().numpy())
    for lb in c.labels:
        assert dec[lb.traj, lb.t].tolist() == [int(s.ws_active[lb.traj, lb.t]), int(s.ws_arg[lb.traj, lb.t]) if s.ws_active[lb.traj, lb.t] else -1], lb


def test_constraint_labels_and_band_cap(all_cases):
    """Outside the band the fp32 oracle's active set is the float64 one (the label's side); inside it the label says banded; banded labels
    are at most a quarter of the constraint labels; the kernel's own fp32 test, replayed in numpy, agrees with both outside the band."""
    c = all_cases["constraint"]
    mask = _sets(c).cons[0].any(-1).numpy()
    grp = c.cons[0]
    banded = [lb for lb in c.labels if not lb.exact]
    assert 0 < len(banded) <= len(c.labels) // 4 and all(lb.kind in ("cons_general", "cons_d2", "cons_r0_denormal") and abs(lb.ulps) <= E.K_BAND for lb in banded)
    assert E.K_BAND <= 4
    tab = O.slot_table(grp)
    for lb in c.labels:
        if not lb.exact:
            continue
        assert bool(mask[lb.traj, lb.t]) == bool(lb.side), lb
        k = int(tab[:, lb.t].max())
        if lb.kind in ("cons_axis", "cons_general"):
            assert lb.kind == "cons_axis" or abs(lb.ulps) > E.K_BAND
            p, q = c.x[lb.traj, lb.t, :2], grp.q[k].numpy()
            d = p - q
            kernel = not (F.fma_f32(d[0], d[0], d[1] * d[1]) > np.float32(grp.radius[k] * abs(grp.radius[k])))
            assert kernel == bool(lb.side), lb
    kinds = _by_kind(c)
    assert sorted(round(lb.ulps) for lb in kinds["cons_axis"]) == sorted([-2, -1, 0, 1, 2] * 4)
    assert {lb.side for lb in kinds["cons_axis"] if lb.ulps == 0} == {1}                    # dist == R is active
    got = sorted(round(lb.ulps) for lb in kinds["cons_general"])
    assert got == sorted([1, -1, 2, -2, 4, -4, 8, -8, 64, -64] * 2), got
    assert [lb.side for lb in kinds["cons_range_in"]] == [1, 1] and [lb.side for lb in kinds["cons_range_end"]] == [0]
    assert [kinds[k][0].side for k in ("cons_d0", "cons_r0_d0")] == [1, 1]
    ref = c.ref32().numpy()
    for lb in c.labels:                                                # both sides show in the gradient
        if lb.exact and lb.kind in ("cons_axis", "cons_general", "cons_range_in", "cons_range_end"):
            assert int(E.decode_active(ref[lb.traj, lb.t])[0]) == lb.side, lb
    # the neutral trajectories are out of every constraint's reach
    assert int(mask.sum()) == sum(lb.side for lb in c.labels if lb.exact) + int(sum(mask[lb.traj, lb.t] for lb in banded)) + 2 * c.x.shape[0]


def test_extras_and_clip_cases_take_the_values_they_are_built_for(all_cases):
    c = all_cases["extras"]
    ref = c.ref32().numpy()
    kinds = _by_kind(c)
    clip = 1 / (1 + 1e-6)
    for lb in kinds["extra_sphere_centre"] + kinds["extra_box_dx0"][1::2]:
        assert np.all(ref[lb.traj, lb.t] == 0), lb                     # active, sub-gradient 0
    for lb in kinds["extra_two_spheres_tie"]:
        assert ref[lb.traj, lb.t, 0] > 0.5, lb                         # the FIRST sphere (to the left of the point) pushes towards +x
    for lb in kinds["extra_box_switch"]:
        assert abs(ref[lb.traj, lb.t, 0] - (0.5 if lb.ulps == 0 else clip)) < 2e-6 and ref[lb.traj, lb.t, 1] == 0, (lb, ref[lb.traj, lb.t])
    for lb in kinds["extra_box_qx_eq_qy"]:
        assert np.allclose(np.abs(ref[lb.traj, lb.t, :2]), 0.5, atol=1e-6), (lb, ref[lb.traj, lb.t])
    for lb in kinds["extra_box_dx0"][0::2]:
        assert ref[lb.traj, lb.t, 0] == 0 and ref[lb.traj, lb.t, 1] > 0.9, lb
    c = all_cases["clip_value"]
    ref = c.ref32().numpy()
    m = np.float32(c.max_grad_value)
    assert {abs(float(ref[lb.traj, lb.t, :2][np.argmin(np.abs(np.abs(ref[lb.traj, lb.t, :2]) - m))])) for lb in c.labels} == {float(m), float(E.ulps(m, -1))}
    c = all_cases["clip_norm"]
    n = np.linalg.norm(c.ref64().numpy() + 0.0, axis=-1)
    assert {lb.side for lb in c.labels} == {0, 1} and float(n.max()) <= c.gp.max_grad_norm * (1 + 1e-6)
    c = all_cases["clip_off"]
    ref = c.ref64().numpy()
    for lb in c.labels:
        assert abs(np.linalg.norm(ref[lb.traj, lb.t, :2]) - lb.ulps) < 1e-9, lb       # 40 unit vectors: 40


def test_three_tables_list_the_same_active_set_at_every_edge_point():
    """The instance of the same-bits GPU test, replayed on the host: at every planted sample point the all-pairs table's active set (the
    kernel's fp32 test of every other robot's point) equals the cell table's (the same test over the robots of the 3 x 3 cells around the
    point); planted pairs sit on both sides of the test, in table slots either side of the 40 / 60 / 80 slots a kernel stages."""
    paths, x, labels = E.tables_instance()
    assert paths.shape == (E.TABLES_N_ALL, H, 2) and x.shape == (2 * E.TABLES_B, H, E.D) and E.TABLES_N_ALL - 1 > 80
    cp = cell_index(paths)
    sides, slots = {}, set()
    for lb in labels:
        self_id = lb.traj // E.TABLES_B
        p, j = x[lb.traj, lb.t, :2], lb.carrier
        others = np.array([r for r in range(E.TABLES_N_ALL) if r != self_id])
        dense = others[accepted(p[None], paths[others, lb.t])]
        near = (np.abs(cp[others, lb.t] - cell_index(p)[None]) <= 1).all(1)
        binned = others[near & accepted(p[None], paths[others, lb.t])]
        assert dense.tolist() == binned.tolist(), lb
        on = j in dense.tolist()
        sides.setdefault(lb.kind, set()).add(on)
        slots.add(j - (j > self_id))
        assert lb.exact == (lb.kind != "tables_d2") and lb.side == int(lb.ulps <= 0)
        if lb.exact:                                                   # along an axis the kernel's fp32 test is the float64 decision
            assert on == bool(lb.side), lb
        if lb.kind == "tables_bin_edge":
            assert abs(int(cp[j, lb.t, 0]) - int(cell_index(p)[0])) <= 1 and int(cp[j, lb.t, 0]) == 7
    assert all(v == {True, False} for v in sides.values()), sides
    assert accepted(x[:, H - 1, :2], paths[10, H - 1][None]).all()                 # row 63 is active in every trajectory
    assert {int(cell_index(x[lb.traj, lb.t, :2])[0]) for lb in labels if lb.kind == "tables_bin_edge"} == {7, 8}
    assert min(slots) < 40 and any(60 <= s < 80 for s in slots) and max(slots) >= 80
    # fma(dx, dx, dy dy) == R|R| and its neighbours are met exactly: a table whose R|R| is one ulp off decides one of them differently
    d2 = set()
    for lb in labels:
        if lb.kind == "tables_d2":
            d = x[lb.traj, lb.t, :2] - paths[lb.carrier, lb.t]
            d2.add(float(F.fma_f32(d[0], d[0], d[1] * d[1])))
    assert d2 == {float(E.ulps(E.R2, k)) for k in (-1, 0, 1)}
