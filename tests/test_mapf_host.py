"""CPU: golden g23 (the reference's CBS / ECBS / XECBS / PrioritizedPlanning driven by the scripted planner of mapf_stub) pinned by a NumPy
restatement of get_conflicts and of the soft-constraint builder, and the pure-host pieces of mmd_amd.multi_agent_planners against it."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import fp32_forms as F
import mapf_stub as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_mapf.npz")
MARGIN = np.float32(2.1 * 0.05)


@pytest.fixture(scope="module")
def g23():
    return np.load(GOLDEN)


def _case(g, name):
    for c in st.CASES:
        if c[0] == name:
            _, kind, flags, n, lengths, stagger, fail_at = c
            seed = int(g[name + ".meta"][4])
            return kind, flags, n, lengths, [stagger * k for k in range(n)], st.make_script(n, lengths, fail_at, seed)
    raise KeyError(name)


def np_conflicts(paths, lengths, starts, ordered):
    """get_conflicts restated: global padding by clamping, ||pa - pb|| < 2.1 r in torch.norm's fp32 form, (pa + pb) / 2; (t, a, b)
    row-major, a != b (CBS, PointConflict) or a < b (PP, VertexConflict)."""
    n = len(paths)
    Tg = max(L + s for L, s in zip(lengths, starts))
    pos = np.stack([paths[k][np.clip(np.arange(Tg) - starts[k], 0, lengths[k] - 1), :2] for k in range(n)])      # [n, Tg, 2]
    rows = []
    for t in range(Tg):
        for a in range(n):
            for b in range(n):
                if (a == b) or (not ordered and b < a):
                    continue
                pa, pb = pos[a, t], pos[b, t]
                if F.pos_norm(pa, pb) < MARGIN:
                    mid = (pa + pb) / np.float32(2) if ordered else np.zeros(2, np.float32)
                    rows.append([t, a, b, *pa, *pb, *mid])
    return np.array(rows, np.float32).reshape(-1, 9)


def np_soft_points(paths, lengths, starts, agent, n_state):
    """create_soft_constraints_from_other_agents_paths restated (cbs.py:468-508)."""
    rows = []
    for j in range(n_state):
        if j == agent:
            continue
        last = lengths[agent] - 1 if agent < n_state else lengths[j] - 1
        for tj in range(lengths[j]):
            ti = tj + starts[j] - starts[agent]
            if 1 <= ti <= last:
                rows.append([*paths[j][tj, :2], ti, ti + 1, np.float32(0.05 * 2.4)])
    return np.array(rows, np.float32).reshape(-1, 5)


@pytest.mark.parametrize("name", [c[0] for c in st.CASES])
def test_g23_script_and_conflicts_restated(g23, name):
    kind, _, n, lengths, starts, script = _case(g23, name)
    sums = [float(np.sum(script[k][e][0], dtype=np.float64)) for k in range(n) for e in range(st.N_ENTRIES)]
    np.testing.assert_array_equal(sums, g23[name + ".script_sum"])
    for si in range(3):
        ix = g23[f"{name}.state{si}_ix"]
        paths = [script[k][si % st.N_ENTRIES][0][ix[k]] for k in range(n)]
        got = np_conflicts(paths, lengths, starts, ordered=kind == "CBS")
        want = g23[f"{name}.state{si}_conflicts"]
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", [c[0] for c in st.CASES])
def test_g23_soft_constraints_restated_and_path_constraints_points(g23, name):
    from mmd_amd.multi_agent import PathConstraints
    _, _, n, lengths, starts, script = _case(g23, name)
    for si in range(3):
        ix = [int(v) for v in g23[f"{name}.state{si}_ix"]]
        batches = [script[k][si % st.N_ENTRIES][0] for k in range(n)]
        for agent in range(n):
            for n_state in (n, agent):
                want = g23[f"{name}.state{si}_soft{agent}_{n_state}"]
                got = np_soft_points([batches[k][ix[k]] for k in range(n)], lengths, starts, agent, n_state)
                np.testing.assert_array_equal(got, want)
                pc = PathConstraints([torch.from_numpy(b) for b in batches[:n_state]], ix[:n_state], agent, starts, n_state=n_state)
                q, r_l = pc.points()
                np.testing.assert_array_equal(q, want[:, :2])
                np.testing.assert_array_equal(np.array(r_l, np.float32).reshape(-1, 2), want[:, 2:4])
                cl = pc.constraint_list()
                assert len(cl) == (1 if len(want) else 0)
                if cl:
                    assert cl[0].is_soft
                    np.testing.assert_array_equal(np.array(cl[0].radius_l, np.float32), want[:, 4])
                    # the ELL extent of the group: as many slots as agents contribute a point at one t < H
                    has, slots = pc.extent()
                    fill = np.zeros(64, int)
                    for t0 in want[:, 2].astype(int):
                        if t0 < 64:
                            fill[t0] += 1
                    assert has and slots == fill.max()


def test_g23_pp_hard_ranges(g23):
    """PP (prioritized_planning.py:149-159): agents 0 .. i-1 as hard constraints, ranges clamped to [0, H-1] -- the call log of g23."""
    from mmd_amd.multi_agent import PathConstraints
    for name in ("pp", "pp_mixed"):
        _, _, n, lengths, starts, script = _case(g23, name)
        calls, cons, pts = g23[name + ".calls"], g23[name + ".cons"], g23[name + ".points"]
        chosen = [int(v) for v in g23[name + ".nodes_ix"][0]]
        p0 = 0
        for ci, (agent, n_cons, exp) in enumerate(calls):
            assert exp == 0
            pc = PathConstraints([torch.from_numpy(script[k][0][0]) for k in range(agent)], chosen[:agent], agent, starts, n_state=agent,
                                 is_soft=False)
            cl = pc.constraint_list()
            assert len(cl) == n_cons
            for c in cl:
                k = c.get_q_l().shape[0]
                want = pts[p0:p0 + k]
                np.testing.assert_array_equal(c.get_q_l().numpy(), want[:, :2].astype(np.float32))
                np.testing.assert_array_equal(np.array(c.get_t_range_l(), np.float64), want[:, 2:4])
                assert not c.is_soft
                p0 += k
        assert p0 == pts.shape[0]


def test_convert_conflicts_and_range_clamping():
    from mmd_amd.constraints import MultiPointConstraint
    from mmd_amd.multi_agent_planners import (PointConflict, VertexConflict, EdgeConflict, convert_conflicts_to_constraints,
                                              shift_and_clamp_t_ranges, TrialSuccessStatus)
    mid = torch.tensor([0.1, -0.2])
    c = PointConflict([2, 0], q_l=[mid, mid], p_l=[torch.zeros(2), torch.ones(2)], t_from=3, t_to=3)
    out = convert_conflicts_to_constraints(c, {PointConflict: {MultiPointConstraint}})
    assert [a for a, _ in out] == [2, 0]
    for _, mc in out:
        assert mc.t_range_l == [(1, 5)] and mc.radius_l == [0.05 * 2.4] and not mc.is_soft and torch.equal(mc.q_l[0], mid)
    with pytest.raises(NotImplementedError):
        convert_conflicts_to_constraints(VertexConflict([0, 1], [mid, mid], 3), {VertexConflict: {MultiPointConstraint}})
    with pytest.raises(NotImplementedError):
        convert_conflicts_to_constraints(EdgeConflict([0, 1], [mid, mid], [mid, mid], 3, 4), {EdgeConflict: {MultiPointConstraint}})
    # cbs.py:395-406: shifted by the start time, clamped to [0, L - 1]
    assert shift_and_clamp_t_ranges([(1, 5)], 5, 64) == [(0, 0)]
    assert shift_and_clamp_t_ranges([(8, 12)], 5, 64) == [(3, 7)]
    assert shift_and_clamp_t_ranges([(70, 74)], 5, 64) == [(63, 63)]
    assert shift_and_clamp_t_ranges([(130, 134)], 0, 128) == [(127, 127)]
    # experiments.py:168-176
    assert [s.value for s in TrialSuccessStatus] == [-1, 0, 1, 2, 3]
    assert [s.name for s in TrialSuccessStatus] == ["UNKNOWN", "SUCCESS", "FAIL_RUNTIME_LIMIT", "FAIL_COLLISION_AGENTS", "FAIL_NO_SOLUTION"]
    assert bool(TrialSuccessStatus.SUCCESS) and not any(bool(s) for s in TrialSuccessStatus if s is not TrialSuccessStatus.SUCCESS)


def test_g23_results_and_global_pad_paths(g23):
    from mmd_amd.multi_agent_planners import TrialSuccessStatus, global_pad_paths
    for name in ("pp", "pp_mixed"):
        _, _, n, lengths, starts, script = _case(g23, name)
        chosen = [int(v) for v in g23[name + ".nodes_ix"][0]]
        got = global_pad_paths([torch.from_numpy(script[k][0][0][chosen[k]]) for k in range(n)], starts)
        np.testing.assert_array_equal(torch.stack(got).numpy(), g23[name + ".result_paths"])
        assert TrialSuccessStatus(int(g23[name + ".result"][1])) is TrialSuccessStatus.SUCCESS
    assert TrialSuccessStatus(int(g23["xecbs.result"][1])) is TrialSuccessStatus.FAIL_NO_SOLUTION


def _round_f32(x):
    """A Fraction rounded to the nearest fp32, ties to even."""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    key = [(abs(Fraction(float(c)) - x), int(np.array(c, np.float32).view(np.int32)) & 1) for c in cands]
    return cands[min(range(3), key=lambda i: key[i])]


def test_torch_norm_is_sqrt_fma_dy_dy_dx_dx():
    """The collision kernels pin torch.norm(d, dim=-1) over (dx, dy) in fp32 as sqrt(fma(dy, dy, dx * dx)).  This host's torch must
    compute that form on near-margin pairs (else the bitwise GPU tests of the decisions have no fixed reference); the fma is exact
    (Fraction), rounded once to nearest-even fp32, and fp32_forms.fma_f32 agrees with it.  The two other forms differ on these pairs."""
    pa, pb = F.margin_pairs(5, 20000)
    d = pa - pb
    dx, dy = d[:, 0], d[:, 1]
    tn = torch.norm(torch.from_numpy(d), dim=-1).numpy()
    ln = torch.linalg.norm(torch.from_numpy(d), dim=-1).numpy()
    sub = np.random.default_rng(6).choice(len(d), 3000, replace=False)
    exact = np.array([np.sqrt(_round_f32(Fraction(float(y)) * Fraction(float(y)) + Fraction(float(np.float32(x * x)))))
                      for x, y in zip(dx[sub], dy[sub])], np.float32)
    np.testing.assert_array_equal(F.torch_norm2(dx[sub], dy[sub]), exact)
    np.testing.assert_array_equal(tn[sub], exact)
    np.testing.assert_array_equal(tn, F.torch_norm2(dx, dy))
    np.testing.assert_array_equal(ln, tn)
    # broadcast [T, n, n, 2] as check_rr_collisions forms it
    q = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (64, 33, 2)).astype(np.float32))
    qn = q.numpy()
    np.testing.assert_array_equal(torch.norm(q.unsqueeze(-2) - q.unsqueeze(-3), dim=-1).numpy(), F.pos_norm(qn[:, :, None], qn[:, None]))
    # the forms the guard tells apart: two roundings, and the fma with the operands the other way round
    assert (np.sqrt(dx * dx + dy * dy) != tn).sum() > 100
    assert (np.sqrt(F.fma_f32(dx, dx, dy * dy)) != tn).sum() > 100
    below, above = F.sides(tn)
    assert below > 5000 and above > 5000


def test_host_restatements_decide_as_check_rr_collisions():
    """np_conflicts and test_gpu_mapf._host_conflicts (the independent recounts of the GPU tests) decide near-margin pairs as
    O.check_rr_collisions does."""
    from oracle import mmd_oracle as O
    import test_gpu_mapf
    pa, pb = F.margin_pairs(8, 2000)
    qa, qb = F.margin_pairs(9, 2000)
    m = min(len(pa), len(qa))
    paths = np.stack([pa[:m], pb[:m], qa[:m], qb[:m]])                                  # [4, T, 2]
    coll, mid = O.check_rr_collisions(torch.from_numpy(paths).permute(1, 0, 2))
    assert F.sides(F.pos_norm(pa, pb))[0] > 500 and F.sides(F.pos_norm(pa, pb))[1] > 500
    nz = torch.nonzero(coll).numpy()
    got = np_conflicts(list(paths), [m] * 4, [0] * 4, ordered=True)
    np.testing.assert_array_equal(got[:, :3].astype(np.int64), nz)
    np.testing.assert_array_equal(got[:, 7:9], mid.numpy()[nz[:, 0], nz[:, 1], nz[:, 2]])
    got = np_conflicts(list(paths), [m] * 4, [0] * 4, ordered=False)
    np.testing.assert_array_equal(got[:, :3].astype(np.int64), nz[nz[:, 1] < nz[:, 2]])
    assert test_gpu_mapf._host_conflicts([torch.from_numpy(p) for p in paths]) == int(coll.sum())
