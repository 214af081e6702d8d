"""-m gpu: the multi-agent search layer (mmd_find_conflicts, mmd_scan_candidates, mmd_path_constraints) and the collision kernels
(mmd_rr_collisions, mmd_count_collisions) beyond golden g23's four agents: up to 64 agents of mixed lengths and start times (global horizons
up to ~340), rows full of hits, truncated lists, hundreds of candidates with ties across waves, and the searches end to end at 10 and 32
agents.  The reference is a vectorised NumPy restatement of get_conflicts in torch.norm's fp32 distance form (fp32_forms)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp32_forms as F                   # noqa: E402
import mapf_stub as st                   # noqa: E402
from oracle import mmd_oracle as O       # noqa: E402

H = 64
SENTINEL = -0x2F2F2F2F
LENGTHS = (1, 2, 64, 128, 192)


def _instance(seed, n, box=0.3, lengths=None, starts=None, n_samples=3):
    """n agents: lengths from LENGTHS, starts in 0 .. 150, positions packed in [-box, box]^2 so that rows hold many hits; agent k's
    path is sample ix[k] of batches[k] [n_samples, L_k, 4]."""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in (rng.choice(LENGTHS, n) if lengths is None else lengths)]
    starts = [int(v) for v in (rng.integers(0, 151, n) if starts is None else starts)]
    batches = [rng.uniform(-box, box, (n_samples, L, 4)).astype(np.float32) for L in lengths]
    ix = [int(v) for v in rng.integers(0, n_samples, n)]
    return batches, ix, lengths, starts


def _padded(paths, lengths, starts):
    """global_pad_paths: pos [Tg, n, 2], agent k at t = path_k[clamp(t - s_k, 0, L_k - 1)]."""
    Tg = max(L + s for L, s in zip(lengths, starts))
    t = np.arange(Tg)
    return np.stack([p[np.clip(t - s, 0, L - 1), :2] for p, L, s in zip(paths, lengths, starts)], 1)


def _hits(pos):
    """[Tg, n, n] bool: ||pa - pb|| < 2.1 r in torch.norm's fp32 form, a != b."""
    h = F.pos_norm(pos[:, :, None], pos[:, None, :]) < F.MARGIN
    n = pos.shape[1]
    h[:, np.arange(n), np.arange(n)] = False
    return h


def _ref_records(pos, ordered):
    """get_conflicts restated: the mmd_conflict words [m, 12] in (t, a, b) row-major order."""
    h = _hits(pos)
    if not ordered:
        h &= np.triu(np.ones(h.shape[1:], bool), 1)[None]
    t, a, b = np.nonzero(h)
    pa, pb = pos[t, a], pos[t, b]
    w = np.zeros((len(t), 12), np.int32)
    w[:, 0], w[:, 1], w[:, 2] = t, a, b
    w[:, 4:6] = pa.view(np.int32)
    w[:, 6:8] = pb.view(np.int32)
    w[:, 8:10] = ((pa + pb) / np.float32(2)).view(np.int32)
    return w


def _table(batches, ix, starts):
    from mmd_amd import multi_agent as ma
    dev = [torch.from_numpy(b).cuda() for b in batches]
    return ma.agent_table(dev, ix, starts), dev


def _raw_find(table, n, Tg, mode, cap):
    """mmd_find_conflicts into sentinel-filled buffers: (summary [16], list [cap + 4, 12]) on the host."""
    from mmd_amd import _lib
    summ = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    rows = torch.empty(Tg, dtype=torch.int32, device="cuda")
    lst = torch.full((cap + 4, 12), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.launch("mmd_find_conflicts", table, table.data_ptr(), n, Tg, float(F.MARGIN), mode, rows.data_ptr(), summ.data_ptr(),
                summ.data_ptr() + 16, lst.data_ptr() if cap else None, cap)
    return summ.cpu().numpy(), lst.cpu().numpy()


def _check_find(batches, ix, lengths, starts, caps=True):
    from mmd_amd import multi_agent as ma
    table, _ = _table(batches, ix, starts)
    n, Tg = len(batches), ma.global_horizon(lengths, starts)
    pos = _padded([b[i] for b, i in zip(batches, ix)], lengths, starts)
    counts = {}
    for ordered, mode in ((True, ma.ORDERED), (False, ma.PAIRS)):
        want = _ref_records(pos, ordered)
        m = len(want)
        counts[ordered] = m
        summ, lst = _raw_find(table, n, Tg, mode, m)
        assert int(summ[0]) == m, (ordered, int(summ[0]), m)
        assert (summ[1:4] == SENTINEL).all()
        bad = np.nonzero((lst[:m] != want).any(1))[0]
        assert bad.size == 0, f"ordered={ordered}: {bad.size} of {m} records differ, first {lst[bad[0]] if bad.size else None}"
        assert (lst[m:] == SENTINEL).all()
        if m:
            np.testing.assert_array_equal(summ[4:16], want[0])
        else:
            assert summ[4:7].tolist() == [-1, -1, -1]
        if caps and m:
            for cap in sorted({1, max(m - 1, 1), m, m + 7}):
                summ, lst = _raw_find(table, n, Tg, mode, cap)
                k = min(cap, m)
                assert int(summ[0]) == m
                np.testing.assert_array_equal(lst[:k], want[:k])
                assert (lst[k:] == SENTINEL).all(), (cap, m)
    assert counts[True] == 2 * counts[False]
    return counts[True], pos


@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (5, 3), (17, 4), (33, 5), (64, 6)])
def test_find_conflicts_at_scale(n, seed):
    """Both modes: the count, the whole list and the first record bitwise, truncated lists a prefix with nothing written past list_cap."""
    batches, ix, lengths, starts = _instance(seed, n)
    m, pos = _check_find(batches, ix, lengths, starts)
    if n == 1:
        assert m == 0
    if n >= 17:
        assert m > 1000 and pos.shape[0] > 256


def test_find_conflicts_rows_full_of_hits():
    """33 agents on one point for ten rows: every cell of those rows (1056 > 256 per pass) is a conflict."""
    batches, ix, lengths, starts = _instance(7, 33, box=1.0, lengths=[64] * 33, starts=[0] * 33)
    for b, i in zip(batches, ix):
        b[i, 10:20, :2] = np.float32([0.1, -0.2])
    m, pos = _check_find(batches, ix, lengths, starts)
    assert _hits(pos)[10:20].all(axis=0)[~np.eye(33, dtype=bool)].all() and m >= 10 * 33 * 32


def test_find_conflicts_only_in_the_last_row_and_none():
    """The only conflict lies in row Tg - 1; agents apart everywhere give a count of 0 and an empty first record (words 4-6 = -1)."""
    far = np.array([[-0.8, -0.8], [0.8, -0.8], [0.0, 0.8]], np.float32)
    batches = [np.zeros((1, L, 4), np.float32) for L in (64, 2, 128)]
    for k, b in enumerate(batches):
        b[0, :, :2] = far[k]
    batches[1][0, 1, :2] = far[0] + np.float32([0.05, 0.0])              # agent 1's last point (t = 150 + 1) meets agent 0's last
    lengths, starts = [64, 2, 128], [0, 150, 24]
    m, pos = _check_find(batches, [0, 0, 0], lengths, starts)
    assert m == 2 and pos.shape[0] == 152
    batches[1][0, 1, :2] = far[1]
    m, _ = _check_find(batches, [0, 0, 0], lengths, starts)
    assert m == 0


def _scan_instance(seed=11, n=17, Bc=800):
    """Agent `agent` (L = 64) of an n-agent instance and Bc candidates for it: 8 distinct trajectories repeated, so the smallest
    count occurs in many waves; candidate 0 sits far from everything."""
    rng = np.random.default_rng(seed)
    batches, ix, lengths, starts = _instance(seed, n)
    agent = 3
    lengths[agent] = 64
    distinct = rng.uniform(-0.3, 0.3, (8, 64, 4)).astype(np.float32)
    cand = distinct[rng.integers(0, 8, Bc)]
    cand[0, :, :2] = np.float32([5.0, 5.0])
    batches[agent] = cand
    ix[agent] = 0
    return batches, ix, lengths, starts, agent, cand


def _ref_scan(batches, ix, lengths, starts, agent, cand):
    """(ordered counts, pair counts) of the state with candidate c put in, for every c: base + mult * candidate hits."""
    paths = [b[i] for b, i in zip(batches, ix)]
    pos = _padded(paths, lengths, starts)
    h = _hits(pos)
    keep = np.ones(len(paths), bool)
    keep[agent] = False
    base = int(h[:, keep][:, :, keep].sum())
    t = np.arange(pos.shape[0])
    cpos = cand[:, np.clip(t - starts[agent], 0, lengths[agent] - 1), :2]                     # [Bc, Tg, 2]
    ch = F.pos_norm(cpos[:, :, None], pos[None]) < F.MARGIN                                   # [Bc, Tg, n]
    ch[:, :, agent] = False
    hits = ch.sum(axis=(1, 2)).astype(np.int64)
    return base + 2 * hits, base // 2 + hits


def _recount(batches, ix, lengths, starts, agent, c):
    ixc = list(ix)
    ixc[agent] = int(c)
    return int(_hits(_padded([b[i] for b, i in zip(batches, ixc)], lengths, starts)).sum())


@pytest.fixture(scope="module")
def scan_case():
    batches, ix, lengths, starts, agent, cand = _scan_instance()
    ordered, pairs = _ref_scan(batches, ix, lengths, starts, agent, cand)
    for c in np.random.default_rng(12).choice(len(cand), 10, replace=False):                   # the decomposition against full recounts
        full = _recount(batches, ix, lengths, starts, agent, c)
        assert ordered[c] == full and pairs[c] * 2 == full
    return batches, ix, lengths, starts, agent, cand, ordered, pairs


@pytest.mark.parametrize("n_free", [0, 1, 63, 64, 65, 255, 256, 257, 700])
def test_scan_candidates_at_scale(scan_case, n_free):
    """Every returned count, the CBS pick (first in list order among the smallest) and the PP rule from an init_idx outside the free list
    whose count lies below, at and above the free minimum; both modes; n_free = 0 gives (-1, -1) under CBS and the init sample under PP."""
    from mmd_amd import multi_agent as ma
    batches, ix, lengths, starts, agent, cand, ordered, pairs = scan_case
    table, dev = _table(batches, ix, starts)
    n, Tg = len(batches), ma.global_horizon(lengths, starts)
    rng = np.random.default_rng(100 + n_free)
    free = rng.permutation(np.arange(1, len(cand)))[:n_free]
    outside = np.setdiff1d(np.arange(len(cand)), free)
    for mode, want_all in ((ma.ORDERED, ordered), (ma.PAIRS, pairs)):
        res, counts = ma.scan_candidates(table, n, Tg, agent, dev[agent], torch.from_numpy(free).cuda(), mode, ma.SELECT_CBS, with_counts=True)
        want = want_all[free]
        assert counts.cpu().numpy().tolist() == want.tolist()
        if n_free:
            k = int(np.argmin(want))
            assert res.cpu().tolist() == [int(free[k]), int(want[k])]
            fmin = int(want[k])
        else:
            assert res.cpu().tolist() == [-1, -1]
            fmin = None
        inits = [0]                                                                            # below: the far candidate
        for rel in (0, 1):                                                                     # equal / above, if outside has them
            sel = outside[(want_all[outside] == fmin) if rel == 0 else (want_all[outside] > (fmin if fmin is not None else -1))] \
                if fmin is not None or rel else np.zeros(0, np.int64)
            if sel.size:
                inits.append(int(sel[0]))
        for init in inits:
            res = ma.scan_candidates(table, n, Tg, agent, dev[agent], torch.from_numpy(free).cuda(), mode, ma.SELECT_PP, init_idx=init)
            if fmin is not None and fmin < want_all[init]:
                assert res.cpu().tolist() == [int(free[int(np.argmin(want))]), fmin]
            else:
                assert res.cpu().tolist() == [init, int(want_all[init])]
    if n_free >= 63:
        assert (ordered[free] == ordered[free].min()).sum() > 1                                 # ties across positions


@pytest.mark.parametrize("hard", [False, True])
def test_path_constraints_at_scale(hard):
    """mmd_path_constraints over states of up to 64 agents with mixed lengths and earlier / later start offsets, the agent inside and
    outside the state: bitwise pack_constraints of the restated point list, unused slots (0, 0, -1, -1) at the end of each column."""
    from mmd_amd import multi_agent as ma
    from test_gpu_mapf import _ref_pack
    batches, ix, lengths, starts = _instance(21, 64)
    lengths[10] = lengths[40] = 64
    for k in (10, 40):
        batches[k] = np.random.default_rng(k).uniform(-0.3, 0.3, (3, 64, 4)).astype(np.float32)
    dev = [torch.from_numpy(b).cuda() for b in batches]
    seen = 0
    for agent, n_state in ((10, 64), (10, 33), (40, 64), (40, 17), (10, 5)):
        pc = ma.PathConstraints(dev[:n_state], ix[:n_state], agent, starts if agent < n_state else starts[:max(n_state, agent + 1)],
                                n_state=n_state, is_soft=not hard)
        has, slots = pc.extent()
        ref = _ref_pack(pc, 0.5)
        if not has:
            assert ref is None
            continue
        ell, gso, gw, rgo = pc.build(0.5)
        if slots == 0:
            continue
        assert torch.equal(ell, ref[0][:slots]) and ref[0].shape[0] == slots
        assert torch.equal(gso, ref[1]) and torch.equal(gw, ref[2]) and torch.equal(rgo, ref[3])
        e = ell.cpu().numpy()
        empty = (e == np.float32([0, 0, -1, -1])).all(-1)                                      # [slots, H]
        assert (np.diff(empty.astype(int), axis=0) >= 0).all()                                 # a column's empty slots come last
        assert np.isclose(e[~empty][:, 2], ma.VERTEX_CONSTRAINT_RADIUS).all()
        seen += 1
    assert seen >= 3


def test_rr_collisions_grid_stride():
    """n = 160, T = 64: more cells than 4096 x 256, so the grid-stride loop runs; mask and midpoints bitwise O.check_rr_collisions."""
    from mmd_amd import multi_agent as ma
    paths = np.random.default_rng(31).uniform(-0.5, 0.5, (160, 64, 2)).astype(np.float32)
    coll, mid = ma.check_rr_collisions(torch.from_numpy(paths).cuda())
    wc, wm = O.check_rr_collisions(torch.from_numpy(paths).permute(1, 0, 2))
    assert torch.equal(coll.cpu(), wc) and int(wc.sum()) > 10000
    got, want = mid.cpu().numpy(), wm.numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~np.isnan(want)].view(np.int32), want[~np.isnan(want)].view(np.int32))


def test_count_collisions_partial_block_and_offset():
    """n_all = 64, robot0 = 5, 3 local robots x 7 samples (21 trajectories, not a multiple of 4): O.count_collisions_with_others."""
    from mmd_amd import multi_agent as ma
    rng = np.random.default_rng(41)
    paths = rng.uniform(-0.4, 0.4, (64, H, 2)).astype(np.float32)
    trajs = rng.uniform(-0.4, 0.4, (21, H, 4)).astype(np.float32)
    got = ma.count_collisions(torch.from_numpy(trajs).cuda(), torch.from_numpy(paths).cuda(), 5, 3).cpu()
    assert got.shape == (3, 7)
    for r in range(3):
        want = O.count_collisions_with_others(torch.from_numpy(trajs[7 * r:7 * (r + 1), :, :2]), torch.from_numpy(paths), 5 + r)
        assert got[r].tolist() == want.tolist() and int(want.sum()) > 0


class _FreeTask:
    def compute_collision(self, x, **kw):
        return torch.zeros(x.shape[:-1], dtype=torch.bool, device=x.device)


@pytest.mark.parametrize("alg_name,n", [("PP", 32), ("ECBS", 10)])
def test_search_end_to_end_at_scale(alg_name, n):
    """Prioritized planning at 32 agents and ECBS at 10 over the scripted planner, each under a runtime limit: a SUCCESS /
    FAIL_COLLISION_AGENTS status agrees with the torch-form recount of the returned paths, and n_conflicts equals the recount."""
    from mmd_amd.constraints import MultiPointConstraint
    from mmd_amd.multi_agent_planners import CBS, PointConflict, PrioritizedPlanning, TrialSuccessStatus
    from mmd_amd.planners import RobotPlanarDiskFacade
    script = st.make_script(n, [64] * n, None, 900 + n)
    robot = RobotPlanarDiskFacade("cuda")
    log = []
    planners = [st.ScriptedPlanner(k, script[k], log, robot, _FreeTask(), device="cuda") for k in range(n)]
    s, g = st.starts_goals(n)
    s, g = s * np.float32(1.5), g * np.float32(1.5)              # (only validated: 0.15 apart at 32 agents; the script plans at 0.6)
    sl, gl = [torch.from_numpy(v).cuda() for v in s], [torch.from_numpy(v).cuda() for v in g]
    times = [2 * k for k in range(n)]
    if alg_name == "PP":
        alg = PrioritizedPlanning(planners, sl, gl, start_time_l=times)
    else:
        alg = CBS(planners, sl, gl, start_time_l=times, conflict_type_to_constraint_types={PointConflict: {MultiPointConstraint}}, is_ecbs=True)
    paths, n_exp, status, n_conf = alg.plan(runtime_limit=25)
    assert status in (TrialSuccessStatus.SUCCESS, TrialSuccessStatus.FAIL_COLLISION_AGENTS, TrialSuccessStatus.FAIL_RUNTIME_LIMIT,
                      TrialSuccessStatus.FAIL_NO_SOLUTION)
    if status in (TrialSuccessStatus.SUCCESS, TrialSuccessStatus.FAIL_COLLISION_AGENTS):
        pos = torch.stack(paths)[..., :2].cpu().numpy().transpose(1, 0, 2)                     # already padded: [Tg, n, 2]
        host = int(_hits(np.ascontiguousarray(pos)).sum())
        assert (status is TrialSuccessStatus.SUCCESS) == (host == 0)
        assert n_conf == (host if alg_name == "ECBS" else host // 2)
