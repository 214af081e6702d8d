"""-m gpu: the seeds of a world fleet's epochs.  mmd_grid_window_goal_samples is the numpy definition window_goals_samples word for word,
on the grids, goals, queries and settings of test_gpu_world_fleet with every goal cell added as a start, and on its hand-built batch of
every status, with guard words round all four outputs; mmd_window_seeds is window_seed bit for bit, on walks and on rows no walk gives;
plan_rounds_seeded(init_trajs) is sample_local on the given trajectories; and a seeded fleet crosses test_gpu_world_fleet's world, every epoch
equal to the sequence built by hand from the public pieces."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import world_fleet_model as M                                    # noqa: E402
import world_fleet_seed_model as S                               # noqa: E402
import test_gpu_world_fleet as W                                 # noqa: E402
from test_gpu_world_fleet import crossing                        # noqa: E402,F401  (the module's fixture: the unseeded run of the same world)
from mmd_amd import _lib, environments as E, map_textures, synth, world_fleet as F      # noqa: E402
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED, UNREACHED      # noqa: E402

GUARD, PAD, I32 = W.GUARD, W.PAD, W.I32
FGUARD = 0x7fc00abc              # a NaN's bits: the guard words round the float outputs


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()                             # (a copy: the shared arrays are read-only)


# ---- 1. the samples kernel is the definition ------------------------------------------------------------------------------------------------------
def raw_samples(dist, starts, which, goals, reach, max_steps, window):
    """mmd_grid_window_goal_samples on numpy inputs, twice into one buffer whose every word outside the four outputs is a guard ->
    (cells, origins, summary, samples) numpy.  The guards must be untouched and the second call must give the first one's words."""
    dist_d = dev(np.array(dist, dtype=np.int32), np.int32)
    starts_d, which_d = dev(np.asarray(starts).reshape(-1, 2), np.int32), dev(np.asarray(which).reshape(-1), np.int32)
    goals_d = dev(np.asarray(goals).reshape(-1, 2), np.int32)
    n = starts_d.shape[0]
    sizes = (2 * n, 2 * n, 4 * n, 128 * n)
    at = [PAD + sum(sizes[:k]) + k * PAD for k in range(4)]      # the first word of cells, origins, summary, samples
    size = at[3] + sizes[3] + PAD
    buf = torch.full((size,), GUARD, dtype=torch.int32, device="cuda")
    inside = np.zeros(size, bool)
    for a, m in zip(at, sizes):
        inside[a:a + m] = True
    runs = []
    for _ in range(2):
        _lib.launch("mmd_grid_window_goal_samples", buf, C.c_void_p(dist_d.data_ptr()), dist.shape[1], dist.shape[2], dist.shape[0],
                    C.c_void_p(starts_d.data_ptr()), C.c_void_p(which_d.data_ptr()), C.c_void_p(goals_d.data_ptr()), n, reach, max_steps,
                    window, *(C.c_void_p(buf.data_ptr() + 4 * k) for k in at))
        torch.cuda.synchronize()
        words = buf.cpu().numpy()
        assert (~inside).sum() == 5 * PAD and (words[~inside] == GUARD).all(), "wrote outside the outputs"
        runs.append(tuple(words[a:a + m].reshape(shape).copy() for a, m, shape in zip(at, sizes, ((n, 2), (n, 2), (n, 4), (n, 64, 2)))))
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "a second call into the same buffer differs"
    return runs[0]


def assert_same(got, want, what):
    W.assert_same(got[:3], want[:3], what)
    g = got[3].cpu().numpy() if isinstance(got[3], torch.Tensor) else got[3]
    assert g.dtype == np.int32 and g.shape == want[3].shape, (what, g.dtype, g.shape)
    bad = np.flatnonzero((g != want[3]).any((1, 2)))
    assert bad.size == 0, f"{what}: samples differ in {bad.size} of {len(g)} queries, first {int(bad[0])}: device {g[bad[0]].tolist()} " \
                          f"definition {want[3][bad[0]].tolist()}"


@pytest.mark.parametrize("grid", list(W.GRIDS))
def test_samples_kernel_is_the_definition(grid):
    make, goals, window, settings = W.GRIDS[grid]
    routable = make()
    dist = M.fields(routable, goals)
    starts, which = W.queries(routable.shape, len(goals), 700, 11)
    starts = np.concatenate([starts, np.asarray(goals, np.int32)])                       # every goal cell as a start, in its own field
    which = np.concatenate([which, np.arange(len(goals), dtype=np.int32)])
    dist_d = torch.from_numpy(dist.copy()).cuda()
    classes = set()
    for reach, max_steps in settings:
        want = F.window_goals_samples(dist, starts, which, goals, reach, max_steps, window)
        ok = want[2][:, 2] == ROUTE_OK
        steps = want[2][ok, 0]
        count = {"0": int((steps == 0).sum()), "<63": int(((steps > 0) & (steps < 63)).sum()), "63": int((steps == 63).sum()),
                 ">=64": int((steps >= 64).sum())}
        print(f"{grid}, reach {reach}, max_steps {max_steps}: {int(ok.sum())} OK queries, steps {count}, longest {int(steps.max())}")
        classes |= {k for k, v in count.items() if v}
        assert ok.sum() > 400 and (~ok).any() and (want[2][-len(goals):, 0] == 0).all() and want[2][-len(goals):, 3].all()
        assert not want[3][~ok].any()
        if (grid, reach, max_steps) == ("serpentine", 31, 1000):                         # this setting alone holds all four classes
            assert (count["0"], count["<63"], count["63"], count[">=64"], int(steps.max())) == (3, 452, 3, 171, 122)
        what = f"{grid}, reach {reach}, max_steps {max_steps}"
        got = raw_samples(dist, starts, which, goals, reach, max_steps, window)
        assert_same(got, want, what)
        assert_same(got[:3] + (got[3],), F.window_goals(dist, starts, which, goals, reach, max_steps, window) + (want[3],), what + " (window_goals)")
        assert_same(F.device_window_goal_samples(dist_d, starts, which, goals, reach, max_steps, window), want, what + " (device_window_goal_samples)")
    # a walk of 63 steps or more needs a reach of 32 or more on open ground, or a corridor: the 40 x 30 grids, whose window of 12 cells
    # allows a reach of 5, hold the first two classes only (a walk inside a box of 11 x 11 cells)
    assert classes == ({"0", "<63", "63", ">=64"} if grid == "serpentine" else {"0", "<63"})


def test_samples_of_every_status_in_one_batch():
    """test_gpu_world_fleet's hand-built batch: an unconverged field (stuck at once and after 2 steps), a converged one, one that is
    UNREACHED everywhere, and one of words no search would leave, with a goal at the ends of int32."""
    stuck, goal0, sticks_at = M.unconverged_field()
    odd = np.zeros((1,) + M.SMALL, np.int32)
    odd[0, 5, 5], odd[0, 6, 6], odd[0, 7, 7] = -3, I32.min, I32.max - 1
    dist = np.concatenate([stuck, M.fields(M.open_grid(), [(20, 15)]), np.full((1,) + M.SMALL, UNREACHED, np.int32), odd])
    goals = [goal0, (20, 15), (1, 1), (I32.min, I32.max)]
    starts = [sticks_at, (10, 12), (14, 10), (20, 15), (20, 14), (-1, 3), (3, 30), (40, 0), (I32.min, I32.max), (14, 10), (14, 10), (14, 10),
              (9, 9), (5, 5), (6, 6), (7, 7), (8, 8)]
    which = [0, 0, 1, 1, 1, 1, 1, 1, 1, 4, -1, I32.max, 2, 3, 3, 3, 3]
    want = F.window_goals_samples(dist, starts, which, goals, M.REACH, 100, M.WINDOW)
    assert set(want[2][:, 2].tolist()) == {ROUTE_OK, ROUTE_UNREACHED, ROUTE_STUCK, ROUTE_OUTSIDE}
    assert want[2][1].tolist() == [2, 14, ROUTE_STUCK, 0] and not want[3][1].any()          # a stuck walk that covered 2 steps: no samples
    assert (want[3][13] == (5, 5)).all() and (want[3][14] == (6, 6)).all()                  # d0 <= 0: no step, 64 times the start
    assert_same(raw_samples(dist, starts, which, goals, M.REACH, 100, M.WINDOW), want, "the batch of every status")
    none = raw_samples(np.zeros((0,) + M.SMALL, np.int32), starts[:3], [0, 0, 0], np.zeros((0, 2), np.int32), M.REACH, 100, M.WINDOW)
    assert none[2].tolist() == [[-1, -1, ROUTE_OUTSIDE, 0]] * 3 and not none[0].any() and not none[1].any() and not none[3].any()


def test_samples_error_returns_leave_the_outputs_alone():
    lib = _lib.load()
    dist = torch.zeros(2, 40, 30, dtype=torch.int32, device="cuda")
    ints = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((1280,), GUARD, dtype=torch.int32, device="cuda")
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * k)                                  # noqa: E731
    good = dict(dist=p(dist), nx=40, ny=30, n_fields=2, starts=p(ints), field=p(ints, 32), goals=p(ints, 48), n=7, reach=5, max_steps=9,
                window=12, cells=p(out, 16), origins=p(out, 64), summary=p(out, 128), samples=p(out, 256))
    order = ("dist", "nx", "ny", "n_fields", "starts", "field", "goals", "n", "reach", "max_steps", "window", "cells", "origins", "summary",
             "samples")
    stream = C.c_void_p(_lib.raw_stream())
    call = lambda **kw: lib.mmd_grid_window_goal_samples(*(dict(good, **kw)[k] for k in order), stream)      # noqa: E731
    for kw in (dict(nx=0), dict(nx=2049), dict(ny=0), dict(ny=2049), dict(n_fields=-1), dict(n=-1), dict(n=I32.max), dict(reach=0),
               dict(reach=6), dict(reach=-1), dict(max_steps=0), dict(max_steps=-5), dict(window=31), dict(window=0), dict(window=3, reach=1),
               dict(window=41, ny=50), dict(dist=None), dict(goals=None), dict(starts=None), dict(field=None), dict(cells=None),
               dict(origins=None), dict(summary=None), dict(samples=None)):
        assert call(**kw) == 2 and lib.mmd_last_error().startswith(b"mmd_grid_window_goal_samples:"), (kw, lib.mmd_last_error())
    assert call(n=0) == 0 and call(n=0, dist=None, starts=None, summary=None, samples=None) == 0
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call, or one of no queries, wrote"
    assert call() == 0                                        # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    words = out.cpu().numpy()
    assert not words[16:30].any() and not words[64:78].any() and not words[256:256 + 7 * 128].any()      # all at cell (0, 0), field 0 of zeros
    assert words[128:156].reshape(7, 4).tolist() == [[0, 0, ROUTE_OK, 1]] * 7
    rest = np.concatenate([words[:16], words[30:64], words[78:128], words[156:256], words[256 + 7 * 128:]])
    assert (rest == GUARD).all()


# ---- 2. the seed kernel is the definition ----------------------------------------------------------------------------------------------------------
def raw_seeds(tex_d, shape, hi, clearance, samples, origins, summary, window, s_pts, g_pts, smooth_iters):
    """mmd_window_seeds on numpy inputs into a buffer with guard words in front of, between and behind seeds and clear_min"""
    n = len(samples)
    at = (PAD, 2 * PAD + 256 * n)
    size = at[1] + n + PAD
    buf = torch.full((size,), FGUARD, dtype=torch.int32, device="cuda")
    ins = [dev(samples, np.int32), dev(origins, np.int32), dev(summary, np.int32), dev(s_pts, np.float32), dev(g_pts, np.float32)]
    _lib.launch("mmd_window_seeds", buf, C.c_void_p(tex_d.data_ptr()), shape[0], shape[1], (C.c_float * 2)(*S.LO), (C.c_float * 2)(*hi),
                float(clearance), *(C.c_void_p(t.data_ptr()) for t in ins[:3]), n, window, C.c_void_p(ins[3].data_ptr()),
                C.c_void_p(ins[4].data_ptr()), int(smooth_iters), float(np.float32(2.0 * S.DT)), C.c_void_p(buf.data_ptr() + 4 * at[0]),
                C.c_void_p(buf.data_ptr() + 4 * at[1]))
    torch.cuda.synchronize()
    words = buf.cpu().numpy()
    guards = np.concatenate([words[:at[0]], words[at[0] + 256 * n:at[1]], words[at[1] + n:]])
    assert guards.size == 3 * PAD and (guards == FGUARD).all(), "wrote outside the outputs"
    return words[at[0]:at[0] + 256 * n].reshape(n, 64, 4).copy(), words[at[1]:at[1] + n].copy()


def assert_seed_bits(got, want, what, rows):
    """Equal bits, word for word.  Where the definition's word is a NaN the device's must be a NaN, of any sign and payload: IEEE 754
    leaves both to the implementation, and numpy's own word there depends on the host (b - NaN keeps the operand's sign on x86 and gives
    the default NaN elsewhere; gfx950 returns the operand negated: 0xffc00000 against 0x7fc00000, measured once, on the velocity next to
    a NaN start point).  Which words are NaN is the definition's rule and is held to; a NaN that is copied, not computed, keeps its bits
    (the test checks the start point's own word)."""
    for name, g, w in zip(("seeds", "clear_min"), got, want):
        w = bits(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        both_nan = np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32))
        g = np.where(both_nan, w, g)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        if bad.size:
            r = int(bad[0])
            at = np.argwhere(np.atleast_1d(g[r] != w[r]))[:4].tolist()
            raise AssertionError(f"{what}: {name} differ in {bad.size} of {len(g)} robots, first {r} ({rows(r)}) at {at}: device "
                                 f"{[hex(int(np.atleast_1d(g[r])[tuple(a)]) & 0xffffffff) for a in at]} definition "
                                 f"{[hex(int(np.atleast_1d(w[r])[tuple(a)]) & 0xffffffff) for a in at]}")


@pytest.mark.parametrize("name", ["door", "serpentine"])
def test_seed_kernel_is_the_definition(name):
    routable, _, _, window, _, tex, hi = S.grid(name)
    shape = routable.shape
    walks = S.robots(name, 112, 7)
    odd = S.odd_rows(name)
    batch = tuple(np.concatenate([a, b]) for a, b in zip(walks, odd[:5]))                   # 117 robots: 112 walks, then the five odd rows
    assert len(batch[0]) == 117 and np.isnan(batch[3][115, 0])
    rows = lambda r: "a walk" if r < 112 else odd[5][r - 112]                               # noqa: E731
    acc, rej = S.first_iteration_verdicts(name, walks[0], walks[3], walks[4], 0.006)
    print(f"{name}: first iteration at clearance 0.006: {acc} midpoints accepted, {rej} rejected")
    assert acc > 0 and rej > 0                                                              # both branches run
    tex_d = dev(tex, np.float32)
    for clearance in (0.0, 0.006):
        for iters in (0, 1, 7, 16):
            for n in (1, 117):
                part = tuple(a[:n] for a in batch)
                want = S.definition_seeds(name, *part, clearance, iters)
                what = f"{name}, clearance {clearance}, {iters} iterations, {n} robots"
                got = raw_seeds(tex_d, shape, hi, clearance, part[0], part[1], part[2], window, part[3], part[4], iters)
                assert_seed_bits(got, want, what, rows)
            if iters == 7:                                                                  # the wrapper: the same launch
                seeds, clear_min = F.device_window_seeds(tex_d, S.LO, hi, dev(batch[0], np.int32), dev(batch[1], np.int32),
                                                         dev(batch[2], np.int32), window, batch[3], batch[4], clearance, iters, S.DT)
                assert seeds.shape == (117, 64, 4) and clear_min.shape == (117,)
                assert_seed_bits((bits(seeds), bits(clear_min)), want, what + " (device_window_seeds)", rows)
            if iters == 16:
                seeds = want[0]
                assert not seeds[112].any() and want[1][112] == 0                           # not OK: zero rows
                for r in (113, 116):                                                        # outside the window: the centres, unmoved
                    assert np.array_equal(bits(seeds[r, 1:-1, :2]), bits(S.cell_centres(batch[0][r], S.LO, hi, shape)[1:-1]))
                assert np.isnan(seeds[115, 0, 0]) and np.isnan(seeds[115, 1, 2]) and not np.isnan(seeds[115, 1:, :2]).any()
                assert got[0][115, 0, 0] == bits(batch[3][115, 0]) and np.isnan(seeds[115]).sum() == 2       # the copied NaN keeps its bits
    with pytest.raises(ValueError):
        F.device_window_seeds(tex_d, S.LO, hi, dev(batch[0], np.int32), dev(batch[1][:5], np.int32), dev(batch[2], np.int32), window, batch[3],
                              batch[4])


# ---- 3. plan_rounds from given trajectories ---------------------------------------------------------------------------------------------------------
def test_plan_rounds_from_init_trajs():
    import gpu_common
    from mmd_amd.multi_robot import MultiRobotSampler
    T, B, seed = 25, 4, 77
    starts = np.float32([[-0.8, -0.7], [0.8, -0.75], [0.05, 0.85]])
    goals = np.float32([[0.8, 0.7], [-0.8, 0.75], [0.0, -0.85]])
    make = lambda: MultiRobotSampler(gpu_common.hip_model(T), starts, goals, env_id="EnvHighways2D", n_samples=B)      # noqa: E731
    s = make()
    lines = torch.from_numpy(synth.straight_line_paths(starts, goals, 64)).cuda()
    state = torch.cat([lines, torch.zeros_like(lines)], -1)
    X = s.dataset.normalize_trajectories(state)[:, None].expand(3, B, 64, 4).reshape(-1, 64, 4).contiguous()
    res = s.plan_rounds_seeded(X, max_rounds=1, seed=seed)
    hand = make()
    hand.set_other_paths(lines)
    trajs = hand.sample_local(X, seed=seed)
    best = hand.best_paths(trajs, lines)
    assert res.n_rounds == 1 and torch.equal(res.trajs, trajs) and torch.equal(res.paths_local, best)
    from_noise = make().plan(max_rounds=1, seed=seed)
    assert not torch.equal(from_noise.trajs, trajs)
    none = make().plan_rounds_seeded(None, max_rounds=1, seed=seed)
    assert torch.equal(none.trajs, from_noise.trajs) and torch.equal(none.paths_local, from_noise.paths_local)
    # later rounds are what they are without it: round 1 from noise, or with local_rounds from round 0
    two = make().plan_rounds_seeded(X, max_rounds=2, seed=seed, local_rounds=True)
    if two.n_rounds == 2:
        hand.set_other_paths(best)
        assert torch.equal(two.trajs, hand.sample_local(trajs, seed=seed + 1))
    for bad in (X[:-1], X[:, :32], X.double(), X.cpu(), X.transpose(0, 1).contiguous().transpose(0, 1), "X"):
        with pytest.raises(ValueError, match="init_trajs"):
            make().plan_rounds_seeded(bad, max_rounds=1, seed=seed)


# ---- 4. a seeded fleet crosses the world ------------------------------------------------------------------------------------------------------------------
def test_seeded_fleet_crosses_the_door_world(crossing):     # noqa: F811
    """clear_min: every final support point of a seed is either a point that an iteration accepted, whose texel value exceeded the
    clearance when it was accepted (the texture does not change), or still the centre of its sample cell, a cell of the walk and so
    routable, value > clearance, or one of the two ends, which lie in the start cell and the sub-goal cell of the walk, routable as well
    (the texel of a point in a cell is that cell).  clear_min is the least of these 64 values: it exceeds the clearance, strictly."""
    import gpu_common
    from mmd_amd.world import WorldRobotSampler
    fleet0, plain, starts, goals, _ = crossing
    model = gpu_common.hip_model(W.T)
    kw = dict(reach=W.REACH, max_steps=W.MAX_STEPS, n_samples=W.B)
    before = len(map_textures._TEXTURES)
    fleet = F.WorldFleet(model, W.WORLD, starts, goals, seed_epochs=True, **kw)
    result = fleet.run(max_rounds=W.ROUNDS, seed=W.SEED)
    assert len(map_textures._TEXTURES) == before and not any(W.WORLD + "@" in m for key in map_textures._TEXTURES for m in key[0])
    assert result.arrived.tolist() == [True] * 4 and len(result.epochs) == len(plain.epochs)
    for e, (seeded, unseeded) in enumerate(zip(result.epochs, plain.epochs)):                # the targets depend on the pinned ends only
        assert np.array_equal(seeded["summary"], unseeded["summary"]) and W.same_bits(seeded["offsets"], unseeded["offsets"]), e
        assert "clear_min" not in unseeded and seeded["clear_min"].shape == (4,) and seeded["clear_min"].dtype == np.float32
        assert (seeded["clear_min"] > np.float32(fleet.clearance)).all(), (e, seeded["clear_min"])
    paths = result.paths.cpu().numpy()
    n_epochs = len(result.epochs)
    assert paths.shape == (4, 64 * n_epochs, 2) and np.isfinite(paths).all()
    assert W.same_bits(paths[:, 0], starts), "the first epoch begins at the starts"
    for e in range(1, n_epochs):
        assert W.same_bits(paths[:, 64 * e], paths[:, 64 * e - 1]), f"epoch {e} does not begin where epoch {e - 1} ended"
    assert W.same_bits(paths[:, -1], goals), "a robot's last point is not its goal"
    again = F.WorldFleet(model, W.WORLD, starts, goals, seed_epochs=True, **kw).run(max_rounds=W.ROUNDS, seed=W.SEED)
    assert W.same_bits(again.paths, result.paths), "two seeded runs with one seed differ"
    assert not W.same_bits(plain.paths, result.paths), "the seeded run is the unseeded one"
    # every epoch by hand: the targets, the seeds, the sampler's rounds from them
    other = F.WorldFleet(model, W.WORLD, starts, goals, seed_epochs=True, **kw)
    tex = map_textures.device_world_texture(W.WORLD, "cuda")
    lo, hi = E.world_map_limits(W.WORLD)
    positions = starts
    for e, epoch in enumerate(result.epochs):
        targets = other.epoch_targets(positions)
        assert np.array_equal(targets.summary, epoch["summary"]) and targets.samples.shape == (4, 64, 2) and targets.samples.is_cuda
        seeds, clear_min = F.device_window_seeds(tex, lo, hi, targets.samples, dev(targets.origins, np.int32), dev(targets.summary, np.int32),
                                                 400, positions, targets.points, other.clearance, 64)
        assert W.same_bits(clear_min, epoch["clear_min"])
        assert W.same_bits(seeds[:, 0, :2], positions) and W.same_bits(seeds[:, 63, :2], targets.points)
        sampler = WorldRobotSampler(model, positions, targets.points, targets.offsets, env_id=W.WORLD, n_samples=W.B)
        res = sampler.plan_rounds_seeded(sampler.trajs_from_global(seeds), paths_local=seeds[..., :2].contiguous(), local_rounds=True,
                                  max_rounds=W.ROUNDS, seed=W.SEED + e)
        assert map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), "cuda") is True
        assert W.same_bits(res.paths_local, result.paths[:, 64 * e:64 * e + 64]), f"epoch {e} is not the hand-built sequence"
        assert list(res.conflict_counts) == epoch["conflict_counts"]
        positions = res.paths_local[:, -1].cpu().numpy()
    # one robot's samples and seed against the definitions, on the fields and the texture the fleet holds
    t0 = other.epoch_targets(starts)
    r, f = 0, int(other.fields[0])
    want = F.window_goal_samples(other.dist[f].cpu().numpy(), W.START_CELLS[r], other.field_goals[f], W.REACH, W.MAX_STEPS, 400)
    assert np.array_equal(t0.samples[r].cpu().numpy(), want[5]) and want[2] >= 64
    # seed_epochs=False, spelled out, is the run without the option
    off = F.WorldFleet(model, W.WORLD, starts, goals, seed_epochs=False, **kw)
    assert off.epoch_targets(starts).samples is None
    run = off.run(max_rounds=W.ROUNDS, seed=W.SEED)
    assert W.same_bits(run.paths, plain.paths) and [e["conflict_counts"] for e in run.epochs] == [e["conflict_counts"] for e in plain.epochs]
    assert all("clear_min" not in e for e in run.epochs)


def test_trajs_from_global_and_refusals(crossing):           # noqa: F811
    import gpu_common
    from mmd_amd.world import WorldRobotSampler
    _, _, starts, goals, _ = crossing
    model = gpu_common.hip_model(W.T)
    fleet = F.WorldFleet(model, W.WORLD, starts, goals, reach=W.REACH, max_steps=W.MAX_STEPS, n_samples=W.B, seed_epochs=True)
    targets = fleet.epoch_targets(starts)
    sampler = WorldRobotSampler(model, starts, targets.points, targets.offsets, env_id=W.WORLD, n_samples=W.B)
    try:
        seeds = torch.zeros(4, 64, 4, device="cuda")
        seeds[..., :2] = torch.from_numpy(starts).cuda()[:, None]
        seeds[1, :, 2] = 1e6                                                                 # a velocity beyond the normaliser's limits
        got = sampler.trajs_from_global(seeds)
        assert got.shape == (16, 64, 4) and got.is_contiguous() and got.dtype == torch.float32
        local = seeds.clone()
        local[..., :2] -= torch.from_numpy(targets.offsets).cuda()[:, None]
        want = torch.clip(sampler.dataset.normalize_trajectories(local), -1, 1)
        for r in range(4):
            for b in range(W.B):
                assert torch.equal(got[r * W.B + b], want[r]), (r, b)
        assert float(got.abs().max()) <= 1.0 and float(got[4, 0, 2]) == 1.0
        assert W.same_bits(sampler.unnormalize(got)[::W.B, 0, :2] + torch.from_numpy(targets.offsets).cuda(), starts)      # exact: the fixture's docstring
        for bad in (seeds[:3], seeds[..., :2], seeds.double()):
            with pytest.raises(ValueError, match="trajs_from_global"):
                sampler.trajs_from_global(bad)
        with pytest.raises(ValueError, match="init_trajs"):
            sampler.plan_rounds_seeded(got[:-1], max_rounds=1)
    finally:
        map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), "cuda")
    for kw in (dict(smooth_iters=-1), dict(n_denoising_steps=0), dict(n_noising_steps=-1)):
        with pytest.raises(ValueError):
            F.WorldFleet(model, W.WORLD, starts, goals, seed_epochs=True, **kw)
