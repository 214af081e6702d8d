"""-m gpu: sub-goals kept apart (mmd_amd.world_fleet.subgoals_apart).  mmd_grid_window_goals_apart is the numpy definition word for word
after every number of sweeps -- on the batches of 24 robots of world_fleet_apart_model, the written-out chain, a batch that holds every
status and one of more than 64 robots with walks of more than 64 cells --, with guard words round every output and the workspace; a
continuation equals the one-shot call; its error returns leave the outputs alone.  End to end, a fleet of 4 robots on a world of 800 x 400
cells whose plain sub-goals collide keeps every epoch's pinned ends RR_MARGIN apart."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import world_fleet_apart_model as A                              # noqa: E402
import world_fleet_model as M                                    # noqa: E402
from mmd_amd import _lib, environments as E, world_fleet as F    # noqa: E402
from mmd_amd.multi_agent import RR_MARGIN                        # noqa: E402
from mmd_amd.world_routes import ROUTE_OK, ROUTE_OUTSIDE, ROUTE_STUCK, ROUTE_UNREACHED      # noqa: E402

GUARD = 0x5A5A5A5A
PAD = 16                         # guard words in front of, between and behind the buffers (a multiple of 4: 16-byte alignment is kept)
NAMES = ("cells", "origins", "summary", "extra", "changed", "samples")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


class Raw:
    """mmd_grid_window_goals_apart on numpy inputs, into one buffer whose every word outside the outputs and the workspace is a guard"""

    def __init__(self, dist, starts, which, goals, reach, max_steps, sep, window, with_samples=True):
        self.dist = torch.from_numpy(np.array(dist, dtype=np.int32)).cuda()              # (a copy: the shared fields are read-only)
        self.starts = torch.tensor(np.asarray(starts).reshape(-1, 2), dtype=torch.int32).cuda()
        self.which = torch.tensor(np.asarray(which).reshape(-1), dtype=torch.int32).cuda()
        self.goals = torch.tensor(np.asarray(goals).reshape(-1, 2), dtype=torch.int32).cuda()
        self.n = n = self.starts.shape[0]
        self.args = (reach, max_steps, window, sep)
        self.with_samples = with_samples
        self.work_bytes = int(_lib.load().mmd_grid_window_apart_work_bytes(n, max_steps))
        assert self.work_bytes >= n * (8 * (max_steps + 1) + 16) and self.work_bytes % 4 == 0
        sizes = dict(cells=2 * n, origins=2 * n, summary=4 * n, extra=2 * n, changed=1, samples=128 * n, work=self.work_bytes // 4)
        self.at, word = {}, PAD
        for name, size in sizes.items():
            self.at[name] = (word, size)
            word += -(-size // 4) * 4 + PAD                  # every buffer starts on a multiple of 4 words
        self.buf = torch.full((word,), GUARD, dtype=torch.int32, device="cuda")
        self.is_guard = np.ones(word, bool)
        for name, (first, size) in self.at.items():
            if name != "samples" or with_samples:
                self.is_guard[first:first + size] = False

    def call(self, restart, n_sweeps):
        p = lambda name: C.c_void_p(self.buf.data_ptr() + 4 * self.at[name][0])          # noqa: E731
        reach, max_steps, window, sep = self.args
        _lib.launch("mmd_grid_window_goals_apart", self.buf, C.c_void_p(self.dist.data_ptr()), self.dist.shape[1], self.dist.shape[2],
                    self.dist.shape[0], C.c_void_p(self.starts.data_ptr()), C.c_void_p(self.which.data_ptr()),
                    C.c_void_p(self.goals.data_ptr()), self.n, reach, max_steps, window, sep, restart, n_sweeps, p("work"), self.work_bytes,
                    p("cells"), p("origins"), p("summary"), p("extra"), p("samples") if self.with_samples else None, p("changed"))
        torch.cuda.synchronize()
        words = self.buf.cpu().numpy()
        assert (words[self.is_guard] == GUARD).all(), "wrote outside the outputs and the workspace"
        cut = lambda name, *shape: words[self.at[name][0]:self.at[name][0] + self.at[name][1]].reshape(shape).copy()      # noqa: E731
        n = self.n
        return (cut("cells", n, 2), cut("origins", n, 2), cut("summary", n, 4), cut("extra", n, 2), int(cut("changed", 1)[0]),
                cut("samples", n, 64, 2) if self.with_samples else None)


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if name == "changed":
            assert g == w, f"{what}: changed {g}, definition {w}"
        elif g is not None:
            assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
            bad = np.flatnonzero((g != w).reshape(len(w), -1).any(1))
            assert bad.size == 0, f"{what}: {name} differ in {bad.size} of {len(w)} queries, first {int(bad[0])}: device " \
                                  f"{g[bad[0]].tolist()} definition {w[bad[0]].tolist()}"


def every_status_batch():
    """robots that walk towards one another among queries of every other status (test_world_fleet_apart_host.py has the same by hand)"""
    stuck, goal0, _ = M.unconverged_field()
    walled = M.fields(M.door_grid(door=(0, 0)), [(25, 5)])
    dist = np.concatenate([stuck, M.fields(M.open_grid(), [(20, 15), (22, 15)]), walled])
    goals = [goal0, (20, 15), (22, 15), (25, 5)]
    starts = [(14, 15), (-1, 3), (26, 15), (15, 15), (10, 12), (16, 15), (28, 15), (20, 15), (14, 16)]
    which = [1, 1, 1, 3, 0, 7, 2, 1, 1]
    return dist, np.asarray(starts, np.int32), np.asarray(which, np.int32), np.asarray(goals, np.int32)


def wide_batch():
    """70 robots on a serpentine of 130 x 70 cells with reach 31 on a window of 64: more robots than a wave has lanes, walks of more than
    64 cells, and starts drawn with no regard to one another, so that some are in conflict from the outset"""
    routable = M.serpentine_grid((130, 70), pitch=16, gap=5)
    goals = [(125, 3), (3, 3), (70, 35)]
    dist = M.fields(routable, goals)
    rng = np.random.Generator(np.random.PCG64(5))
    free = np.argwhere(routable)
    starts = free[rng.choice(len(free), 70, replace=False)].astype(np.int32)
    return dist, starts, rng.integers(0, 3, 70).astype(np.int32), np.asarray(goals, np.int32)


BATCHES = {
    # name: (the batch, (reach, max_steps, sep, window))
    "open": (lambda: A.batch("open"), (M.REACH, 100, A.SEP, M.WINDOW)),
    "door": (lambda: A.batch("door"), (M.REACH, 100, A.SEP, M.WINDOW)),
    "serpentine": (lambda: A.batch("serpentine"), (M.REACH, 100, A.SEP, M.WINDOW)),
    "chain": (A.chain, (M.REACH, 100, A.SEP, M.WINDOW)),
    "every status": (every_status_batch, (M.REACH, 100, A.SEP, M.WINDOW)),
    "wide": (wide_batch, (31, 200, 9, 64)),
}


# ---- 1. the kernels are the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BATCHES))
def test_kernel_is_the_definition_after_every_sweep(name):
    make, (reach, max_steps, sep, window) = BATCHES[name]
    dist, starts, which, goals = make()
    want = lambda s: F.subgoals_apart_sweeps(dist, starts, which, goals, reach, max_steps, sep, s, window, with_samples=True)      # noqa: E731
    raw = Raw(dist, starts, which, goals, reach, max_steps, sep, window)
    wants, s = [], 0
    while True:                                              # s = 0, 1, 2, .. up to the sweep that reads changed == 0, and one beyond
        wants.append(want(s))
        assert_same(raw.call(1, s), wants[s], f"{name}, one call of {s} sweeps")
        if s > 0 and wants[s - 1][4] == 0:
            break
        s += 1
        assert s <= len(starts) + 2
    fixed = s - 1                                            # the first count of sweeps that reads changed == 0
    definition = F.subgoals_apart_samples(dist, starts, which, goals, reach, max_steps, sep, window)
    assert_same(raw.call(1, fixed)[:4] + (0, raw.call(0, 0)[5]), definition[:4] + (0, definition[4]), f"{name}, the fixed point")
    # continuations: sweep by sweep, and in uneven pieces with calls of no sweep in between
    raw.call(1, 0)
    for k in range(1, fixed + 1):
        assert_same(raw.call(0, 1), wants[k], f"{name}, sweep {k} as a continuation")
        assert_same(raw.call(0, 0), wants[k], f"{name}, sweep {k} emitted again")
    raw.call(1, 1)
    assert_same(raw.call(0, fixed - 1), wants[fixed], f"{name}, 1 + {fixed - 1} sweeps")
    # without samples the other outputs are alike, and the samples' words stay guards (Raw.call checks them)
    bare = Raw(dist, starts, which, goals, reach, max_steps, sep, window, with_samples=False)
    assert_same(bare.call(1, fixed), wants[fixed], f"{name}, samples = NULL")
    if name == "chain":
        assert fixed == 6 and [w[2][:, 0].tolist() for w in wants[1:7]] == A.CHAIN_K and [w[4] for w in wants[1:7]] == A.CHAIN_CHANGED
    elif name == "every status":
        assert set(wants[0][2][:, 2].tolist()) == {ROUTE_OK, ROUTE_UNREACHED, ROUTE_STUCK, ROUTE_OUTSIDE}
        assert (wants[fixed][2][:, 0] < wants[fixed][3][:, 0]).any()
    elif name == "wide":
        assert len(starts) > 64 and wants[0][3][:, 0].max() >= 64 and fixed >= 3
        k, walked, clear = wants[fixed][2][:, 0], wants[fixed][3][:, 0], wants[fixed][3][:, 1]
        assert ((k > 0) & (walked - k >= 64)).any() and (clear == 0).any() and (walked - k > 0).sum() >= 8      # a choice in a later chunk of 64
    else:
        assert fixed >= 3


def test_device_subgoals_apart():
    dist, starts, which, goals = A.chain()
    dist_d = torch.from_numpy(dist.copy()).cuda()
    want = F.subgoals_apart_samples(dist, starts, which, goals, M.REACH, 100, A.SEP, M.WINDOW)
    got = F.device_subgoals_apart(dist_d, starts, which, goals, M.REACH, 100, A.SEP, M.WINDOW, sweeps=4, with_samples=True)
    assert got[5] == 8 and all(t.is_cuda and t.dtype == torch.int32 for t in got[:5])      # 4 sweeps read changed = 1, 4 more read 0
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[:5], want))
    for sweeps, run in ((1, 6), (6, 6), (5, 9), (9, 9), (100, 9)):            # at most n + 1 = 9 in all, the first call included
        got = F.device_subgoals_apart(dist_d, starts, which, goals, M.REACH, 100, A.SEP, M.WINDOW, sweeps=sweeps)
        assert len(got) == 5 and got[4] == run, (sweeps, got[4])
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[:4], want))
    dist, starts, which, goals = A.batch("door")
    got = F.device_subgoals_apart(torch.from_numpy(dist.copy()).cuda(), starts, which, goals, M.REACH, 100, A.SEP, M.WINDOW)
    assert got[4] == 4 and all(np.array_equal(g.cpu().numpy(), w) for g, w in
                               zip(got[:4], F.subgoals_apart(dist, starts, which, goals, M.REACH, 100, A.SEP, M.WINDOW)))
    for kw in (dict(sep=0), dict(sep=1025), dict(sweeps=0), dict(max_steps=4096), dict(reach=6), dict(starts=starts[:0], fields=which[:0])):
        with pytest.raises(ValueError):
            F.device_subgoals_apart(dist_d, **dict(dict(starts=starts[:8], fields=which[:8], goals=goals[:8], reach=M.REACH, max_steps=100,
                                                        sep=A.SEP, window=M.WINDOW), **kw))


def test_error_returns_leave_the_outputs_alone():
    lib = _lib.load()
    dist = torch.zeros(2, 40, 30, dtype=torch.int32, device="cuda")
    ints = torch.zeros(64, dtype=torch.int32, device="cuda")
    need = int(lib.mmd_grid_window_apart_work_bytes(7, 9))
    out = torch.full((1536 + need // 4,), GUARD, dtype=torch.int32, device="cuda")
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * k)                                  # noqa: E731
    good = dict(dist=p(dist), nx=40, ny=30, n_fields=2, starts=p(ints), field=p(ints, 32), goals=p(ints, 48), n=7, reach=5, max_steps=9,
                window=12, sep=3, restart=1, n_sweeps=2, work=p(out, 1536), work_bytes=need, cells=p(out, 16), origins=p(out, 64),
                summary=p(out, 128), extra=p(out, 192), samples=p(out, 256), changed=p(out, 1280))
    order = ("dist", "nx", "ny", "n_fields", "starts", "field", "goals", "n", "reach", "max_steps", "window", "sep", "restart", "n_sweeps", "work",
             "work_bytes", "cells", "origins", "summary", "extra", "samples", "changed")
    stream = C.c_void_p(_lib.raw_stream())
    call = lambda **kw: lib.mmd_grid_window_goals_apart(*(dict(good, **kw)[k] for k in order), stream)      # noqa: E731
    for kw in (dict(nx=0), dict(nx=2049), dict(ny=0), dict(n_fields=-1), dict(n=-1), dict(n=np.iinfo(np.int32).max), dict(reach=0), dict(reach=6),
               dict(max_steps=0), dict(max_steps=4096), dict(window=31), dict(window=0), dict(sep=0), dict(sep=1025), dict(n_sweeps=-1),
               dict(dist=None), dict(goals=None), dict(starts=None), dict(field=None), dict(work=None), dict(work=p(out, 1538)),
               dict(work_bytes=need - 1), dict(cells=None), dict(origins=None), dict(summary=None), dict(extra=None), dict(changed=None)):
        assert call(**kw) == 2 and lib.mmd_last_error().startswith(b"mmd_grid_window_goals_apart:"), (kw, lib.mmd_last_error())
    assert call(n=0) == 0 and call(n=0, dist=None, work=None, summary=None) == 0
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call, or one of no queries, wrote"
    assert call() == 0                                        # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    words = out.cpu().numpy()
    # all seven at cell (0, 0) of a field of zeros: arrived, nobody walks, and the starts are in conflict
    assert not words[16:30].any() and not words[64:78].any() and words[128:156].reshape(7, 4).tolist() == [[0, 0, ROUTE_OK, 1]] * 7
    assert words[192:206].reshape(7, 2).tolist() == [[0, 0]] * 7 and not words[256:256 + 7 * 128].any() and words[1280] == 0
    rest = np.concatenate([words[:16], words[30:64], words[78:128], words[156:192], words[206:256], words[256 + 7 * 128:1280], words[1281:1536]])
    assert (rest == GUARD).all()


# ---- 2. a fleet whose plain sub-goals collide ------------------------------------------------------------------------------------------------------
WORLD = "FleetApartWorld"
SHAPE = (800, 400)
ORIGIN = (2.0, 2.0)
T, B, ROUNDS, SEED = 25, 4, 2, 31
REACH, MAX_STEPS = 120, 360
# robot 1 stands on its goal; robot 0's walk of 120 cells ends 10 cells from it, on the way to a goal beyond it; robot 2 comes through the
# door towards both; robot 3 keeps to itself
START_CELLS = np.asarray([(190, 200), (300, 200), (560, 200), (600, 60)])
GOAL_CELLS = np.asarray([(340, 200), (300, 200), (260, 200), (640, 90)])


def world_bitmap():
    """A wall of 4 cells across the world's middle, with one door of 120 cells (the clearance of 0.16 = 32 cells leaves 56 of them)"""
    occ = np.zeros(SHAPE, np.uint8)
    occ[398:402, :] = 1
    occ[398:402, 140:260] = 0
    return occ


def points_in(cells, shift):
    """float32 global points inside the cells, `shift` off their centres"""
    return (np.asarray(ORIGIN) + (np.asarray(cells) + 0.5) * E.SDF_CELL_SIZE + shift).astype(np.float32)


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def least_distance(points):
    p = np.asarray(points, np.float64)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    return d[np.triu_indices(len(p), 1)].min()


@pytest.fixture(scope="module")
def apart_world():
    """(model, starts, goals, the run with separation = 23) on the door world (test_gpu_world_fleet.py argues why its ends can be held to
    the bit: the world's lower corner at (2, 2) makes every frame operation exact)"""
    import gpu_common
    E.register_world_map(WORLD, world_bitmap(), origin=ORIGIN)
    model = gpu_common.hip_model(T)
    starts, goals = points_in(START_CELLS, 0.001), points_in(GOAL_CELLS, -0.0015)
    fleet = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, separation=F.SUBGOAL_SEPARATION)
    yield model, starts, goals, fleet, fleet.run(max_rounds=ROUNDS, seed=SEED)
    E.unregister_world_map(WORLD)


def test_fleet_keeps_every_epochs_ends_apart(apart_world):
    model, starts, goals, fleet, result = apart_world
    dist = fleet.dist.cpu().numpy()
    # the premise, on the fleet's own fields: the plain sub-goals of the first epoch put two robots closer than 23 cells
    plain = F.window_goals(dist, START_CELLS, fleet.fields, fleet.field_goals, REACH, MAX_STEPS, 400)
    assert (plain[2][:, 2] == ROUTE_OK).all() and A.apart(plain[0]) < 23 * 23
    assert A.apart(START_CELLS) >= 23 * 23 and A.apart(GOAL_CELLS) >= 23 * 23
    n_epochs = len(result.epochs)
    assert n_epochs >= 2 and result.paths.shape == (4, 64 * n_epochs, 2) and bool(torch.isfinite(result.paths).all())
    paths = result.paths.cpu().numpy()
    assert same_bits(paths[:, 0], starts)
    at, lo_hi = START_CELLS.astype(np.int32), E.world_map_limits(WORLD)
    for e, epoch in enumerate(result.epochs):
        ends = paths[:, 64 * e + 63]
        print(f"epoch {e}: least distance of two pinned ends {least_distance(ends):.6f}, summary {epoch['summary'].tolist()}, "
              f"held back {epoch['held_back'].tolist()}, sweeps {epoch['sweeps']}")
        assert least_distance(ends) >= RR_MARGIN, f"epoch {e}: two pinned ends closer than RR_MARGIN"
        if e:
            assert same_bits(paths[:, 64 * e], paths[:, 64 * e - 1]), f"epoch {e} does not begin where epoch {e - 1} ended"
        cells, _, summary, extra = F.subgoals_apart(dist, at, fleet.fields, fleet.field_goals, REACH, MAX_STEPS, F.SUBGOAL_SEPARATION, 400)
        assert np.array_equal(epoch["summary"], summary) and np.array_equal(epoch["held_back"], extra[:, 0] - summary[:, 0]), e
        assert (extra[:, 1] == 1).all() and A.apart(cells) >= 23 * 23 and 1 <= epoch["sweeps"] <= 5 and epoch["stalled"] is False
        for r in range(4):
            end = goals[r] if summary[r, 3] else F.cell_centres(cells[r], lo_hi[0], lo_hi[1], SHAPE)
            assert same_bits(ends[r], np.asarray(end, np.float32)), (e, r)
        at = cells
    assert any(epoch["held_back"].any() for epoch in result.epochs)
    assert result.arrived.tolist() == [True] * 4 and same_bits(paths[:, -1], goals)
    assert (result.epochs[-1]["summary"][:, 3] == 1).all()
    # the same run again, to the bit
    again = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, separation=23).run(max_rounds=ROUNDS, seed=SEED)
    assert same_bits(again.paths, result.paths)
    assert [e["conflict_counts"] for e in again.epochs] == [e["conflict_counts"] for e in result.epochs]
    capped = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, separation=23).run(1, ROUNDS, SEED)
    assert len(capped.epochs) == 1 and same_bits(capped.paths, result.paths[:, :64]) and not capped.arrived.all()


def test_seeded_fleet_keeps_its_ends_apart(apart_world):
    model, starts, goals, fleet, result = apart_world
    seeded = F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, separation=23, seed_epochs=True)
    res = seeded.run(max_rounds=ROUNDS, seed=SEED)
    assert len(res.epochs) == len(result.epochs) and res.arrived.all()
    paths = res.paths.cpu().numpy()
    for e, epoch in enumerate(res.epochs):
        assert np.array_equal(epoch["summary"], result.epochs[e]["summary"])              # the same targets, seeded or not
        assert least_distance(paths[:, 64 * e + 63]) >= RR_MARGIN, e
        assert epoch["clear_min"].shape == (4,) and (epoch["clear_min"] > seeded.clearance).all(), (e, epoch["clear_min"])
    assert same_bits(paths[:, -1], goals)


def test_the_default_is_untouched(apart_world):
    model, starts, goals, fleet, result = apart_world
    kw = dict(reach=REACH, max_steps=MAX_STEPS, n_samples=B)
    plain, none = F.WorldFleet(model, WORLD, starts, goals, **kw), F.WorldFleet(model, WORLD, starts, goals, separation=None, **kw)
    assert plain.separation is None and none.separation is None
    a, b = plain.run(2, ROUNDS, SEED), none.run(2, ROUNDS, SEED)
    assert same_bits(a.paths, b.paths) and len(a.epochs) == len(b.epochs) == 2
    for ea, eb in zip(a.epochs, b.epochs):
        assert ea["conflict_counts"] == eb["conflict_counts"] and np.array_equal(ea["summary"], eb["summary"])
        assert set(ea) == set(eb) == {"conflict_counts", "summary", "offsets"}            # none of the separation's entries
    # and its first sub-goals are the plain ones, 10 cells apart where the separation held robot 0 back
    targets = plain.epoch_targets(starts)
    assert targets.extra is None and targets.sweeps is None and A.apart(targets.cells) < 23 * 23
    assert not np.array_equal(targets.summary, result.epochs[0]["summary"])
