"""-m gpu: standing robots step aside (mmd_amd.world_fleet.subgoals_aside).  mmd_grid_window_goals_aside is the numpy definition word for
word at its fixed point -- on the written-out cases of world_fleet_aside_model, crowds of 65, 130 and 600 robots, walks of hundreds of cells
that wind inside a side box, the largest and the smallest box --, with guard words round every output and both workspaces, and the apart
workspace left as it was; every epoch of whole runs through device_subgoals_aside; its error returns leave the outputs alone.  End to
end, a fleet of 4 on a world of 800 x 400 cells where a robot that stands on its goal in a doorway holds another back: with
step_aside=True the run arrives, without it it stalls, and persistent=True gives the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import world_fleet_apart_model as A                              # noqa: E402
import world_fleet_aside_model as S                              # noqa: E402
import world_fleet_model as M                                    # noqa: E402
from mmd_amd import _lib, environments as E, world_fleet as F    # noqa: E402
from mmd_amd.fleet_subgoals import _walk                         # noqa: E402
from mmd_amd.multi_agent import RR_MARGIN                        # noqa: E402
from mmd_amd.world_routes import ROUTE_OK                        # noqa: E402

GUARD = 0x5A5A5A5A
PAD = 16                         # guard words in front of, between and behind the buffers (a multiple of 4: 16-byte alignment is kept)
NAMES = ("cells", "origins", "summary", "extra", "aside")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()


class Raw:
    """mmd_grid_window_goals_apart to its fixed point and then mmd_grid_window_goals_aside on numpy inputs, into one buffer whose every
    word outside the outputs and the two workspaces is a guard"""

    def __init__(self, dist, starts, which, goals, args):
        self.dist = torch.from_numpy(np.array(dist, dtype=np.int32)).cuda()              # (a copy: the shared fields are read-only)
        self.starts = torch.tensor(np.asarray(starts).reshape(-1, 2), dtype=torch.int32).cuda()
        self.which = torch.tensor(np.asarray(which).reshape(-1), dtype=torch.int32).cuda()
        self.goals = torch.tensor(np.asarray(goals).reshape(-1, 2), dtype=torch.int32).cuda()
        self.n = n = self.starts.shape[0]
        self.args = args
        lib = _lib.load()
        self.apart_bytes, self.work_bytes = int(lib.mmd_grid_window_apart_work_bytes(n, args[1])), int(lib.mmd_grid_window_aside_work_bytes(n))
        assert self.work_bytes >= 36 * n and self.work_bytes % 4 == 0 and self.apart_bytes % 4 == 0
        sizes = dict(cells=2 * n, origins=2 * n, summary=4 * n, extra=2 * n, aside=2 * n, changed=1, apart=self.apart_bytes // 4,
                     work=self.work_bytes // 4)
        self.at, word = {}, PAD
        for name, size in sizes.items():
            self.at[name] = (word, size)
            word += -(-size // 4) * 4 + PAD                  # every buffer starts on a multiple of 4 words
        self.buf = torch.full((word,), GUARD, dtype=torch.int32, device="cuda")
        self.is_guard = np.ones(word, bool)
        for first, size in self.at.values():
            self.is_guard[first:first + size] = False
        self.p = lambda name: C.c_void_p(self.buf.data_ptr() + 4 * self.at[name][0])
        # phase 1, into the same outputs: n + 1 sweeps always read changed == 0
        reach, max_steps, sep, _, _, window = args
        _lib.launch("mmd_grid_window_goals_apart", self.buf, C.c_void_p(self.dist.data_ptr()), self.dist.shape[1], self.dist.shape[2],
                    self.dist.shape[0], C.c_void_p(self.starts.data_ptr()), C.c_void_p(self.which.data_ptr()), C.c_void_p(self.goals.data_ptr()),
                    n, reach, max_steps, window, sep, 1, n + 1, self.p("apart"), self.apart_bytes, self.p("cells"), self.p("origins"),
                    self.p("summary"), self.p("extra"), None, self.p("changed"))
        torch.cuda.synchronize()
        words = self.buf.cpu().numpy()
        assert words[self.at["changed"][0]] == 0
        self.apart_words = self.cut(words, "apart").copy()

    def cut(self, words, name, *shape):
        return words[self.at[name][0]:self.at[name][0] + self.at[name][1]].reshape(shape or (-1,)).copy()

    def call(self, restart, n_sweeps):
        """-> (cells, origins, summary, extra, aside, changed)"""
        reach, max_steps, sep, aside_reach, aside_steps, window = self.args
        p = self.p
        _lib.launch("mmd_grid_window_goals_aside", self.buf, C.c_void_p(self.dist.data_ptr()), self.dist.shape[1], self.dist.shape[2],
                    self.dist.shape[0], C.c_void_p(self.which.data_ptr()), self.n, reach, max_steps, window, sep, aside_reach, aside_steps,
                    restart, n_sweeps, p("apart"), self.apart_bytes, p("work"), self.work_bytes, p("cells"), p("origins"), p("summary"),
                    p("extra"), p("aside"), p("changed"))
        torch.cuda.synchronize()
        words = self.buf.cpu().numpy()
        assert (words[self.is_guard] == GUARD).all(), "wrote outside the outputs and the workspaces"
        assert np.array_equal(self.cut(words, "apart"), self.apart_words), "wrote the apart workspace"
        n = self.n
        return (self.cut(words, "cells", n, 2), self.cut(words, "origins", n, 2), self.cut(words, "summary", n, 4), self.cut(words, "extra", n, 2),
                self.cut(words, "aside", n, 2), int(self.cut(words, "changed")[0]))


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(1))
        assert bad.size == 0, f"{what}: {name} differ in {bad.size} of {len(w)} queries, first {int(bad[0])}: device " \
                              f"{g[bad[0]].tolist()} definition {w[bad[0]].tolist()}"


def batch_case(grid):
    return A.batch(grid) + (S.ARGS,)


CASES = dict(S.HOST_CASES)
CASES.update({
    "open": lambda: batch_case("open"), "door": lambda: batch_case("door"), "serpentine": lambda: batch_case("serpentine"),
    "65 robots": lambda: S.crowd(65, 1), "130 robots": lambda: S.crowd(130, 2),
    # the side kernel stages blockers 256 at a time: three chunks, with yielders and the robots they clear in different ones
    "600 robots": lambda: S.big_crowd(600, 3),
    # 120 x 120 and not the strip of 120 x 30: a window is at most the grid's shorter side, and reach 59 needs a window of 120
    "walk of 318 cells, reach 59": lambda: S.long_walk((120, 120), 59, 59, 120)[0],
    "aside_reach 63": lambda: S.long_walk((200, 200), 99, 63, 200)[0],
    "aside_reach 1": lambda: S.long_walk((200, 200), 99, 1, 200)[0],
})


# ---- 1. the kernels are the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_is_the_definition(name):
    dist, starts, which, goals, args = CASES[name]()
    want = F.subgoals_aside(dist, starts, which, goals, *args)
    apart = F.subgoals_apart(dist, starts, which, goals, args[0], args[1], args[2], args[5])
    raw = Raw(dist, starts, which, goals, args)
    n = len(starts)
    # before any sweep: phase 1's words, the roles, and nothing proved
    got = raw.call(1, 0)
    assert_same(got[:4], apart, f"{name}, no sweep")
    assert np.array_equal(got[4][:, 0], want[4][:, 0] & (S.HELD | S.YIELDS)) and not got[4][:, 1].any()
    assert got[5] == int((apart[2][:, 2] == ROUTE_OK).sum())
    # sweep by sweep, as continuations, to the sweep that reads changed == 0
    sweeps = 0
    while True:
        got = raw.call(0, 1)
        sweeps += 1
        if got[5] == 0:
            break
        assert sweeps <= 2 * n, f"{name}: no fixed point after {sweeps} sweeps"
    assert_same(got, want, f"{name}, the fixed point after {sweeps} sweeps")
    assert_same(raw.call(0, 0), want, f"{name}, emitted again")
    again = raw.call(0, 1)
    assert again[5] == 0
    assert_same(again, want, f"{name}, one sweep beyond")
    one = raw.call(1, sweeps)                                 # one call of as many sweeps
    assert one[5] == 0
    assert_same(one, want, f"{name}, one call of {sweeps} sweeps")
    if sweeps > 1:
        assert raw.call(1, sweeps - 1)[5] > 0                # the sweep before still moved
    bits = want[4][:, 0]
    print(f"{name}: {sweeps} sweeps, held {int((bits & S.HELD != 0).sum())}, yields {int((bits & S.YIELDS != 0).sum())}, "
          f"moved {int((bits & S.MOVED != 0).sum())}, released {int((bits & S.RELEASED != 0).sum())}")
    if name in ("65 robots", "130 robots"):
        assert n > 64 and (bits & S.MOVED != 0).sum() >= 8 and (bits & S.RELEASED != 0).sum() >= 8 and sweeps >= 3
        if n > 128:                                          # robots of the second and third chunk of 64 move aside and are released
            assert (np.flatnonzero(bits & S.MOVED) >= 128).any() and (np.flatnonzero(bits & S.RELEASED) >= 64).any()
    elif name == "600 robots":
        _, clears, _ = S.roles_by_hand(dist, starts, which, goals, args)
        moved, yielders = np.flatnonzero(bits & S.MOVED), np.flatnonzero(bits & S.YIELDS)
        chunks = {j: {r // 256 for r in clears[j]} for j in yielders}      # the chunks of 256 blockers in which yielder j stages walks
        assert n > 512 and len(moved) >= 40 and (bits & S.RELEASED != 0).sum() >= 40 and (moved >= 512).any() and sweeps >= 3
        # held robots yield to lower indices only, so a yielder's walks lie in its own chunk and the chunks below
        assert {(j // 256, c) for j in yielders for c in chunks[j]} >= {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)}
        assert sum(len(c) >= 2 for c in chunks.values()) >= 50 and max(len(c) for c in chunks.values()) == 3
        assert max(len(clears[j]) for j in moved) >= 2       # and some yielder that moved staged more than one walk
    elif name.startswith("walk of") or name == "aside_reach 63":
        walked = int(want[3][0, 0])
        assert walked > 256 and want[4][0].tolist() == [S.HELD | S.RELEASED, 0] and want[4][1].tolist() == [S.YIELDS | S.MOVED, 3]
        box = np.abs(np.asarray(_walk(dist[0], tuple(starts[0]), tuple(goals[0]), int(dist[0][tuple(starts[0])]), args[0], args[1])[0])
                     - starts[1]).max(1) <= args[3] + args[2]
        assert box[:256].any() and box[256:].any()           # class (d) survives the cull in more than one chunk of 256 walk cells
    elif name == "aside_reach 1":
        assert want[4][1].tolist() == [S.YIELDS, 0] and not (bits & (S.MOVED | S.RELEASED)).any()


@pytest.mark.parametrize("grid", list(A.GRIDS))
def test_every_epoch_of_whole_runs(grid):
    dist, starts, which, goals = A.batch(grid)
    dist_d = torch.from_numpy(dist.copy()).cuda()
    end, epochs = S.run_aside(dist, starts, which, goals, cap=60)
    reach, max_steps, sep, aside_reach, aside_steps, window = S.ARGS
    most = 0
    for e, (at, want) in enumerate(epochs):
        got = F.device_subgoals_aside(dist_d, at, which, goals, reach, max_steps, sep, aside_reach, aside_steps, window)
        assert len(got) == 6 and all(t.is_cuda and t.dtype == torch.int32 for t in got[:5]) and 1 <= got[5] <= 2 * len(at) + 1
        assert_same([t.cpu().numpy() for t in got[:5]], want, f"{grid}, epoch {e}")
        most = max(most, got[5])
    print(f"{grid}: {end} after {len(epochs)} epochs, at most {most} sweeps")
    assert len(epochs) >= 8


def test_device_subgoals_aside_counts_its_sweeps():
    dist, starts, which, goals, args = S.crowd(65, 1)
    dist_d = torch.from_numpy(dist.copy()).cuda()
    want = F.subgoals_aside(dist, starts, which, goals, *args)
    raw, fixed = Raw(dist, starts, which, goals, args), 1
    raw.call(1, 0)
    while raw.call(0, 1)[5]:
        fixed += 1                                           # the first count of sweeps that reads changed == 0
    assert fixed >= 3
    for sweeps in (1, 2, 4, fixed, 1000):
        got = F.device_subgoals_aside(dist_d, starts, which, goals, *args[:5], window=args[5], sweeps=sweeps)
        assert got[5] == min(-(-fixed // sweeps) * sweeps, 2 * 65 + 1), (sweeps, got[5], fixed)
        assert_same([t.cpu().numpy() for t in got[:5]], want, f"sweeps = {sweeps}")
    for kw in (dict(sep=0), dict(sweeps=0), dict(max_steps=4096), dict(reach=6), dict(aside_reach=6), dict(aside_reach=0), dict(aside_steps=0),
               dict(aside_steps=4096), dict(starts=starts[:0], fields=which[:0])):
        with pytest.raises(ValueError):
            F.device_subgoals_aside(dist_d, **dict(dict(starts=starts, fields=which, goals=goals, reach=M.REACH, max_steps=100, sep=S.SEP,
                                                        aside_reach=5, aside_steps=10, window=M.WINDOW), **kw))


def test_error_returns_leave_the_outputs_alone():
    lib = _lib.load()
    dist = torch.zeros(2, 40, 30, dtype=torch.int32, device="cuda")
    ints = torch.zeros(64, dtype=torch.int32, device="cuda")
    apart_need, need = int(lib.mmd_grid_window_apart_work_bytes(7, 9)), int(lib.mmd_grid_window_aside_work_bytes(7))
    apart = torch.zeros(apart_need // 4, dtype=torch.int32, device="cuda")               # seven queries at (0, 0), status OK, k = 0, walked 0
    out = torch.full((512 + need // 4,), GUARD, dtype=torch.int32, device="cuda")
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * k)                                  # noqa: E731
    good = dict(dist=p(dist), nx=40, ny=30, n_fields=2, field=p(ints), n=7, reach=5, max_steps=9, window=12, sep=3, aside_reach=5, aside_steps=10,
                restart=1, n_sweeps=2, apart=p(apart), apart_bytes=apart_need, work=p(out, 512), work_bytes=need, cells=p(out, 16),
                origins=p(out, 64), summary=p(out, 128), extra=p(out, 192), aside=p(out, 256), changed=p(out, 320))
    order = ("dist", "nx", "ny", "n_fields", "field", "n", "reach", "max_steps", "window", "sep", "aside_reach", "aside_steps", "restart", "n_sweeps",
             "apart", "apart_bytes", "work", "work_bytes", "cells", "origins", "summary", "extra", "aside", "changed")
    stream = C.c_void_p(_lib.raw_stream())
    call = lambda **kw: lib.mmd_grid_window_goals_aside(*(dict(good, **kw)[k] for k in order), stream)      # noqa: E731
    for kw in (dict(nx=0), dict(ny=2049), dict(n_fields=-1), dict(n=-1), dict(reach=0), dict(reach=6), dict(max_steps=0), dict(max_steps=4096),
               dict(window=31), dict(sep=0), dict(sep=1025), dict(aside_reach=0), dict(aside_reach=6), dict(aside_steps=0), dict(aside_steps=4096),
               dict(n_sweeps=-1), dict(dist=None), dict(field=None), dict(apart=None), dict(apart=p(apart, 2)), dict(apart_bytes=apart_need - 1),
               dict(work=None), dict(work=p(out, 514)), dict(work_bytes=need - 1), dict(cells=None), dict(origins=None), dict(summary=None),
               dict(extra=None), dict(aside=None), dict(changed=None)):
        assert call(**kw) == 2 and lib.mmd_last_error().startswith(b"mmd_grid_window_goals_aside:"), (kw, lib.mmd_last_error())
    assert call(n=0) == 0 and call(n=0, dist=None, work=None, summary=None) == 0
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call, or one of no queries, wrote"
    assert call() == 0                                        # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    words = out.cpu().numpy()
    # all seven stand at cell (0, 0) of a field of zeros: arrived, nobody walks, nobody is held, nobody yields
    assert not words[16:30].any() and not words[64:78].any() and words[128:156].reshape(7, 4).tolist() == [[0, 0, ROUTE_OK, 1]] * 7
    assert not words[192:206].any() and not words[256:270].any() and words[320] == 0
    rest = np.concatenate([words[:16], words[30:64], words[78:128], words[156:192], words[206:256], words[270:320], words[321:512]])
    assert (rest == GUARD).all() and not bool(apart.any())


# ---- 2. a fleet with a robot that stands in a doorway ---------------------------------------------------------------------------------------------
WORLD = "FleetAsideWorld"
SHAPE = (800, 400)
ORIGIN = (2.0, 2.0)
T, B, ROUNDS, SEED = 25, 4, 2, 31
REACH, MAX_STEPS, ASIDE_REACH, ASIDE_STEPS = 40, 360, 40, 80
# robot 1 stands on its goal in the middle of the door; robot 0's goal lies 23 cells beyond it and its walk of 40 cells ends 17 cells beyond
# it: every cell of the walk conflicts with robot 1, and the separation alone holds robot 0 for good; robots 2 and 3 keep to themselves
START_CELLS = np.asarray([(377, 200), (400, 200), (600, 60), (150, 300)])
GOAL_CELLS = np.asarray([(423, 200), (400, 200), (630, 80), (180, 320)])


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
def doorway():
    import gpu_common
    E.register_world_map(WORLD, world_bitmap(), origin=ORIGIN)
    yield gpu_common.hip_model(T), points_in(START_CELLS, 0.001), points_in(GOAL_CELLS, -0.0015)
    E.unregister_world_map(WORLD)


def fleet(doorway, **kw):
    model, starts, goals = doorway
    return F.WorldFleet(model, WORLD, starts, goals, reach=REACH, max_steps=MAX_STEPS, n_samples=B, separation=F.SUBGOAL_SEPARATION, **kw)


def test_fleet_arrives_with_the_rule_and_stalls_without_it(doorway):
    model, starts, goals = doorway
    aside = dict(step_aside=True, aside_reach=ASIDE_REACH, aside_steps=ASIDE_STEPS)
    with pytest.raises(ValueError, match="max_epochs"):
        fleet(doorway, **aside).run(max_rounds=ROUNDS, seed=SEED)
    with_rule = fleet(doorway, **aside)
    dist = with_rule.dist.cpu().numpy()
    result = with_rule.run(6, ROUNDS, SEED)
    assert result.arrived.tolist() == [True] * 4 and len(result.epochs) == 2
    paths = result.paths.cpu().numpy()
    assert same_bits(paths[:, 0], starts) and same_bits(paths[:, -1], goals)
    at, lo_hi = START_CELLS.astype(np.int32), E.world_map_limits(WORLD)
    for e, epoch in enumerate(result.epochs):
        ends = paths[:, 64 * e + 63]
        want = F.subgoals_aside(dist, at, with_rule.fields, with_rule.field_goals, REACH, MAX_STEPS, 23, ASIDE_REACH, ASIDE_STEPS, 400)
        print(f"epoch {e}: summary {epoch['summary'].tolist()}, aside {epoch['aside'].tolist()}, least distance {least_distance(ends):.6f}")
        assert np.array_equal(epoch["summary"], want[2]) and np.array_equal(epoch["aside"], want[4]), e
        assert epoch["moved_aside"] == int((want[4][:, 0] & S.MOVED != 0).sum()) and epoch["released"] == int((want[4][:, 0] & S.RELEASED != 0).sum())
        assert epoch["stalled"] is False and epoch["cycling"] is False and A.apart(want[0], 23) >= 23 * 23
        assert least_distance(ends) >= RR_MARGIN, f"epoch {e}: two pinned ends closer than RR_MARGIN"
        for r in range(4):
            end = goals[r] if want[2][r, 3] else F.cell_centres(want[0][r], lo_hi[0], lo_hi[1], SHAPE)
            assert same_bits(ends[r], np.asarray(end, np.float32)), (e, r)
        at = want[0]
    first = result.epochs[0]
    assert first["aside"].tolist() == [[S.HELD | S.RELEASED, 0], [S.YIELDS | S.MOVED, 23], [0, 0], [0, 0]]
    assert first["summary"][:2].tolist() == [[40, 6, ROUTE_OK, 0], [23, 23, ROUTE_OK, 0]] and (first["moved_aside"], first["released"]) == (1, 1)
    # without the rule robot 0 never moves
    without = fleet(doorway).run(6, ROUNDS, SEED)
    assert len(without.epochs) == 2 and without.epochs[-1]["stalled"] is True and without.arrived.tolist() == [False, True, True, True]
    assert "aside" not in without.epochs[0] and without.epochs[0]["summary"][:2].tolist() == [[0, 46, ROUTE_OK, 0], [0, 0, ROUTE_OK, 1]]
    # one sampler for the whole run, moved in place: the same bits
    kept = fleet(doorway, persistent=True, **aside).run(6, ROUNDS, SEED)
    assert same_bits(kept.paths, result.paths) and len(kept.epochs) == 2
    for a, b in zip(kept.epochs, result.epochs):
        assert a["conflict_counts"] == b["conflict_counts"] and np.array_equal(a["summary"], b["summary"]) and np.array_equal(a["aside"], b["aside"])


def test_without_step_aside_an_epoch_is_device_subgoals_aparts(doorway):
    plain = fleet(doorway, step_aside=False)
    assert plain.step_aside is False
    targets = plain.epoch_targets(doorway[1])
    got = F.device_subgoals_apart(plain.dist, START_CELLS, plain.fields, plain.field_goals, REACH, MAX_STEPS, 23, 400)
    assert targets.aside is None and targets.sweeps == got[4]
    for mine, theirs in zip((targets.cells, targets.origins, targets.summary, targets.extra), got[:4]):
        assert np.array_equal(mine, theirs.cpu().numpy())
    assert np.array_equal(targets.words.cpu().numpy(), torch.cat([t.reshape(-1) for t in got[:3]]).cpu().numpy())
