"""Per-round time of WorldRobotSampler.plan() with the framed table at its static slot bound (side A) against the all-pairs form of the
same table (side B), on one GPU.

  instances: world.random_world_instance on EnvEmpty2D, N = 128, 512, 1024, the world's side sqrt(N / 8): the density of 32 robots per
             2 x 2 tile; straight lines of the global ends as the first paths;
  side A:    neighbor_slots = constraints.framed_slot_bound(offsets, ...), the default window (limits -/+ 1.0625 x radius);
  side B:    neighbor_slots = N - 1 and an unbounded window: every other robot in every robot's table, which is what the all-pairs table
             of MultiRobotSampler amounts to in a world;
  timing:    a HIP event is recorded at every all-gather of the loop, i.e. at the start of every round and of the final report: the
             interval between two is one round as the stream sees it (report, table, sampling, pick; the host's synchronisation on the
             report's count is inside).  The two sides alternate, `--reps` times, in one process; the first pass of each warms up and is
             not counted; the median over the passes is printed per round;
  compared:  one guided step of both tables on the same input (the same active terms in other slots: the difference is the rounding of
             the step's four-accumulator slot sum), the two sides' samples of the last pass (that rounding amplified by the guided
             loop), and per side used.max(), dropped.sum() and the conflict count of every report.
T = 25 synthetic weights (random-init: no convergence is claimed or can be read off the counts; the count of round 0's report -- the
straight lines -- tells whether the instance family reaches the sparse regime).

Usage: python tools/dbg/world_rounds_ab.py [--out profiles/world_rounds.txt] [--samples 4] [--rounds 2] [--reps 3] [--table binned] [N ...]"""
import os
import sys

HERE = os.path.abspath(__file__)


def _take(args, flag, default, cast=str):
    if flag in args:
        k = args.index(flag)
        v = cast(args[k + 1])
        del args[k:k + 2]
        return v
    return default


args = sys.argv[1:]
TREE = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
OUT = _take(args, "--out", None)
B = _take(args, "--samples", 4, int)
ROUNDS = _take(args, "--rounds", 2, int)
REPS = _take(args, "--reps", 3, int)
TABLE = _take(args, "--table", "binned")
SIZES = [int(a) for a in args] or [128, 512, 1024]
sys.path.insert(0, TREE)
sys.path.insert(1, os.path.join(TREE, "tests"))

import numpy as np                                          # noqa: E402
import torch                                                # noqa: E402
from mmd_amd import multi_robot, synth, world                      # noqa: E402
from mmd_amd.constraints import framed_slot_bound           # noqa: E402
from mmd_amd.environments import LIMITS                     # noqa: E402
import gpu_common                                           # noqa: E402

T = 25
UNBOUNDED = ((-1e30, -1e30), (1e30, 1e30))


class RoundClock:
    """an event at every all-gather of the loop"""

    def __init__(self):
        self.events, self.gather = [], multi_robot.all_gather_paths

    def __enter__(self):
        def gather(*a, **kw):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.events.append(e)
            return self.gather(*a, **kw)
        multi_robot.all_gather_paths = gather
        return self

    def __exit__(self, *exc):
        multi_robot.all_gather_paths = self.gather
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append(e)
        torch.cuda.synchronize()

    def rounds_ms(self):
        ms = [a.elapsed_time(b) for a, b in zip(self.events, self.events[1:])]
        return ms[:-1]


lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


fmt = lambda ms: " ".join(f"{v:8.2f}" for v in ms)          # noqa: E731
say(f"{torch.cuda.get_device_name(0)}; WorldRobotSampler.plan(max_rounds={ROUNDS}), constraint_table={TABLE!r}, B = {B} samples per robot, "
    f"T = {T}; ms per round (HIP events between the loop's all-gathers, median of {REPS} passes after a warm-up pass, the sides alternating)")
for n in SIZES:
    extent = float(np.sqrt(n / 8.0))
    starts, goals, offsets = world.random_world_instance(n, extent, seed=n)
    bound = framed_slot_bound(offsets, 0, n, LIMITS, multi_robot.VERTEX_CONSTRAINT_RADIUS)
    sides = {}
    for name, slots, window in (("A bound", bound, None), ("B all-pairs", n - 1, UNBOUNDED)):
        s = world.WorldRobotSampler(gpu_common.hip_model(T), starts, goals, offsets, env_id="EnvEmpty2D", n_samples=B,
                                    constraint_table=TABLE, neighbor_slots=slots)
        s.window = window
        sides[name] = (s, [])
    last = {}
    for rep in range(REPS + 1):
        for name, (s, runs) in sides.items():
            with RoundClock() as clock:
                res = s.plan(max_rounds=ROUNDS, seed=n)
            if rep > 0:
                runs.append(clock.rounds_ms())
            last[name] = (res, int(s.last_used.max()), int(s.last_dropped.sum()))
    say(f"N = {n}, world side {extent:.2f} (32 robots per tile), grid {sides['A bound'][0].world_grid}, slot bound {bound}")
    for name, (s, runs) in sides.items():
        k = min(len(r) for r in runs)
        ms = [float(np.median([r[i] for r in runs])) for i in range(k)]
        res, used, dropped = last[name]
        say(f"  {name:>12}: slots {s.neighbor_slots:5d} | {fmt(ms)} | used.max {used} dropped.sum {dropped} | conflicts per report "
            f"{res.conflict_counts}")
    # one guided step of both tables on the same input: the same active terms, so only the rounding of the slot sum may differ
    p0 = torch.from_numpy(synth.straight_line_paths(starts, goals, 64)).cuda()
    x = (torch.from_numpy(synth.synth_noise(n, (n * B, 64, 4))) * 0.5).cuda()
    grads = []
    for name, (s, _) in sides.items():
        s.set_other_paths(p0)
        grads.append(s.guide(x))
    step = float((grads[0] - grads[1]).abs().max())
    a, b = last["A bound"][0], last["B all-pairs"][0]
    same = torch.equal(a.trajs, b.trajs) and torch.equal(a.paths_local, b.paths_local)
    diff = float((a.trajs - b.trajs).abs().max()) if a.trajs.shape == b.trajs.shape else float("nan")
    say(f"  A against B: one guided step on the same input, largest difference {step:.3e} (largest gradient {float(grads[0].abs().max()):.3e}); "
        f"the plan's samples {'equal bit for bit' if same else f'differ by up to {diff:.3e} (the rounding of the slot sum, amplified by the guided loop)'}")
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
