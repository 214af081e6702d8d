"""Per-round time of MultiRobotSampler.plan_rounds_subset(replan=) for the three modes ("all", "conflicted", "independent"), next to the
PARENT COMMIT's plan() on the same instances, on one GPU.

  instances: trials.get_start_goal_pos_random_in_env on EnvEmpty2D, N = 32 ... 1024, straight lines as the first paths.  The generator's
             margin is its default 0.15 while the robots fit, else 0.5 sqrt(area / N) (from N = 128 on starts closer than the 0.105
             collision margin exist: conflicts no round can remove; this is a timing instance, not a benchmark of solutions);
  tables:    the dense all-pairs table and the cell table;
  timing:    a HIP event is recorded at every all-gather of the loop, i.e. at the start of every round and of the final report: the
             interval between two is one round as the stream sees it (report, selection, tables, sampling, pick; the host's
             synchronisation on the report's count is inside).  The three modes alternate, `--reps` times, in one process; the
             first pass of every mode warms up and is not counted; the median over the passes is printed per round;
  baseline:  `--baseline-tree DIR`: a checkout of the parent commit with its library built (python -c 'import __graft_entry__ as g;
             g.build()' in DIR).  Its plan() runs in a child process of its own with DIR in front of sys.path, on the same instances,
             timed the same way -- never this tree's own replan="all" path, which is a column of its own.
T = 25 synthetic weights (the benchmarks' random-init weights: no convergence is claimed or can be read off the conflict counts).

Usage: python tools/dbg/subset_rounds_ab.py [--baseline-tree DIR] [--out profiles/subset_rounds.txt] [--samples 4] [--rounds 3]
       [--reps 3] [N ...]"""
import json
import os
import subprocess
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
TREE = _take(args, "--tree", os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
AS_BASELINE = "--as-baseline" in args
if AS_BASELINE:
    args.remove("--as-baseline")
BASELINE_TREE = _take(args, "--baseline-tree", None)
OUT = _take(args, "--out", None)
B = _take(args, "--samples", 4, int)
ROUNDS = _take(args, "--rounds", 3, int)
REPS = _take(args, "--reps", 3, int)
SIZES = [int(a) for a in args] or [32, 128, 512, 1024]
sys.path.insert(0, TREE)
sys.path.insert(1, os.path.join(TREE, "tests"))

import numpy as np                                          # noqa: E402
import torch                                                # noqa: E402
from mmd_amd import multi_robot, trials                     # noqa: E402
import gpu_common                                           # noqa: E402

T, AREA = 25, 1.9 * 1.9
TABLES = ("dense", "binned")


def instance(n):
    margin = 0.15 if n <= 64 else 0.5 * float(np.sqrt(AREA / n))
    starts, goals = trials.get_start_goal_pos_random_in_env(n, "EnvEmpty2D", margin=margin, seed=n)
    return np.asarray(starts, np.float32), np.asarray(goals, np.float32), margin


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
        """per round run; the last interval (the final report) apart"""
        ms = [a.elapsed_time(b) for a, b in zip(self.events, self.events[1:])]
        return ms[:-1], ms[-1]


def measure(n, table, modes):
    """{mode: (median ms per round [rounds], conflict_counts, replanned_counts)}"""
    starts, goals, _ = instance(n)
    s = multi_robot.MultiRobotSampler(gpu_common.hip_model(T), starts, goals, env_id="EnvEmpty2D", n_samples=B, constraint_table=table)
    runs = {m: [] for m in modes}
    last = {}
    for rep in range(REPS + 1):
        for m in modes:
            with RoundClock() as clock:
                if m == "parent":
                    res = s.plan(max_rounds=ROUNDS, seed=n)
                else:
                    res = s.plan_rounds_subset(max_rounds=ROUNDS, seed=n, replan=m)
            if rep > 0:
                runs[m].append(clock.rounds_ms()[0])
            last[m] = (res.conflict_counts, getattr(res, "replanned_counts", None))
    out = {}
    for m in modes:
        k = min(len(r) for r in runs[m])
        out[m] = ([float(np.median([r[i] for r in runs[m]])) for i in range(k)],) + last[m]
    return out


if AS_BASELINE:
    for n in SIZES:
        for table in TABLES:
            print("BASELINE " + json.dumps({"n": n, "table": table, "parent": measure(n, table, ["parent"])["parent"]}), flush=True)
    sys.exit(0)

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


baseline = {}
if BASELINE_TREE:
    cmd = [sys.executable, HERE, "--as-baseline", "--tree", os.path.abspath(BASELINE_TREE), "--samples", str(B), "--rounds", str(ROUNDS),
           "--reps", str(REPS)] + [str(n) for n in SIZES]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True)
    for ln in r.stdout.splitlines():
        if ln.startswith("BASELINE "):
            d = json.loads(ln[len("BASELINE "):])
            baseline[(d["n"], d["table"])] = d["parent"]

fmt = lambda ms: " ".join(f"{v:8.2f}" for v in ms)          # noqa: E731
say(f"{torch.cuda.get_device_name(0)}; plan_rounds_subset(max_rounds={ROUNDS}), B = {B} samples per robot, T = {T}; ms per round (HIP events "
    f"between the loop's all-gathers, median of {REPS} passes after a warm-up pass, the modes alternating)")
say("parent = the parent commit's plan() from its own checkout and library" + ("" if BASELINE_TREE else " (NOT RUN: no --baseline-tree)"))
for n in SIZES:
    margin = instance(n)[2]
    for table in TABLES:
        got = measure(n, table, ["all", "conflicted", "independent"])
        say(f"N = {n} (generator margin {margin:.3f}), {table} table")
        if (n, table) in baseline:
            ms, counts, _ = baseline[(n, table)]
            say(f"  {'parent':>12}: {fmt(ms)} | conflicts {counts}")
        for m, (ms, counts, replanned) in got.items():
            say(f"  {m:>12}: {fmt(ms)} | conflicts {counts} | replanned {replanned}")
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
