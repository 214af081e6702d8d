"""What the report of a fleet's run costs on the device, needs one GPU (run it under `timeout`; one process):

    python tools/dbg/fleet_report_time.py [OUT.txt]

The world is world_route_time.py's: 2048 x 2048 cells, 300 random boxes.  With N = 64 and N = 256 robots (fleet_time.py's sizes) and
E = 5 epochs, L = 320 columns: seeded random walks over the world with steps of about 3 cells (a fleet's step length), every eighth robot
walking a robot-robot margin beside its neighbour, goals at the last points of half of the robots.  margin = the robot's radius,
rr_margin = RR_MARGIN, n_interp = 3, goal_tol = the cell pitch.  The paths are synthetic: the figures say what the report costs, nothing
about any planner's quality, and no threshold, default or test depends on them.
  launch   world_fleet.device_run_report_words: the two memsets and the two kernels of mmd_fleet_run_report, 20 calls per pass, per call;
  report   world_fleet.device_run_report: the same and its ONE device -> host copy, and the split of the words on the host;
  numpy    world_fleet.run_report, the definition, on the downloaded texture (one pass, on the host).
Before anything is timed the device's report is compared with the definition's: every integer, clear_min, max_step and end_error bit for
bit, `length` within L * 2^-24.  Per device figure: 1 warm-up pass, then the median of 5 passes.  'gpu ms' = HIP events around the pass
on the current stream, 'wall ms' = perf_counter around the pass with a device synchronisation at both ends.

Prints the table; with OUT.txt also writes it there."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmd_amd import environments as E, map_textures, world_fleet as F                              # noqa: E402
from world_route_time import LINES, random_world, say, timed                                      # noqa: E402

EPOCHS, CALLS = 5, 20
EXACT = ("points_hit", "interp_hit", "first_hit", "bad_points", "outside", "arrival", "conflicts", "clear_min", "max_step", "end_error",
         "conflict_count", "first_conflict", "robots_hit", "robots_in_conflict", "robots_arrived", "column_conflicts")


def walks(n, length, lo, hi, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    paths = rng.uniform(lo, hi, (n, 1, 2)) + np.cumsum(rng.normal(0, 0.011, (n, length, 2)), 1)
    paths[1::8] = paths[0::8][:len(paths[1::8])] + rng.normal(0, 0.07, (len(paths[1::8]), 1, 2))
    paths = np.clip(paths, lo, hi).astype(np.float32)
    goals = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
    goals[::2] = paths[::2, -1]
    return paths, goals


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}; 1 warm-up pass, median of 5 (numpy: one pass)")
    occ = random_world(1)
    E.register_world_map("Timed", occ)
    tex = map_textures.device_world_texture("Timed", "cuda")
    tex_host = tex.cpu().numpy()
    lo, hi = E.world_map_limits("Timed")
    length = 64 * EPOCHS
    say(f"world  {occ.shape[0]} x {occ.shape[1]} cells ({100 * occ.mean():.1f} % occupied); E = {EPOCHS} epochs, L = {length} columns, margin "
        f"{F.ROBOT_RADIUS}, rr_margin {F.RR_MARGIN:.3f}, n_interp 3")
    for n in (64, 256):
        paths, goals = walks(n, length, lo, hi, n)
        paths_d, goals_d = torch.from_numpy(paths).cuda(), torch.from_numpy(goals).cuda()
        args = (lo, hi, goals_d, F.ROBOT_RADIUS, F.RR_MARGIN, 3, None)
        t0 = time.perf_counter()
        want = F.run_report(paths, tex_host, lo, hi, goals, F.ROBOT_RADIUS, F.RR_MARGIN, 3, None, column_conflicts=True)
        host_ms = 1e3 * (time.perf_counter() - t0)
        got = F.device_run_report(paths_d, tex, *args, column_conflicts=True)
        for k in EXACT:
            a, b = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
            assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b), (n, k)
        exact = F.segment_lengths(paths).astype(np.float64).sum(1)
        assert (np.abs(got.length - exact) <= length * 2.0 ** -24 * exact).all(), (n, "length")

        def launches():
            for _ in range(CALLS):
                F.device_run_report_words(paths_d, tex, *args)
        gpu, wall = timed(launches)
        gpu_r, wall_r = timed(lambda: F.device_run_report(paths_d, tex, *args))
        say(f"N = {n:3d} | {want.conflict_count} conflicts, {want.robots_hit} robots hit, {want.robots_arrived} arrived: equal to the definition"
            f" | launch: gpu {gpu / CALLS:7.3f} ms, wall {wall / CALLS:7.3f} ms per call | report (launch, one copy, split): gpu {gpu_r:7.3f} ms, "
            f"wall {wall_r:7.3f} ms | numpy: wall {host_ms:9.1f} ms")
    E.unregister_world_map("Timed")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
