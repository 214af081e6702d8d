"""What an epoch of a world fleet costs on the device, needs one GPU (run it under `timeout`; one process):

    python tools/dbg/fleet_time.py [OUT.txt]

The world is world_route_time.py's: 2048 x 2048 cells, 300 random boxes, clearance world.OBSTACLE_MARGIN.  With N = 64 and N = 256 robots,
starts and distinct goals drawn from the cells that one routable cell reaches, random-init weights, T = 25, B = 4 samples per robot,
reach 180 and max_steps 360 (WorldFleet's defaults), plan(max_rounds = 2):
  fields    the one-off build in WorldFleet's constructor: device_distance_field over the whole grid, one field per goal -- ONE pass, wall
            time with a device synchronisation at both ends (it allocates 4 * nx * ny bytes per goal; it is not repeated);
  sub-goals WorldFleet.epoch_targets: the upload of the robots' cells, one launch of mmd_grid_window_goals, one copy back, the offsets;
  sampler   WorldRobotSampler's construction on the epoch's windows, with the cut of its window slices (the map set is released after
            every pass, so every pass cuts);
  rounds    its plan(max_rounds = 2, seed).
Before anything is timed: the field of robot 0's goal is compared with the numpy definition, and the sub-goals of every 8th robot with
window_goals on the downloaded fields, integer for integer.  Per repeated figure: 1 warm-up pass, then the median of 5 passes.  'gpu ms'
= HIP events around the pass on the current stream, 'wall ms' = perf_counter around the pass with a device synchronisation at both ends.
The weights are random-init: the figures say what the loop costs, nothing about planning quality, and no threshold or default depends
on them.

Prints the table; with OUT.txt also writes it there."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mmd_amd import environments as E, map_textures, world_fleet as F, world_routes as R          # noqa: E402
from mmd_amd.world import WorldRobotSampler                                                        # noqa: E402
from world_route_time import LINES, random_world, say, timed                                      # noqa: E402

T, B, ROUNDS, SEED = 25, 4, 2, 7


def main():
    import gpu_common
    say(f"# device: {torch.cuda.get_device_name(0)}; 1 warm-up pass, median of 5 (the field build: one pass)")
    occ = random_world(1)
    E.register_world_map("Timed", occ)
    wtex = map_textures.device_world_texture("Timed", "cuda")
    lo, hi = E.world_map_limits("Timed")
    rng = np.random.Generator(np.random.PCG64(3))
    rt = R.routable_cells(wtex.cpu().numpy(), R.OBSTACLE_MARGIN)
    seed_cell = np.argwhere(rt)[rng.integers(0, int(rt.sum()))]
    reached = (R.device_distance_field(wtex, seed_cell[None])[0][0] != R.UNREACHED).cpu().numpy()
    cells = np.argwhere(reached)
    say(f"world  {occ.shape[0]} x {occ.shape[1]} cells ({100 * occ.mean():.1f} % occupied), {int(rt.sum())} routable cells at clearance "
        f"{R.OBSTACLE_MARGIN}, {len(cells)} of them connected to cell {seed_cell.tolist()}; T = {T}, B = {B}, plan(max_rounds = {ROUNDS})")
    model = gpu_common.hip_model(T)
    for n in (64, 256):
        pick = cells[rng.choice(len(cells), 2 * n, replace=False)]
        starts, goals = R.cell_centres(pick[:n], lo, hi, occ.shape), R.cell_centres(pick[n:], lo, hi, occ.shape)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fleet = F.WorldFleet(model, "Timed", starts, goals, n_samples=B)
        torch.cuda.synchronize()
        t_fields = 1e3 * (time.perf_counter() - t0)
        assert fleet.dist.shape[0] == n
        ref = R.grid_distance_field(rt, fleet.field_goals[fleet.fields[0]][None])
        assert np.array_equal(fleet.dist[int(fleet.fields[0])].cpu().numpy(), ref[0]), "the device field is not the definition's"
        targets = fleet.epoch_targets(fleet.positions)
        for r in range(0, n, 8):
            f = int(fleet.fields[r])
            want = F.window_goals(fleet.dist[f:f + 1].cpu().numpy(), pick[r:r + 1], [0], fleet.field_goals[f:f + 1], fleet.reach, fleet.max_steps,
                                  fleet.window)
            assert (targets.cells[r].tolist(), targets.origins[r].tolist(), targets.summary[r].tolist()) == \
                (want[0][0].tolist(), want[1][0].tolist(), want[2][0].tolist()), f"robot {r}'s sub-goal is not the definition's"
        g_gpu, g_wall = timed(lambda: fleet.epoch_targets(fleet.positions))
        made = []

        def construct():
            for s in made:
                map_textures.release_sdf_textures(sorted(set(s._window_ids)), "cuda")
            made[:] = [WorldRobotSampler(model, fleet.positions, targets.points, targets.offsets, env_id="Timed", n_samples=B)]
        c_gpu, c_wall = timed(construct)
        sampler = made[0]
        p_gpu, p_wall = timed(lambda: sampler.plan(max_rounds=ROUNDS, seed=SEED))
        res = sampler.plan(max_rounds=ROUNDS, seed=SEED)
        map_textures.release_sdf_textures(sorted(set(sampler._window_ids)), "cuda")
        say(f"N = {n:3d} | fields ({n} goals, {4 * n * occ.size / 2 ** 20:.0f} MiB): wall {t_fields:9.1f} ms | epochs needed at most "
            f"{fleet.epoch_bound()}, longest way {int(fleet.start_distances.max())} cells | sub-goals: gpu {g_gpu:7.3f} ms, wall {g_wall:7.3f} ms | "
            f"sampler + window cut ({len(set(sampler._window_ids))} windows): gpu {c_gpu:8.2f} ms, wall {c_wall:8.2f} ms | rounds "
            f"({res.n_rounds} run, conflicts {res.conflict_counts}): gpu {p_gpu:8.2f} ms, wall {p_wall:8.2f} ms")
        made.clear()
        del fleet, sampler
        torch.cuda.empty_cache()
    E.unregister_world_map("Timed")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
