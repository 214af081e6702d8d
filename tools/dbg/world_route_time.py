"""What routing on a world map costs on the device, needs one GPU (run it under `timeout`; one process):

    python tools/dbg/world_route_time.py [OUT.txt]

The world is 2048 x 2048 cells (environments.OCCUPANCY_MAX_SIDE = 5 x 5 tiles and a leftover strip), 300 random boxes, clearance
world.OBSTACLE_MARGIN; goals and starts are drawn from the routable cells.  With 1 goal and with 16 goals:
  field    world_routes.device_distance_field on the resident world texture: the launch sequence of mmd_grid_distance_field, 8 sweeps per
           call, with its read of `changed` after every call -- and the number of sweeps it ran;
  descent  world_routes.device_descend: 64 starts per goal, one launch of mmd_grid_descend;
  numpy    world_routes.grid_distance_field, the definition, on the same routable mask (one pass, on the host).
The device fields are compared with the definition's, integer for integer, before anything is timed.  Per device figure: 1 warm-up pass,
then the median of 5 passes.  'gpu ms' = HIP events around the pass on the current stream, 'wall ms' = perf_counter around the pass with a
device synchronisation at both ends.

Prints the table; with OUT.txt also writes it there."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mmd_amd import environments as E, map_textures, world_routes as R                 # noqa: E402

WARMUP, PASSES = 1, 5
SIDE, STARTS_PER_GOAL = E.OCCUPANCY_MAX_SIDE, 64
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, passes=PASSES, warmup=WARMUP):
    """(median gpu ms, median wall ms) of fn()"""
    gpu, wall = [], []
    for k in range(warmup + passes):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            gpu.append(e0.elapsed_time(e1))
            wall.append(1e3 * (t1 - t0))
    return statistics.median(gpu), statistics.median(wall)


def random_world(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    occ = np.zeros((SIDE, SIDE), np.uint8)
    for _ in range(300):
        x, y = rng.integers(0, SIDE - 80, 2)
        w, h = rng.integers(4, 80, 2)
        occ[x:x + w, y:y + h] = 1
    return occ


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}; {WARMUP} warm-up pass, median of {PASSES}")
    occ = random_world(1)
    E.register_world_map("Timed", occ)
    wtex = map_textures.device_world_texture("Timed", "cuda")
    region, n_tiles = R.world_lattice("Timed")
    rt = R.routable_cells(wtex.cpu().numpy(), R.OBSTACLE_MARGIN, region)
    say(f"world  {SIDE} x {SIDE} cells ({100 * occ.mean():.1f} % occupied), {n_tiles[0]} x {n_tiles[1]} tiles, {int(rt.sum())} routable cells "
        f"at clearance {R.OBSTACLE_MARGIN}")
    rng = np.random.Generator(np.random.PCG64(2))
    cells = np.argwhere(rt)
    for n_goals in (1, 16):
        goals = cells[rng.choice(len(cells), n_goals, replace=False)]
        t0 = time.perf_counter()
        ref = R.grid_distance_field(rt, goals)
        t_numpy = 1e3 * (time.perf_counter() - t0)
        dist, sweeps = R.device_distance_field(wtex, goals, R.OBSTACLE_MARGIN, region)
        assert np.array_equal(dist.cpu().numpy(), ref), "the device field is not the definition's"
        f_gpu, f_wall = timed(lambda: R.device_distance_field(wtex, goals, R.OBSTACLE_MARGIN, region))
        starts = cells[rng.choice(len(cells), n_goals * STARTS_PER_GOAL, replace=False)]
        fields = np.repeat(np.arange(n_goals), STARTS_PER_GOAL)
        tiles, summary = R.device_descend(dist, starts, fields, 400, (0, 0), 32)
        summary = summary.cpu().numpy()
        for q in range(0, len(starts), 16):
            want = R.descend(ref[fields[q]], starts[q], 400, (0, 0), 32)
            assert summary[q].tolist() == [want[1], want[2], want[3], 0], f"descent {q} is not the definition's"
        d_gpu, d_wall = timed(lambda: R.device_descend(dist, starts, fields, 400, (0, 0), 32))
        ok = summary[:, 2] == R.ROUTE_OK
        say(f"{n_goals:2d} goal(s) | field: {sweeps} sweeps, gpu {f_gpu:9.2f} ms, wall {f_wall:9.2f} ms | descent of {len(starts)} starts "
            f"({int(ok.sum())} reach their goal, longest {int(summary[ok, 0].max()) if ok.any() else 0} steps, most tiles "
            f"{int(summary[ok, 1].max()) if ok.any() else 0}): gpu {d_gpu:9.2f} ms, wall {d_wall:9.2f} ms | numpy definition of the "
            f"field(s): {t_numpy:9.1f} ms")
    E.unregister_world_map("Timed")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
