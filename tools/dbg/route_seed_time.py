"""What the seed trajectories of world routes cost on the device, needs one GPU (run it under `timeout`; one process):

    python tools/dbg/route_seed_time.py [OUT.txt]

The world is world_route_time.py's: 2048 x 2048 cells (5 x 5 tiles and a leftover strip), 300 random boxes, clearance world.OBSTACLE_MARGIN;
16 goals and the starts are drawn from the routable cells.  With 1, 64 and 1024 routes:
  samples  world_routes.device_descend_samples: one launch of mmd_grid_descend_samples (two walks per lane);
  seeds    world_routes.device_route_seeds: one launch of mmd_route_seeds, with smooth_iters 0 / 64 / 256;
  numpy    descend_samples and seed_trajectory, the definitions, for the same routes (one pass, on the host).
Every device output is compared with the definition's, integers and float32 bits, before anything is timed (at 1024 routes: every 16th
route).  Per device figure: 1 warm-up pass, then the median of 5 passes.  'gpu ms' = HIP events around the pass on the current stream,
'wall ms' = perf_counter around the pass with a device synchronisation at both ends.

One informational line at the end: on a two-tile world with two doors, the number of collision-free samples of one planner call seeded by
route_experience against the same planner's call from noise.  The weights are random-init: the line shows that both calls run, and says
nothing about planning quality.

Prints the table; with OUT.txt also writes it there."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmd_amd import environments as E, map_textures, synth, world_routes as R           # noqa: E402
from world_route_time import LINES, random_world, say, timed                           # noqa: E402

N_GOALS, MAX_TILES, TILE = 16, 16, 400
DT = 5.0 / 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def doors_line():
    occ = np.zeros((800, 400), np.uint8)
    occ[398:402, :] = 1
    occ[398:402, 20:140] = 0
    occ[398:402, 260:380] = 0
    E.register_world_map("TimedDoors", occ)
    centre = lambda c: np.asarray([(c[k] + 0.5) * 0.005 - occ.shape[k] * 0.0025 for k in range(2)], np.float32)      # noqa: E731
    start, goal = torch.from_numpy(centre((100, 350))), torch.from_numpy(centre((700, 300)))
    route, seed = R.world_route_seeded("TimedDoors", start, goal, device="cuda")
    B = 32
    sd = synth.synth_unet_state_dict(0)
    planner = R.route_planner(route, "EnvHighways2D-RobotPlanarDisk", start, goal, planner_alg="mmd", device="cuda", seed=23, n_samples=B,
                              model_state_dicts=[sd] * len(route.env_ids), model_args=dict(n_diffusion_steps=25), trained_models_dir="")
    free = []
    for experience in (R.route_experience(seed, B), None):
        out = planner(start, goal, experience=experience, seed=77)
        free.append(0 if out.trajs_final_free is None else len(out.trajs_final_free))
    say(f"doors world, {len(route.env_ids)} tiles, {B} samples, random-init weights (no claim about planning quality): free samples of the "
        f"seeded call {free[0]}, of the from-noise call {free[1]}")
    E.unregister_world_map("TimedDoors")


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}; 1 warm-up pass, median of 5")
    occ = random_world(1)
    E.register_world_map("Timed", occ)
    wtex = map_textures.device_world_texture("Timed", "cuda")
    tex = wtex.cpu().numpy()
    lo, hi = E.world_map_limits("Timed")
    region, n_tiles = R.world_lattice("Timed")
    rt = R.routable_cells(tex, R.OBSTACLE_MARGIN, region)
    say(f"world  {occ.shape[0]} x {occ.shape[1]} cells ({100 * occ.mean():.1f} % occupied), {n_tiles[0]} x {n_tiles[1]} tiles, {int(rt.sum())} "
        f"routable cells at clearance {R.OBSTACLE_MARGIN}; {N_GOALS} goals, max_tiles {MAX_TILES}")
    rng = np.random.Generator(np.random.PCG64(2))
    cells = np.argwhere(rt)
    goals = cells[rng.choice(len(cells), N_GOALS, replace=False)]
    dist, _ = R.device_distance_field(wtex, goals, R.OBSTACLE_MARGIN, region)
    ref = dist.cpu().numpy()
    for n in (1, 64, 1024):
        starts = cells[rng.choice(len(cells), n, replace=False)]
        fields = rng.integers(0, N_GOALS, n)
        s_pts, g_pts = R.cell_centres(starts, lo, hi, tex.shape), R.cell_centres(goals[fields], lo, hi, tex.shape)
        got = R.device_descend_samples(dist, starts, fields, TILE, (0, 0), MAX_TILES)
        tiles, summary, visit_cells, sample_cells = [a.cpu().numpy() for a in got]
        check = range(0, n, 16 if n > 64 else 1)
        t0 = time.perf_counter()
        want = {q: R.descend_samples(ref[fields[q]], starts[q], TILE, (0, 0), MAX_TILES) for q in check}
        t_walk = 1e3 * (time.perf_counter() - t0)
        for q, w in want.items():
            assert summary[q].tolist() == [w[1], w[2], w[3], 0] and np.array_equal(visit_cells[q, :len(w[4])], w[4]) and \
                np.array_equal(sample_cells[q, :len(w[5])], w[5]) and not sample_cells[q, len(w[5]):].any(), f"samples {q} are not the definition's"
        w_gpu, w_wall = timed(lambda: R.device_descend_samples(dist, starts, fields, TILE, (0, 0), MAX_TILES))
        ok = summary[:, 2] == R.ROUTE_OK
        say(f"{n:4d} route(s) ({int(ok.sum())} ok, longest {int(summary[ok, 0].max()) if ok.any() else 0} steps, most tiles "
            f"{int(summary[ok, 1].max()) if ok.any() else 0}) | samples: gpu {w_gpu:8.3f} ms, wall {w_wall:8.3f} ms | numpy descend_samples of "
            f"{len(want)} of them: {t_walk:9.1f} ms")
        for iters in (0, 64, 256):
            call = lambda: R.device_route_seeds(wtex, lo, hi, got[3], got[0], got[1], TILE, (0, 0), s_pts, g_pts, R.OBSTACLE_MARGIN, iters, DT)   # noqa: E731
            seeds, clear_min = [a.cpu().numpy() for a in call()]
            t0 = time.perf_counter()
            for q, w in want.items():
                seed, cmin = R.seed_trajectory(tex, lo, hi, w[5], w[0][:len(w[5])], TILE, (0, 0), s_pts[q], g_pts[q], R.OBSTACLE_MARGIN, iters, DT)
                assert np.array_equal(bits(seeds[q, :len(seed)]), bits(seed)) and not bits(seeds[q, len(seed):]).any() and \
                    bits(clear_min[q]) == bits(cmin), f"seed {q} at {iters} iterations is not the definition's"
            t_seed = 1e3 * (time.perf_counter() - t0)
            s_gpu, s_wall = timed(call)
            say(f"       smooth_iters {iters:4d} | seeds: gpu {s_gpu:8.3f} ms, wall {s_wall:8.3f} ms | numpy seed_trajectory of {len(want)} of them: "
                f"{t_seed:9.1f} ms")
    E.unregister_world_map("Timed")
    doors_line()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
