"""What a custom map's SDF texture costs to put on the device, needs one GPU:

    python tools/dbg/sdf_grid_time.py [OUT.txt]

Side A: environments.device_sdf_grid -- the upload of the primitives and mmd_sdf_grid_build into a resident [400, 400, 4] texture.
Side B: the host build of the same map (sdf_grid_texture, torch autograd, cache dropped before every pass) plus the 2.56 MB upload.
Maps of 9, 100 and 1 000 primitives (half spheres, half boxes, seeded).  Both sides are compared word for word before they are timed.
Per figure: 3 warm-up passes, then the median of 15 passes (the host build of 1 000 primitives: 1 and 3).  'gpu us' = HIP events around the pass on the current stream (for side B
the upload alone: the host build is CPU work), 'wall us' = perf_counter around the pass with a device synchronisation at both ends.

Then environments.update_map on a map a live guide reads (one resident slice rebuilt in place) against tearing the guide down and
re-creating it on a fresh registration of the new primitives (a device build into a new texture and a new guide object), wall clock.

Prints the table; with OUT.txt also writes it there."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mmd_amd import environments as E, guides, map_textures, synth                                  # noqa: E402
from mmd_amd.normalization import TrajectoryDatasetFacade                              # noqa: E402

WARMUP, PASSES = 3, 15
SLOW = dict(passes=3, warmup=1)      # the host build of 1 000 primitives takes seconds and gigabytes: fewer passes
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def primitives(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_s = n // 2
    spheres = np.concatenate([rng.uniform(-1, 1, (n_s, 2)), rng.uniform(0.02, 0.15, (n_s, 1))], 1).astype(np.float32)
    boxes = np.concatenate([rng.uniform(-1, 1, (n - n_s, 2)), rng.uniform(0.02, 0.3, (n - n_s, 2))], 1).astype(np.float32)
    return boxes.tolist(), spheres.tolist()


def timed(fn, prep=None, passes=PASSES, warmup=WARMUP):
    """(median gpu us, median wall us) of fn(); prep() runs before every pass, outside the brackets"""
    gpu, wall = [], []
    for k in range(warmup + passes):
        if prep:
            prep()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            gpu.append(1e3 * e0.elapsed_time(e1))
            wall.append(1e6 * (t1 - t0))
    return statistics.median(gpu), statistics.median(wall)


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}; {WARMUP} warm-up passes, median of {PASSES}")
    say(f"{'primitives':>10s} | {'A: device build':>32s} | {'B: host build':>14s} {'B: upload':>24s} | B wall / A wall")
    say(f"{'':>10s} | {'gpu us':>15s} {'wall us':>16s} | {'wall us':>14s} {'gpu us':>11s} {'wall us':>12s} |")
    out = torch.empty(400, 400, 4, device="cuda")
    for n in (9, 100, 1000):
        boxes, spheres = primitives(n, n)
        name = f"Timed{n}"
        E.register_map(name, boxes, spheres)
        host = torch.from_numpy(E.sdf_grid_texture(name))
        E.device_sdf_grid(boxes, spheres, "cuda", out=out)
        assert torch.equal(out.cpu().view(torch.int32), host.view(torch.int32)), f"{n} primitives: the device grid is not the host texture"
        a_gpu, a_wall = timed(lambda: E.device_sdf_grid(boxes, spheres, "cuda", out=out))
        _, b_host = timed(lambda: E.sdf_grid_texture(name), prep=lambda: E._drop_host_texture(name), **(SLOW if n >= 1000 else {}))
        b_gpu, b_up = timed(lambda: out.copy_(host))
        say(f"{n:10d} | {a_gpu:15.1f} {a_wall:16.1f} | {b_host:14.1f} {b_gpu:11.1f} {b_up:12.1f} | {(b_host + b_up) / a_wall:10.1f} x")
        E.unregister_map(name)

    say("# update_map on a map a live guide reads, against tearing the guide down and re-creating it on the new primitives (wall us)")
    ds = TrajectoryDatasetFacade(synth.NORM_MINS, synth.NORM_MAXS)
    for n in (9, 100, 1000):
        a, b = primitives(n, n), primitives(n, n + 1)
        E.register_map("Live", *a)
        guide = guides.GuideManagerTrajectoriesWithVelocity(ds, env_id="Live", device="cuda")
        flip = [0]

        def update():
            flip[0] ^= 1
            E.update_map("Live", *(b if flip[0] else a))

        def recreate():
            flip[0] ^= 1
            E.unregister_map("Live")
            E.register_map("Live", *(b if flip[0] else a))
            return guides.GuideManagerTrajectoriesWithVelocity(ds, env_id="Live", device="cuda")

        ptr = guide._grids.data_ptr()
        _, up = timed(update)
        assert guide._grids.data_ptr() == ptr
        builds = map_textures.N_TEXTURE_BUILDS
        _, re = timed(recreate)
        say(f"{n:10d} | update_map {up:12.1f} | unregister + register + new guide (device build) {re:12.1f} | {re / up:6.1f} x   "
            f"({map_textures.N_TEXTURE_BUILDS - builds} device builds on the right-hand side)")
        E.unregister_map("Live")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
