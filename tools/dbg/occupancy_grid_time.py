"""What an occupancy map's SDF texture costs to put on the device, needs one GPU:

    python tools/dbg/occupancy_grid_time.py [OUT.txt]

The map is the 400 x 400 occupancy test map (tests/occupancy_model.py::test_occupancy), and the same grid all free and all occupied (the
longest row walks of pass 1).
Side A: mmd_sdf_grid_from_occupancy alone on a resident bitmap ('kernels'), and environments.device_occupancy_sdf_grid from a host array
(with the 160 kB upload and the workspace allocation) and from a device tensor, into a resident [400, 400, 4] texture.
Side B: the host definition (environments.occupancy_sdf_texture, numpy) plus the 2.56 MB upload.
Both sides are compared word for word before they are timed.  Per figure: 3 warm-up passes, then the median of 15 passes (the host
definition: 1 and 3).  'gpu us' = HIP events around the pass on the current stream, 'wall us' = perf_counter around the pass with a device
synchronisation at both ends.

Then environments.update_occupancy_map on a map a live guide reads (one resident slice rebuilt in place), from a host array and from a
device tensor, wall clock.

Prints the table; with OUT.txt also writes it there."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import occupancy_model                                                                 # noqa: E402
from mmd_amd import _lib, environments as E, guides, synth                             # noqa: E402
from mmd_amd.normalization import TrajectoryDatasetFacade                              # noqa: E402

WARMUP, PASSES = 3, 15
SLOW = dict(passes=3, warmup=1)      # the host definition takes more than a second
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, passes=PASSES, warmup=WARMUP):
    """(median gpu us, median wall us) of fn()"""
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
            gpu.append(1e3 * e0.elapsed_time(e1))
            wall.append(1e6 * (t1 - t0))
    return statistics.median(gpu), statistics.median(wall)


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}; {WARMUP} warm-up passes, median of {PASSES} (host definition: {SLOW['warmup']} and {SLOW['passes']})")
    say(f"{'map':>14s} | {'A: kernels':>10s} | {'A: from a host array':>22s} | {'A: from a device tensor':>23s} | {'B: host definition':>18s} "
        f"{'B: upload':>20s} | B wall / A wall")
    say(f"{'':>14s} | {'gpu us':>10s} | {'gpu us':>10s} {'wall us':>11s} | {'gpu us':>11s} {'wall us':>11s} | {'wall us':>18s} {'gpu us':>9s} "
        f"{'wall us':>10s} | (from a host array)")
    nx, ny = E.grid_shape()
    out = torch.empty(nx, ny, 4, device="cuda")
    n_work = int(_lib.load().mmd_sdf_grid_occupancy_work_bytes(nx, ny))
    work = torch.empty(n_work, dtype=torch.uint8, device="cuda")
    test = occupancy_model.test_occupancy()
    for name, occ in (("test map", test), ("all free", np.zeros_like(test)), ("all occupied", np.ones_like(test))):
        host = torch.from_numpy(E.occupancy_sdf_texture(occ))
        occ_dev = torch.from_numpy(occ).cuda()

        def kernels():
            _lib.launch("mmd_sdf_grid_from_occupancy", out, C.c_void_p(occ_dev.data_ptr()), nx, ny, E.SDF_CELL_SIZE,
                        C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), n_work)

        for build in (kernels, lambda: E.device_occupancy_sdf_grid(occ, "cuda", out=out),
                      lambda: E.device_occupancy_sdf_grid(occ_dev, "cuda", out=out)):
            out.fill_(float("nan"))
            build()
            assert torch.equal(out.cpu().view(torch.int32), host.view(torch.int32)), f"{name}: the device grid is not the host texture"
        k_gpu, _ = timed(kernels)
        h_gpu, h_wall = timed(lambda: E.device_occupancy_sdf_grid(occ, "cuda", out=out))
        d_gpu, d_wall = timed(lambda: E.device_occupancy_sdf_grid(occ_dev, "cuda", out=out))
        _, b_host = timed(lambda: E.occupancy_sdf_texture(occ), **SLOW)
        b_gpu, b_up = timed(lambda: out.copy_(host))
        say(f"{name:>14s} | {k_gpu:10.1f} | {h_gpu:10.1f} {h_wall:11.1f} | {d_gpu:11.1f} {d_wall:11.1f} | {b_host:18.1f} {b_gpu:9.1f} {b_up:10.1f} | "
            f"{(b_host + b_up) / h_wall:10.1f} x")

    say("# update_occupancy_map on a map a live guide reads: one resident slice rebuilt in place (wall us)")
    ds = TrajectoryDatasetFacade(synth.NORM_MINS, synth.NORM_MAXS)
    a, b = test, np.ascontiguousarray(test[::-1, ::-1])
    a_dev, b_dev = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    E.register_occupancy_map("Live", a)
    guide = guides.GuideManagerTrajectoriesWithVelocity(ds, env_id="Live", device="cuda")
    ptr, flip = guide._grids.data_ptr(), [0]

    def update(maps):
        flip[0] ^= 1
        E.update_occupancy_map("Live", maps[flip[0]])

    _, from_host = timed(lambda: update((a, b)))
    _, from_dev = timed(lambda: update((a_dev, b_dev)))
    assert guide._grids.data_ptr() == ptr
    assert torch.equal(guide._grids[0, 0].cpu().view(torch.int32), torch.from_numpy(E.sdf_grid_texture("Live")).view(torch.int32))
    say(f"{'test map':>14s} | from a host array {from_host:10.1f} | from a device tensor (with the registry's copy to the host) {from_dev:10.1f}")
    E.unregister_map("Live")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
