"""What a world map costs on the device, needs one GPU:

    python tools/dbg/world_map_time.py [OUT.txt]

The world is 2048 x 2048 cells (environments.OCCUPANCY_MAX_SIDE), 300 random boxes; 64 robot windows at random origins.
  build    the world texture from the resident bitmap: mmd_sdf_grid_from_occupancy alone, and environments.device_world_sdf_grid (with
           the 4 MB upload and the workspace allocation) into the resident texture;
  cut      mmd_sdf_grid_windows alone: 64 windows of 400 x 400 into a resident map set, one launch; bytes moved = 2 x 64 x 2.56 MB;
  update   environments.update_world_map end to end on a world a live guide of 64 robots reads: registry, rebuild, recut.
The cut is compared word for word with an index gather of the resident world texture before it is timed (the host definition takes
minutes at this size; tests/test_gpu_world_maps.py holds build and cut to it on a 640 x 520 world).  Per figure: 2 warm-up passes, then
the median of 9 passes.  'gpu us' = HIP events around the pass on the current stream, 'wall us' = perf_counter around the pass with a
device synchronisation at both ends.

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
from mmd_amd import _lib, environments as E, guides, synth                             # noqa: E402
from mmd_amd.normalization import TrajectoryDatasetFacade                              # noqa: E402

WARMUP, PASSES = 2, 9
SIDE, N_WINDOWS = E.OCCUPANCY_MAX_SIDE, 64
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


def random_world(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    occ = np.zeros((SIDE, SIDE), np.uint8)
    for _ in range(300):
        x, y = rng.integers(0, SIDE - 80, 2)
        w, h = rng.integers(4, 80, 2)
        occ[x:x + w, y:y + h] = 1
    return occ


def main():
    say(f"# device: {torch.cuda.get_device_name(0)}; {WARMUP} warm-up passes, median of {PASSES}")
    nx, ny = E.grid_shape()
    worlds = [random_world(1), random_world(2)]
    E.register_world_map("Timed", worlds[0])
    wtex = guides.device_world_texture("Timed", "cuda")
    occ_dev = torch.from_numpy(worlds[0]).cuda()
    n_work = int(_lib.load().mmd_sdf_grid_occupancy_work_bytes(SIDE, SIDE))
    work = torch.empty(n_work, dtype=torch.uint8, device="cuda")

    def build_kernels():
        _lib.launch("mmd_sdf_grid_from_occupancy", wtex, C.c_void_p(occ_dev.data_ptr()), SIDE, SIDE, E.SDF_CELL_SIZE,
                    C.c_void_p(wtex.data_ptr()), C.c_void_p(work.data_ptr()), n_work)

    k_gpu, k_wall = timed(build_kernels)
    b_gpu, b_wall = timed(lambda: E.device_world_sdf_grid("Timed", "cuda", out=wtex))
    say(f"build  {SIDE} x {SIDE} ({100 * worlds[0].mean():.1f} % occupied) | kernels alone: gpu {k_gpu:11.1f} us, wall {k_wall:11.1f} us | "
        f"device_world_sdf_grid: gpu {b_gpu:11.1f} us, wall {b_wall:11.1f} us")

    rng = np.random.Generator(np.random.PCG64(3))
    origins = rng.integers(0, SIDE - nx + 1, (N_WINDOWS, 2)).astype(np.int32)
    org_dev = torch.from_numpy(origins).cuda()
    windows = torch.full((N_WINDOWS, 1, nx, ny, 4), float("nan"), device="cuda")

    def cut():
        _lib.launch("mmd_sdf_grid_windows", windows, C.c_void_p(wtex.data_ptr()), SIDE, SIDE, C.c_void_p(org_dev.data_ptr()), N_WINDOWS, nx, ny,
                    C.c_void_p(windows.data_ptr()))

    cut()
    for k in range(N_WINDOWS):
        i0, j0 = origins[k].tolist()
        assert torch.equal(windows[k, 0].view(torch.int32), wtex[i0:i0 + nx, j0:j0 + ny].view(torch.int32)), f"window {k} is not the crop"
    c_gpu, c_wall = timed(cut)
    moved = 2 * N_WINDOWS * nx * ny * 16
    say(f"cut    {N_WINDOWS} windows of {nx} x {ny}, one launch | gpu {c_gpu:9.1f} us, wall {c_wall:9.1f} us | {moved / 1e6:.1f} MB moved, "
        f"{moved / c_gpu / 1e6:.2f} TB/s by the gpu time")

    # update_world_map on a world a live guide of 64 robots reads (their windows are distinct slices of one map set)
    names = [E.world_window_name("Timed", o) for o in origins]
    ds = TrajectoryDatasetFacade(synth.NORM_MINS, synth.NORM_MAXS)
    guide = guides.GuideManagerTrajectoriesWithVelocity(ds, env_id=names[0], n_robots=N_WINDOWS, robot_env_ids=names, device="cuda")
    n_slices = guide._grids.shape[0]
    ptr, flip = guide._grids.data_ptr(), [0]

    def update():
        flip[0] ^= 1
        E.update_world_map("Timed", worlds[flip[0]])

    u_gpu, u_wall = timed(update)
    assert guide._grids.data_ptr() == ptr and guides.device_world_texture("Timed", "cuda") is wtex
    k = guide._robot_map[5].item()
    i0, j0 = origins[5].tolist()
    assert torch.equal(guide._grids[k, 0].view(torch.int32), wtex[i0:i0 + nx, j0:j0 + ny].view(torch.int32))
    say(f"update update_world_map end to end, {n_slices} resident window slices recut | gpu {u_gpu:11.1f} us, wall {u_wall:11.1f} us")
    E.unregister_world_map("Timed")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
