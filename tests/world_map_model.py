"""World maps (environments.register_world_map): the test world and the models the tests hold the two kernels and the samplers to.

  world_bitmap     the 640 x 520 test world: one box the two test windows both see, a bar 5 cells below the lower border of the first
                   window (outside it), and the small features of an occupancy test map;
  gather_windows   mmd_sdf_grid_windows in numpy on 32-bit words: the clamped gather;
  lookup           mmd_sdf_grid_lookup in numpy fp32, operation for operation;
  host_free_mask   postprocess_batch's free flag on a host texture (the method of tests/test_gpu_occupancy_maps.py::_host_free_mask)."""
import numpy as np

SHAPE = (640, 520)
WINDOW_A, WINDOW_B = (0, 60), (240, 60)          # origin cells: A covers ix 0..399, B ix 240..639, both iy 60..459; they share ix 240..399
BAR = (slice(100, 140), slice(30, 56))           # its last row of cells, iy = 55, lies 5 cells below window A's first, iy = 60
SHARED_BOX = (slice(300, 340), slice(200, 320))  # inside both windows


def world_bitmap():
    """[640, 520] uint8, indexed [ix, iy]"""
    occ = np.zeros(SHAPE, np.uint8)
    occ[BAR] = 1
    occ[SHARED_BOX] = 1
    occ[60:90, 300:380] = 1                                    # in window A only
    occ[520:600, 120:160] = 1                                  # in window B only
    i, j = np.arange(SHAPE[0])[:, None], np.arange(SHAPE[1])[None, :]
    occ[(i - 470) ** 2 + (j - 400) ** 2 <= 30 ** 2] = 1        # a disc (window B, and the corner of A's columns)
    occ[180:260, 140] = 1                                      # a wall one cell thick ...
    occ[221, 140] = 0                                          # ... with a gap of one cell
    for c in ((15, 75), (222, 411), (377, 90), (610, 300), (399, 459), (240, 60), (0, 0), (639, 519), (639, 0)):
        occ[c] = 1                                             # single cells: window corners and world corners among them
    occ[420:440, 490:520] = 1                                  # above both windows, at the world's upper edge
    return occ



def gather_windows(world, origins, nx, ny):
    """windows[k][ix][iy] = world[clamp(i0_k + ix, 0, wnx - 1)][clamp(j0_k + iy, 0, wny - 1)] on uint32 words [wnx, wny, 4]"""
    world = np.asarray(world)
    assert world.dtype == np.uint32
    wnx, wny = world.shape[:2]
    out = np.empty((len(origins), nx, ny, 4), np.uint32)
    for k, (i0, j0) in enumerate(np.asarray(origins, np.int64).tolist()):
        sx = np.clip(i0 + np.arange(nx, dtype=np.int64), 0, wnx - 1)
        sy = np.clip(j0 + np.arange(ny, dtype=np.int64), 0, wny - 1)
        out[k] = world[sx[:, None], sy[None, :]]
    return out


def lookup(grid, lo, hi, points):
    """out[i] = grid[ix][iy] with ix = floor((px - lo[0]) / |hi[0] - lo[0]| * nx) in fp32 (one rounding per operation), clamped to
    [0, nx - 1]; four NaNs for a point with a non-finite coordinate.  grid float32 [nx, ny, 4], points float32 [n, 2] -> float32 [n, 4]"""
    f = np.float32
    grid, points = np.asarray(grid, f), np.asarray(points, f)
    lo, hi = np.asarray(lo, f), np.asarray(hi, f)
    out = np.full((len(points), 4), np.nan, f)
    for i, p in enumerate(points):
        if not np.isfinite(p).all():
            continue
        idx = []
        for k in range(2):
            with np.errstate(over="ignore"):
                v = np.floor(f(f(f(p[k] - lo[k]) / f(abs(f(hi[k] - lo[k])))) * f(grid.shape[k])))
            idx.append(int(min(max(v, f(0)), f(grid.shape[k] - 1))))
        out[i] = grid[idx[0], idx[1]]
    return out


def nearest_cell_collides(tex, px, py, margin):
    """PlanningTask.compute_collision on a tile's grid (grid_map_sdf.py:84-99, tasks.py:204-232) in numpy fp32: nearest cell of the host
    texture or a workspace boundary (1.08 x the limits, tasks.py:81-83) nearer than margin."""
    f = np.float32
    ix = np.clip(np.floor((px - f(-1)) / f(2) * f(tex.shape[0])).astype(np.int64), 0, tex.shape[0] - 1)
    iy = np.clip(np.floor((py - f(-1)) / f(2) * f(tex.shape[1])).astype(np.int64), 0, tex.shape[1] - 1)
    lo, hi = f(-1) * f(1.08), f(1) * f(1.08)
    return (tex[ix, iy, 0] < margin) | (px - lo < margin) | (py - lo < margin) | (hi - px < margin) | (hi - py < margin)


def host_free_mask(tex, trajs):
    """postprocess_batch's free flag of un-normalised trajectories [n, H, 4] in the tile's frame by the host texture `tex`: no
    interpolated point (5 per segment) collides at the robot radius and every support point is inside the joint limits."""
    from mmd_amd import postprocess as post
    f = np.float32
    trajs = np.asarray(trajs, f)
    alpha = post.interpolation_alphas(5)
    px = trajs[:, :-1, None, 0] * alpha + trajs[:, 1:, None, 0] * (f(1) - alpha)
    py = trajs[:, :-1, None, 1] * alpha + trajs[:, 1:, None, 1] * (f(1) - alpha)
    coll = nearest_cell_collides(tex, px, py, f(post.ROBOT_RADIUS)).reshape(len(trajs), -1)
    q_min, q_max = np.asarray(post.Q_MIN, f), np.asarray(post.Q_MAX, f)
    inside = ((trajs[..., :2] >= q_min) & (trajs[..., :2] <= q_max)).all((1, 2))
    return ~coll.any(1) & inside
