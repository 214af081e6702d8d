"""A numpy model of the framed all-pairs table (include/mmd_amd.h: mmd_framed_constraints_from_paths), shared by the CPU tests, which pin
it to mmd_pack_constraints, and the GPU tests, which compare the kernel with it word for word.  Everything is fp32, operation by operation."""
import numpy as np

H = 64
RADIUS = np.float32(0.05 * 2.4)
EMPTY = np.array([0.0, 0.0, -1.0, -1.0], np.float32)


def default_window(radius=RADIUS, limits=((-1.0, -1.0), (1.0, 1.0))):
    """limits -/+ 1.0625 x radius, in fp32 (constraints.framed_window)"""
    w = np.float32(1.0625) * np.float32(radius)
    return np.asarray(limits[0], np.float32) - w, np.asarray(limits[1], np.float32) + w


def included(paths, offsets, r, wlo, whi):
    """-> (q [n_all, H, 2] fp32 = paths - offsets[r], inc [n_all, H] bool): robot j at time step t is included in robot r's table"""
    paths, offsets = np.asarray(paths, np.float32), np.asarray(offsets, np.float32)
    q = (paths - offsets[r][None, None, :]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        inc = (q[..., 0] >= wlo[0]) & (q[..., 0] <= whi[0]) & (q[..., 1] >= wlo[1]) & (q[..., 1] <= whi[1])
    inc[r] = False
    inc[:, 0] = False                                      # constraints cover t >= 1
    return q, inc


def point_list(paths, offsets, r, wlo, whi):
    """robot r's included points as a constraint list: (q [n, 2], t_range [(t, t + 1)]) in the order other robot ascending, t ascending"""
    q, inc = included(paths, offsets, r, wlo, whi)
    j, t = np.nonzero(inc)
    return q[j, t], [(int(v), int(v) + 1) for v in t]


def framed_table(paths, offsets, robot0, n_local, S, radius=RADIUS, weight=2e-2, window=None):
    """-> (ell [n_local * S, H, 4], grp_slot_off [n_local + 1], grp_weight [n_local], robot_grp_off [n_local + 1], used [n_local],
    dropped [n_local]) exactly as the entry point defines them"""
    wlo, whi = default_window(radius) if window is None else (np.asarray(window[0], np.float32), np.asarray(window[1], np.float32))
    radius = np.float32(radius)
    word_r = np.array([radius, radius * np.abs(radius)], np.float32)
    ell = np.tile(EMPTY, (n_local * S, H, 1))
    used, dropped = np.zeros(n_local, np.int32), np.zeros(n_local, np.int32)
    for i in range(n_local):
        q, inc = included(paths, offsets, robot0 + i, wlo, whi)
        for t in range(1, H):
            ids = np.flatnonzero(inc[:, t])
            keep = ids[:S]
            ell[i * S + np.arange(len(keep)), t, :2] = q[keep, t]
            ell[i * S + np.arange(len(keep)), t, 2:] = word_r
            used[i] = max(used[i], len(keep))
            dropped[i] += len(ids) - len(keep)
    gso = (np.arange(n_local + 1) * S).astype(np.int32)
    return ell, gso, np.full(n_local, weight, np.float32), np.arange(n_local + 1, dtype=np.int32), used, dropped


def slot_bound(offsets, robot0, n_local, radius=RADIUS, limits=((-1.0, -1.0), (1.0, 1.0))):
    """brute force: per local robot the other robots whose window box meets this robot's widened window; the maximum in [1, N - 1]"""
    off = np.asarray(offsets, np.float64)
    wlo, whi = (v.astype(np.float64) for v in default_window(radius, limits))
    lo, hi = np.asarray(limits[0], np.float64), np.asarray(limits[1], np.float64)
    worst = 0
    for r in range(robot0, robot0 + n_local):
        c = 0
        for j in range(len(off)):
            if j == r:
                continue
            meets = all(off[j][k] + hi[k] >= off[r][k] + wlo[k] and off[j][k] + lo[k] <= off[r][k] + whi[k] for k in range(2))
            c += int(meets)
        worst = max(worst, c)
    return min(max(worst, 1), len(off) - 1)


def conflicts(paths, margin=np.float32(2.1 * 0.05)):
    """brute force of the conflict report of global paths [N, H, 2]: (count, robot_counts [N], first (t, a, b) or None) with the collision
    decision sqrt(fma(dy, dy, dx * dx)) < margin replayed in fp32 (dx * dx rounded, the fma exact in float64 then rounded)"""
    p = np.asarray(paths, np.float32)
    n = p.shape[0]
    d = (p[:, None] - p[None, :]).astype(np.float32)                      # [a, b, t, 2]
    dxx = (d[..., 0] * d[..., 0]).astype(np.float32)
    s = (d[..., 1].astype(np.float64) * d[..., 1].astype(np.float64) + dxx.astype(np.float64)).astype(np.float32)
    hit = np.sqrt(s).astype(np.float32) < np.float32(margin)
    hit[np.arange(n), np.arange(n)] = False
    robot_counts = hit.sum(axis=(1, 2)).astype(np.int32)
    first = None
    for t in range(p.shape[1]):
        a, b = np.nonzero(np.triu(hit[:, :, t], 1))
        if len(a):
            first = (t, int(a[0]), int(b[0]))
            break
    return int(np.triu(hit.transpose(2, 0, 1), 1).sum()), robot_counts, first


def edge_instance():
    """The instance of the kernel's bit-for-bit test: N = 7, offsets zero and a few units, and in the frames of robots 2 .. 4 points
    exactly on a window edge and one ulp either side, a NaN, two robots on one point, a time step with no robot included, more included
    robots than S = 3 slots.  -> (paths [7, H, 2], offsets [7, 2])"""
    rng = np.random.Generator(np.random.PCG64(2024))
    offsets = np.array([[0, 0], [0, 0], [0, 0], [0.5, -0.25], [3, 0], [3, 1], [0, 0]], np.float32)
    paths = (rng.uniform(-0.9, 0.9, (7, H, 2)).astype(np.float32) + offsets[:, None, :]).astype(np.float32)
    wlo, whi = default_window()
    # t = 5, frame of robot 2 (offset 0): robot 0 on the upper x edge, robot 1 one ulp outside it, robot 6 one ulp inside
    paths[0, 5] = (whi[0], 0.1)
    paths[1, 5] = (np.nextafter(whi[0], np.float32(np.inf)), 0.1)
    paths[6, 5] = (np.nextafter(whi[0], np.float32(-np.inf)), 0.1)
    # t = 6: the lower y edge in the frame of robot 3 (offset (0.5, -0.25)), on it / outside / inside
    paths[0, 6] = (0.5, np.float32(wlo[1]) + np.float32(-0.25))
    paths[1, 6] = (0.5, np.nextafter(np.float32(wlo[1]) + np.float32(-0.25), np.float32(-np.inf)))
    paths[6, 6] = (0.5, np.nextafter(np.float32(wlo[1]) + np.float32(-0.25), np.float32(np.inf)))
    paths[0, 7] = (np.nan, 0.0)                           # a NaN point: excluded everywhere
    paths[1, 7] = (0.0, np.nan)
    paths[1, 8] = paths[0, 8]                             # two robots on one point
    paths[:, 9] = offsets + np.float32(50.0)              # nobody is in anybody's window
    paths[:, 10] = np.float32(0.25)                       # everybody within reach of the robots at offset 0: 6 included, S = 3 drops 3
    return paths, offsets
