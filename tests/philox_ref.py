"""Host reference of the in-kernel Gaussian noise (csrc/guide_dev.h: philox4x32 / normal4 / traj_normal4), in plain numpy: Philox4x32-10
(Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are in test_philox_ref_host.py)
followed by Box-Muller, and the counter contract of include/mmd_amd.h:

    counter = (point & 0xFFFFFFFF, draw, point >> 32, 0)        key = (seed & 0xFFFFFFFF, seed >> 32)
    point   = global trajectory index * H + support point       (traj_index_base + index in the call's arrays), or, with
              mmd_sampler_desc.robot_seeds_dev, the index INSIDE the robot under that robot's seed
    draw    = 0xFFFFFFFF for x_T, 0xFFFFFFFE for q_sample, k = 0, 1, ... for the steps of mmd_p_sample_loop, the caller's
              draw_index (the Python layer passes the loop index i) for mmd_ddpm_step

No device code and nothing of the library is imported here: a mistake in the kernels cannot be shared with this file."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
DRAW_XT, DRAW_Q_SAMPLE = 0xFFFFFFFF, 0xFFFFFFFE
H = 64


def philox4x32_10(counter_words, k0, k1):
    """counter_words [..., 4], k0 / k1 scalars or [...] -> [..., 4] uint64 holding the four 32-bit output words."""
    c = np.asarray(counter_words, dtype=np.uint64) & M32
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0 = np.asarray(k0, dtype=np.uint64) & M32
    k1 = np.asarray(k1, dtype=np.uint64) & M32
    for _ in range(10):
        p0 = PHILOX_M0 * c0                       # 32 x 32 -> 64 bits: exact in uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def uniform01(words):
    """The kernel's u = ((float)c + 0.5f) * 2^-32, every operation rounded to float32 (u32 -> f32 is round-to-nearest-even in numpy as
    on the device): in [2^-33, 1.0], 1.0 included."""
    f = np.asarray(words, dtype=np.uint64).astype(np.uint32).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def normal4(seed, draw, points):
    """The four Gaussian values of every point: (z float64 [n, 4], r float64 [n, 4]).  The float32 roundings of the INPUTS of the
    transcendental functions (u, and the angle 2 pi u) are the kernel's; ln, sqrt, cos and sin are evaluated in float64.  r is the
    Box-Muller radius that multiplies each component (r0, r0, r1, r1): the scale of the kernel's rounding error."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    draw = int(draw) & 0xFFFFFFFF
    p = np.asarray(points, dtype=np.uint64).reshape(-1)
    ctr = np.stack([p & M32, np.full_like(p, draw), p >> np.uint64(32), np.zeros_like(p)], axis=-1)
    w = philox4x32_10(ctr, seed & 0xFFFFFFFF, seed >> 32)
    u = uniform01(w)                                                             # float32 [n, 4]
    with np.errstate(divide="raise"):
        rad = np.sqrt(np.abs(-2.0 * np.log(u[:, 0::2].astype(np.float64))))      # (abs: u = 1 gives -0.0)
    ang = (np.float32(6.283185307179586) * u[:, 1::2]).astype(np.float64)        # the product rounded to float32 first
    z = np.stack([rad[:, 0] * np.cos(ang[:, 0]), rad[:, 0] * np.sin(ang[:, 0]),
                  rad[:, 1] * np.cos(ang[:, 1]), rad[:, 1] * np.sin(ang[:, 1])], axis=-1)
    return z, np.repeat(rad, 2, axis=-1)


def traj_points(traj_base, n_traj, horizon=H):
    """Point indices of a call's [n_traj, horizon] array when trajectory 0 has the global index traj_base (one stream per call)."""
    return np.uint64(int(traj_base) * horizon) + np.arange(int(n_traj) * horizon, dtype=np.uint64)


def robot_points(n_robots, samples_per_robot, horizon=H):
    """Per-robot streams (robot_seeds): (robot [n], point [n]) of a robot-major [n_robots * samples_per_robot, horizon] array -- the point
    index restarts at 0 inside every robot."""
    per = int(samples_per_robot) * horizon
    return np.repeat(np.arange(int(n_robots)), per), np.tile(np.arange(per, dtype=np.uint64), int(n_robots))


def traj_normal4(seed, draw, n_traj, traj_base=0, robot_seeds=None, samples_per_robot=None, horizon=H):
    """normal4 for a whole call's array: (z, r) float64 [n_traj, horizon, 4].  robot_seeds: one seed per robot, keyed inside the
    robot (seed and traj_base are then ignored, as in the kernels)."""
    if robot_seeds is None:
        z, r = normal4(seed, draw, traj_points(traj_base, n_traj, horizon))
    else:
        assert n_traj == len(robot_seeds) * samples_per_robot
        pts = np.arange(samples_per_robot * horizon, dtype=np.uint64)
        parts = [normal4(s, draw, pts) for s in robot_seeds]
        z, r = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    return z.reshape(n_traj, horizon, 4), r.reshape(n_traj, horizon, 4)


RAW_TOL = 2.0 ** -20


def raw_bound(r):
    """|z_dev - z_ref| <= 2^-20 max(r, 1): logf, sincosf and the correctly rounded sqrtf are within 1-2 ulp each (documented figures
    of the device math library, no fast-math in the build), the product rounds once more: about 1.75 * 2^-22 * r in all; four times
    that.  A wrong constant, word or counter gives differences of order 1."""
    return RAW_TOL * np.maximum(r, 1.0)
