"""Inputs that put the sampler's step arithmetic (tests/step_model.py) at its edges.  Host only: numpy, torch-CPU and the oracle.
tests/test_step_edges_host.py shows that every builder reaches both sides of its edge; tests/test_gpu_step_edges.py runs the kernels on them.

All inputs are small: B <= 24 trajectories, H = 64, a T = 25 schedule.  A test that needs crafted schedule coefficients overwrites the
model instance's `_tables` arrays in place (the sampler descriptor points at them) and puts them back (`tables_set`)."""
import contextlib

import numpy as np
import torch

import step_model as M
from mmd_amd import synth
from oracle import mmd_oracle as O

H, D = M.H, M.D
F32 = np.float32
T_STEPS = 25
FLT_MAX = np.finfo(np.float32).max
TINY = np.float32(1e-45)                   # the smallest denormal
NAN_WORD = 0x7FC01234                      # a quiet NaN with a payload
STEP_KEYS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
             "posterior_log_variance_clipped")


def ulps(x, k):
    x = F32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return F32(x)


@contextlib.contextmanager
def tables_set(model, **arrays):
    """model._tables[name][:] = array for the block, the model's own values afterwards"""
    saved = {k: model._tables[k].copy() for k in arrays}
    try:
        for k, v in arrays.items():
            model._tables[k][:] = np.asarray(v, F32)
        yield model
    finally:
        for k, v in saved.items():
            model._tables[k][:] = v


def identity_tables(T=T_STEPS):
    """a = 1, b = 0, c1 = 1, c2 = 0, log-variance 0 (sigma = expf(0) = 1): the DDPM step returns clamp(x) (+ z extra where it draws noise)"""
    one, zero = np.ones(T, F32), np.zeros(T, F32)
    return dict(sqrt_recip_alphas_cumprod=one, sqrt_recipm1_alphas_cumprod=zero, posterior_mean_coef1=one, posterior_mean_coef2=zero,
                posterior_log_variance_clipped=zero)


def real_tables(T=T_STEPS):
    return {k: np.ascontiguousarray(v.numpy(), dtype=F32) for k, v in O.schedule_tables(T).items()}


# ---- clamp ladder -------------------------------------------------------------------------------------------------------------------
LADDER = [ulps(s, k) for s in (1.0, -1.0) for k in (-2, -1, 0, 1, 2)] + \
         [F32(0.0), F32(-0.0), TINY, -TINY, F32(1e-40), F32(-1e-40), np.finfo(F32).tiny, -np.finfo(F32).tiny, F32(0.5), F32(-0.75)]
N_FINITE, ROW_HUGE, ROW_PINF, ROW_NINF, N_LADDER = 5, 5, 6, 7, 8


def clamp_ladder():
    """x [8, 64, 4]: rows 0 .. 4 cycle through LADDER (+-1 +- {0, 1, 2} ulp, +-0, denormals); row 5 holds +-FLT_MAX, rows 6 and 7 a few +inf / -inf
    among ordinary values -- the network's output for those three rows is not finite, so each keeps to a trajectory of its own"""
    x = np.zeros((N_LADDER, H, D), F32)
    flat = x[:N_FINITE].reshape(-1)
    flat[:] = np.asarray(LADDER, F32)[(np.arange(flat.size) * 7) % len(LADDER)]           # (7 and 20 coprime: every value in every channel)
    x[ROW_HUGE] = np.asarray([FLT_MAX, -FLT_MAX, 1.0, -0.25], F32)[(np.arange(H * D) % 4)].reshape(H, D)
    x[ROW_PINF:] = synth.synth_noise(301, (2, H, D)) * 0.5
    x[ROW_PINF, 5::16, 1] = np.inf
    x[ROW_NINF, 9::16, 2] = -np.inf
    return x


def sides_of_unit(v):
    """(# < -1, # == -1, # in (-1, 1), # == 1, # > 1) of the finite values"""
    v = np.asarray(v, np.float64)
    v = v[np.isfinite(v)]
    return int((v < -1).sum()), int((v == -1).sum()), int((np.abs(v) < 1).sum()), int((v == 1).sum()), int((v > 1).sum())


# ---- clamp with the real schedule and the real network ----------------------------------------------------------------------------
REAL_T = (0, 1, T_STEPS - 1)
N_REAL = 12
_SD = {}


def oracle_state_dict():
    if "sd" not in _SD:
        _SD["sd"] = O.state_dict_to_torch(synth.synth_unet_state_dict(0))
    return _SD["sd"]


def real_eps_input(t, T=T_STEPS):
    """x [12, 64, 4] for the DDPM step at time t on the seed-0 network: noise at scales 3 .. 0.05, so that x0 = a x - b eps spreads over both
    bounds and their inside where a is about 1 (t = 0, 1).  At t = T - 1, a = b = 4.6e3: x0 lies inside the clamp only where |x - eps(x)| < 2.2e-4,
    which no scaling reaches for more than a handful of elements (x <- (target + b eps(x)) / a does not contract on this network, nor does
    Newton's method on the CPU oracle); there both bounds are reached and the inside is the ladder's and the steps' t = 0, 1."""
    key = ("x", t, T)
    if key not in _SD:
        x = synth.synth_noise(310 + t, (N_REAL, H, D)).astype(F32)
        scales = np.asarray([3.0, 2.0, 1.5, 1.25, 1.0, 1.0, 0.875, 0.75, 0.5, 0.25, 0.05, 1e-3], F32)
        _SD[key] = x * scales[:, None, None]
    return _SD[key].copy()


def oracle_eps(x, t):
    return O.unet_forward(oracle_state_dict(), torch.from_numpy(np.asarray(x, F32)), torch.full((len(x),), int(t), dtype=torch.long)).numpy()


def clamp_counts(x, eps, a, b):
    """(# clamped at -1, # not clamped, # clamped at +1) of x0 = fma(a, x, -(b eps)) in fp32"""
    x0 = M.fma_f32(F32(a), x, -(F32(b) * np.asarray(eps, F32)))
    return int((x0 < -1).sum()), int((np.abs(x0) <= 1).sum()), int((x0 > 1).sum())


# ---- a network whose output is not finite in channel 0 --------------------------------------------------------------------------------
def nonfinite_state_dict(value):
    """the seed-0 weights with final_conv.1.bias[0] = value (NaN / +inf): eps is `value`-poisoned in channel 0 and finite in channels 1 .. 3"""
    sd = {k: np.array(v) for k, v in synth.synth_unet_state_dict(0).items()}
    sd["final_conv.1.bias"][0] = value
    return sd


def bias_only_state_dict():
    """the seed-0 weights with final_conv.1.weight = 0: eps is final_conv.1.bias in every element, whatever x is"""
    sd = {k: np.array(v) for k, v in synth.synth_unet_state_dict(0).items()}
    sd["final_conv.1.weight"][...] = 0.0
    return sd


def constant_eps_input(t=T_STEPS - 1, T=T_STEPS, n=N_REAL):
    """x [12, 64, 4] with a x - b bias = target, target uniform in +-1.5: the inside of the clamp and both bounds at the REAL coefficients of
    t = T - 1, which the real network's eps does not let an input reach (real_eps_input).  (x0 moves by a ulp(x) = 3e-5 per step of x.)"""
    tb = real_tables(T)
    a, b = np.float64(tb["sqrt_recip_alphas_cumprod"][t]), np.float64(tb["sqrt_recipm1_alphas_cumprod"][t])
    bias = synth.synth_unet_state_dict(0)["final_conv.1.bias"].astype(np.float64)
    target = np.random.default_rng(370).uniform(-1.5, 1.5, (n, H, D))
    return ((target + b * bias) / a).astype(F32)


# ---- noise ----------------------------------------------------------------------------------------------------------------------------
EXTRA_BY_T = (0.5 + np.arange(T_STEPS) / 32.0).astype(F32)          # distinct per t, exact in fp32


def noise_extra_fn(t):
    return float(EXTRA_BY_T[int(t)])


Z_PLANTS = [F32(0.0), F32(-0.0), F32(1e30), F32(-1e30), TINY, -TINY, F32(1e-40)]


def noise_input(B):
    """z [B, 64, 4]: ordinary normals with +-0 and denormals planted in every trajectory, +-1e30 in the last one only (the state it leaves is
    too large for the network: that trajectory is not finite in the steps that follow, the others do not see it)"""
    z = synth.synth_noise(330, (B, H, D)).astype(F32)
    for j in range(B):
        for k, v in enumerate(Z_PLANTS):
            if abs(v) < 1 or j == B - 1:
                z[j, (3 + 8 * k + j) % H, (k + j) % D] = v
    return z


# ---- pinned rows -------------------------------------------------------------------------------------------------------------------------
MASKS = [(), (0,), (63,), (0, 63), (1, 62), (31, 32), (0, 17, 40, 63), tuple(range(H))]
MASK_IDS = ["none", "r0", "r63", "r0_63", "r1_62", "r31_32", "r0_17_40_63", "all64"]
N_ROBOTS = 3
SPRS = (1, 6, 8)


def hard_values(rows, n_robots=N_ROBOTS, nan=True):
    """[n_robots, max(len(rows), 1), 4] fp32: a distinct value per (robot, slot, dim); -0.0 at (robot 0, slot 0, dim 0) and, with `nan`, a
    NaN with a payload at (robot 1, last slot, dim 1) -- the network's output for robot 1's trajectories is then NaN everywhere, and what
    is left to compare in them is the pinned rows' words"""
    n = max(len(rows), 1)
    r, s, d = np.meshgrid(np.arange(n_robots), np.arange(n), np.arange(D), indexing="ij")
    hard = ((r + 1) / 4.0 - 0.5 + (s + 1) / 256.0 + (d + 1) / 4096.0).astype(F32) * np.where((r + s + d) % 2, -1, 1).astype(F32)
    if len(rows):
        hard[0, 0, 0] = -0.0
        if nan:
            hard[1, n - 1, 1:2].view(np.uint32)[:] = NAN_WORD
    return hard


def hard_conds(rows, hard):
    """the dict apply_hard_conditioning takes: {row: [n_robots, 4]}, rows in ANY order (the table's slots are the sorted rows)"""
    order = sorted(rows)
    return {int(t): torch.from_numpy(hard[:, order.index(t)].copy()) for t in sorted(rows, key=lambda t: (t * 37) % 64)}


def step_input(B, seed=340):
    return (synth.synth_noise(seed, (B, H, D)) * 0.6).astype(F32)


# ---- cross conditioning --------------------------------------------------------------------------------------------------------------
def boundary_of(rel):
    """sample_functions.py:24-26 in fp32: rel / ||rel||, a zero component -> 1e6"""
    rel = torch.tensor(np.asarray(rel, F32))
    bnd = rel / torch.norm(rel, keepdim=True)
    bnd[bnd == 0] = 1e6
    return bnd.numpy().astype(F32)


CROSS_RELS = {"fwd": (2.0, 0.0, 0.0, 0.0), "rev": (-2.0, 0.0, 0.0, 0.0), "diag": (1.5, -2.0, 0.0, 0.0)}
CROSS_N = (1, 255, 256, 257)
CROSS_SPECIALS = [np.nan, np.inf, -np.inf]


def cross_input(rel, ind1, ind2, n=257, seed=350):
    """x1, x2 [n, 64, 4]: ordinary tiles; the stitch row x2[:, ind2] holds, trajectory by trajectory, v2 with v2 + rel at boundary + {-2 .. 2}
    ulp (as far as fp32 lets the sum land there: the host test counts both sides), at -boundary likewise, and NaN / +inf / -inf."""
    rel = np.asarray(rel, F32)
    bnd = boundary_of(rel)
    x1 = (synth.synth_noise(seed, (n, H, D)) * 0.5).astype(F32)
    x2 = (synth.synth_noise(seed + 1, (n, H, D)) * 0.5).astype(F32)
    for j in range(n):
        kind = j % 16
        for c in range(D):
            if kind < 5:                                                            # (v2's own neighbours: the sum moves by v2's ulp)
                x2[j, ind2, c] = ulps(F32(np.float64(bnd[c]) - np.float64(rel[c])), kind - 2)
            elif kind < 10:
                x2[j, ind2, c] = F32(np.float64(ulps(-bnd[c], kind - 7)))       # v1 - rel = v2 again where the min did not act
            elif kind < 13 and c == (j // 16) % D:
                x2[j, ind2, c] = CROSS_SPECIALS[kind - 10]
    return x1, x2, rel, bnd


def by_robot_table():
    """[2, 8]: robot 0 stitches with the forward offset, robot 1 with the diagonal one"""
    return np.stack([np.concatenate([np.asarray(CROSS_RELS[k], F32), boundary_of(CROSS_RELS[k])]) for k in ("fwd", "diag")]).astype(F32)


# ---- q_sample ------------------------------------------------------------------------------------------------------------------------------
Q_N = (1, 4, 5)                                                       # n_pts = 64, 256 (one block), 320


def q_input(n):
    x0 = (synth.synth_noise(360, (n, H, D)) * 0.7).astype(F32)
    z = synth.synth_noise(361, (n, H, D)).astype(F32)
    x0[0, 0, 0], x0[0, 1, 1], z[0, 2, 2], z[0, 3, 3] = 0.0, -0.0, 0.0, 1e-40
    return x0, z
