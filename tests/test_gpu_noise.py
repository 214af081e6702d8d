"""-m gpu: every consumer of the in-kernel Gaussian noise (csrc/guide_dev.h: normal4 / traj_normal4 -- Philox4x32-10 + Box-Muller)
against the host reference tests/philox_ref.py, which shares no code with the library: init_kernel (x_T, also through ddim_sample and
with per-robot streams), q_sample_kernel, and the step draws of mmd_p_sample_loop through the step fused into the UNet launch, the
persistent run and the cooperative, one-wave and binned guided step kernels, plus mmd_ddpm_step's own draw numbering.  The other
Philox tests compare one GPU path with another; these say what the noise must BE: counter = (point lo, draw, point hi, 0), key = seed,
draw 0xFFFFFFFF = x_T, 0xFFFFFFFE = q_sample, k = 0, 1, ... for the loop's steps and the loop index i for mmd_ddpm_step.

Bound of a raw draw: |z_dev - z_ref| <= 2^-20 max(r_ref, 1) (philox_ref.raw_bound: four times the documented libm error of logf /
sqrtf / sincosf and the product's rounding; a wrong constant, counter word or index gives differences of order 1).  A step is checked by
replaying it from the loop's own chain row with the REFERENCE noise injected, so nothing propagates from step to step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                                                        # noqa: E402
import cases                                                                     # noqa: E402
import parity_log                                                                # noqa: E402
import philox_ref as P                                                           # noqa: E402
from cases import H, D                                                           # noqa: E402

T, T_START_GUIDE = 25, 13
SEED_STREAM = (18 << 24) + 5                   # the shape next_stream_seed produces
SEED_HIGH = 0x9E3779B97F4A7C15                 # non-zero high key word
SEED_ONES = 0xFFFFFFFFFFFFFFFF                 # negative as a signed 64-bit value
F32_SUM = 2.0 ** -22                           # the last rounding(s) of a value x = v + c z computed in float32, relative to max(1, |x|)


def _half(t):
    return 0.5


def _model():
    import gpu_common
    return gpu_common.hip_model(T)


def _raw_check(case, dev, z, r, rows=None):
    """dev [n, H, D] device draws against the reference (z, r) [n, H, D]; rows: the support points compared (default all)"""
    dev = dev.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(dev).all(), case
    ratio = np.abs(dev - z) / np.maximum(r, 1.0)
    if rows is not None:
        ratio = ratio[:, rows]
    worst = float(ratio.max())
    print(f"philox {case}: max |dz| / max(r, 1) = {worst:.3e} = {worst / P.RAW_TOL:.3f} of the bound")
    parity_log.record("philox", case, None, worst, bound=P.RAW_TOL)
    assert worst <= P.RAW_TOL, (case, worst, P.RAW_TOL)


# ---- a. x_T -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 7, 2 ** 26 - 1, 2 ** 26], ids=["b0", "b7", "b2p26m1", "b2p26"])
@pytest.mark.parametrize("seed", [0, 123, SEED_STREAM, SEED_HIGH, SEED_ONES], ids=["s0", "s123", "stream", "high", "ones"])
def test_x_T_is_the_reference_draw(seed, base):
    """base 2^26 - 1: point index 2^32 - 1 is the last support point of trajectory 0, the rest of the batch has high word 1"""
    n = 5
    x = _model().p_sample_loop((n, H, D), {}, n_diffusion_steps=0, n_diffusion_steps_without_noise=0, seed=seed, traj_index_base=base)
    z, r = P.normal4(seed, P.DRAW_XT, base * 64 + np.arange(n * 64, dtype=np.uint64))
    _raw_check(f"x_T_seed{seed:x}_base{base}", x, z.reshape(n, H, D), r.reshape(n, H, D))


def test_x_T_with_hard_rows_and_through_ddim_sample():
    n, base = 5, 7
    hc = cases.hard_conds_for((-0.6, 0.3), (0.7, -0.2))
    z, r = P.traj_normal4(SEED_HIGH, P.DRAW_XT, n, traj_base=base)
    inner = np.arange(1, H - 1)
    model = _model()
    x, chain = model.p_sample_loop((n, H, D), hc, n_diffusion_steps=0, n_diffusion_steps_without_noise=0, seed=SEED_HIGH,
                                   traj_index_base=base, return_chain=True)
    assert chain.shape == (n, 1, H, D) and torch.equal(chain[:, 0], x)
    for row in (0, H - 1):
        assert torch.equal(x[:, row].cpu(), hc[row][None].expand(n, D)), row
    _raw_check("x_T_hard_rows", x, z, r, rows=inner)
    _, dchain = model.ddim_sample((n, H, D), hc, n_diffusion_steps=T, return_chain=True, seed=SEED_HIGH, traj_index_base=base)
    assert torch.isfinite(dchain).all()
    for row in (0, H - 1):
        assert torch.equal(dchain[:, 0, row].cpu(), hc[row][None].expand(n, D)), row
    _raw_check("x_T_ddim_chain0", dchain[:, 0], z, r, rows=inner)


# ---- b. per-robot streams ---------------------------------------------------------------------------------------------------------------
def test_per_robot_streams_are_keyed_inside_the_robot():
    R, B = 3, 5
    seeds = [SEED_STREAM, SEED_ONES, SEED_HIGH]
    x = _model().p_sample_loop((R * B, H, D), {}, n_diffusion_steps=0, n_diffusion_steps_without_noise=0, n_robots=R, robot_seeds=seeds,
                               seed=99, traj_index_base=1000)            # (both ignored under robot_seeds)
    for rb in range(R):
        z, r = P.normal4(seeds[rb], P.DRAW_XT, np.arange(B * 64, dtype=np.uint64))
        _raw_check(f"x_T_robot_stream{rb}", x[rb * B:(rb + 1) * B], z.reshape(B, H, D), r.reshape(B, H, D))


# ---- c. q_sample ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 11])
def test_q_sample_is_the_reference_draw(base):
    model, t, n, K = _model(), 3, 3, 2
    x0 = torch.from_numpy(synth.synth_noise(510, (n, K * H, D))) * 0.5
    out = model.q_sample(x0.cuda(), t, seed=SEED_HIGH, traj_index_base=base).cpu().numpy()
    z, r = P.normal4(SEED_HIGH, P.DRAW_Q_SAMPLE, base * 64 + np.arange(n * K * 64, dtype=np.uint64))
    z, r = z.reshape(n, K * H, D), r.reshape(n, K * H, D)
    a, b = np.float32(float(model.sqrt_alphas_cumprod[t])), np.float32(float(model.sqrt_one_minus_alphas_cumprod[t]))
    ref = a * x0.numpy() + b * z.astype(np.float32)                      # float32 throughout
    assert ref.dtype == np.float32 and np.isfinite(out).all()
    err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    bound = float(b) * P.raw_bound(r) + F32_SUM * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    worst = float((err / bound).max())
    print(f"philox q_sample base {base}: max err / bound = {worst:.3f}, max err {err.max():.3e}, b = {float(b):.4f}")
    parity_log.record("philox", f"q_sample_base{base}", t, worst, bound=1.0, note="err / (b * raw bound + 2^-22 max(1, |x|))")
    assert worst <= 1.0, (base, worst)
    # teeth: the sampler's x_T draw under the same seed is a different stream
    zT = P.normal4(SEED_HIGH, P.DRAW_XT, base * 64 + np.arange(n * K * 64, dtype=np.uint64))[0].reshape(n, K * H, D)
    assert np.abs(out - (a * x0.numpy() + b * zT.astype(np.float32))).max() > 0.05        # (b = 0.028 at t = 3)


# ---- d. the steps of mmd_p_sample_loop --------------------------------------------------------------------------------------------------
STEP_ROWS = (0, 11, 12, 13, 23, 24, 25)        # first step; last unguided, first two guided (t_start_guide = 13); last noisy; the two t = 0


def _robots(R, n_agents=None):
    """hard conditions of R robots on a circle of max(R, 6) and everybody's straight-line paths"""
    starts, goals = synth.start_goal_circle(n_agents or max(R, 6), 0.8)
    paths = synth.straight_line_paths(starts, goals, H)
    hc = {0: torch.stack([cases.hard_conds_for(starts[r], goals[r])[0] for r in range(R)]),
          H - 1: torch.stack([cases.hard_conds_for(starts[r], goals[r])[H - 1] for r in range(R)])}
    return hc, paths


def _soft_guide(R, paths):
    import gpu_common
    return gpu_common.hip_guide("EnvHighways2D", [[cases.soft_group(paths, r)] for r in range(R)], n_robots=R)


def _binned_guide(R, paths):
    import gpu_common
    from mmd_amd.constraints import binned_constraints_from_paths
    g = gpu_common.hip_guide("EnvHighways2D", [[] for _ in range(R)], n_robots=R)
    g.set_binned_constraints(binned_constraints_from_paths(torch.from_numpy(paths).cuda(), 0, R))
    return g


def _check_loop_steps(case, hc, R, B, seed, guide=None, flags=0, n_streams=0, traj_index_base=0, robot_seeds=None):
    from mmd_amd.diffusion_model import ddpm_sample_fn
    model, n = _model(), R * B
    tsg = T_START_GUIDE if guide is not None else float("inf")
    step_kw = dict(guide=guide, n_guide_steps=20, t_start_guide=tsg, noise_std_extra_schedule_fn=_half, n_robots=R)
    model.sampler_flags = flags
    try:
        _, chain = model.p_sample_loop((n, H, D), hc, n_diffusion_steps=T, return_chain=True, sample_fn=ddpm_sample_fn,
                                       n_diffusion_steps_without_noise=1, seed=seed, n_streams=n_streams,
                                       traj_index_base=traj_index_base, robot_seeds=robot_seeds, **step_kw)
    finally:
        model.sampler_flags = 0
    assert chain.shape == (n, T + 2, H, D) and torch.isfinite(chain).all()

    def noise(k):
        return P.traj_normal4(seed, k, n, traj_base=traj_index_base, robot_seeds=robot_seeds, samples_per_robot=B)

    def replay(k, z):
        x = chain[:, k].clone().contiguous()
        model.sample_step(x, hc, T - 1 - k, noise=torch.from_numpy(z.astype(np.float32)).cuda(), **step_kw)
        return x

    worst = 0.0
    for k in STEP_ROWS:
        i = T - 1 - k
        z, r = noise(k)
        x, want = replay(k, z), chain[:, k + 1]
        if i <= 0:                                                        # t = 0: no noise is drawn, the replay is the same arithmetic
            assert torch.equal(x, want), (case, k, float((x - want).abs().max()))
            continue
        sigma = float(np.exp(0.5 * float(model.posterior_log_variance_clipped[i])))
        want = want.cpu().numpy().astype(np.float64)
        err = np.abs(x.cpu().numpy().astype(np.float64) - want)
        bound = sigma * 0.5 * P.raw_bound(r) + F32_SUM * np.maximum(1.0, np.abs(want))
        ratio = float((err / bound).max())
        # the same difference read as a difference of the draw (it then also holds the float32 roundings of the step's last sum)
        dz = float((err / (sigma * 0.5 * np.maximum(r, 1.0))).max())
        print(f"philox {case} step k={k} i={i}: max err / bound = {ratio:.3f}, max err {err.max():.3e}, as |dz| / max(r, 1): {dz:.3e}")
        parity_log.record("philox", case, k, ratio, bound=1.0, dz_over_r=dz, sigma=sigma,
                          note="err / (sigma * 0.5 * raw bound + 2^-22 max(1, |x|))")
        assert ratio <= 1.0, (case, k, i, ratio)
        worst = max(worst, ratio)
    # teeth: row 11 replayed with the NEXT draw's noise is not the loop's row 12
    off = replay(11, noise(12)[0])
    assert float((off - chain[:, 12]).abs().max()) > 0.01, case
    return worst


def test_loop_steps_prior_only_fused_into_the_unet_launch():
    """n = 5: the UNet workgroup has waves without a trajectory"""
    _check_loop_steps("loop_prior_fused", _robots(1)[0], 1, 5, SEED_HIGH)


def test_loop_steps_prior_only_persistent_run():
    from mmd_amd import _lib
    _check_loop_steps("loop_prior_persist", _robots(1)[0], 1, 5, SEED_HIGH, flags=_lib.SAMPLER_PERSIST)


def test_loop_steps_guided_cooperative_kernel():
    hc, paths = _robots(2)
    _check_loop_steps("loop_guided_coop", hc, 2, 5, SEED_STREAM, guide=_soft_guide(2, paths))


def test_loop_steps_guided_one_wave_kernel():
    """640 trajectories in ONE launch (n_streams = 1): past the cooperative kernel's launch size"""
    hc, paths = _robots(10)
    _check_loop_steps("loop_guided_one_wave_640", hc, 10, 64, SEED_HIGH, guide=_soft_guide(10, paths), n_streams=1)


def test_loop_steps_two_stream_chunks():
    """the second chunk's launches start at trajectory traj0 = 16 of the arrays"""
    hc, paths = _robots(5)
    _check_loop_steps("loop_guided_two_chunks", hc, 5, 8, SEED_STREAM, guide=_soft_guide(5, paths), n_streams=2)


def test_loop_steps_with_a_trajectory_index_base():
    hc, paths = _robots(2)
    _check_loop_steps("loop_guided_base24", hc, 2, 5, SEED_STREAM, guide=_soft_guide(2, paths), traj_index_base=24)


def test_loop_steps_per_robot_streams():
    hc, paths = _robots(2)
    _check_loop_steps("loop_guided_robot_seeds", hc, 2, 5, 99, guide=_soft_guide(2, paths), robot_seeds=[SEED_HIGH, SEED_STREAM],
                      traj_index_base=1000)


def test_loop_steps_binned_constraint_table():
    hc, paths = _robots(2, n_agents=10)
    _check_loop_steps("loop_guided_binned", hc, 2, 5, SEED_STREAM, guide=_binned_guide(2, paths))


# ---- e. mmd_ddpm_step's own numbering ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided,base", [(False, 0), (True, 0), (True, 3)], ids=["prior", "guided", "guided_base3"])
def test_step_api_draws_by_the_loop_index(guided, base):
    model, R, B, i = _model(), 2, 5, 7
    n = R * B
    hc, paths = _robots(R)
    kw = dict(guide=_soft_guide(R, paths) if guided else None, n_guide_steps=20, t_start_guide=T_START_GUIDE if guided else float("inf"),
              noise_std_extra_schedule_fn=_half, n_robots=R)
    x0 = torch.from_numpy(synth.synth_noise(520, (n, H, D))) * 0.5
    x0[:, 0], x0[:, -1] = hc[0].repeat_interleave(B, 0), hc[H - 1].repeat_interleave(B, 0)
    own = model.sample_step(x0.clone().cuda(), hc, i, seed=SEED_HIGH, traj_index_base=base, **kw).cpu().numpy().astype(np.float64)
    z, r = P.traj_normal4(SEED_HIGH, i, n, traj_base=base)                # the draw is i = 7, not k = T - 1 - i = 17
    ref = model.sample_step(x0.clone().cuda(), hc, i, noise=torch.from_numpy(z.astype(np.float32)).cuda(), **kw).cpu().numpy().astype(np.float64)
    sigma = float(np.exp(0.5 * float(model.posterior_log_variance_clipped[i])))
    err = np.abs(own - ref)
    bound = sigma * 0.5 * P.raw_bound(r) + F32_SUM * np.maximum(1.0, np.abs(ref))
    ratio = float((err / bound).max())
    case = f"step_api_{'guided' if guided else 'prior'}_base{base}"
    print(f"philox {case} i={i}: max err / bound = {ratio:.3f}, max err {err.max():.3e}")
    parity_log.record("philox", case, i, ratio, bound=1.0, sigma=sigma, note="err / (sigma * 0.5 * raw bound + 2^-22 max(1, |x|))")
    assert ratio <= 1.0, (case, ratio)
    zk = P.traj_normal4(SEED_HIGH, T - 1 - i, n, traj_base=base)[0]
    off = model.sample_step(x0.clone().cuda(), hc, i, noise=torch.from_numpy(zk.astype(np.float32)).cuda(), **kw).cpu().numpy()
    assert np.abs(own - off).max() > 0.01


def test_step_api_last_step_draws_nothing():
    """i = -1 is passed on as draw 0xFFFFFFFF, the x_T draw's index: harmless only because t = 0 adds no noise"""
    model, R, B = _model(), 2, 5
    hc, _ = _robots(R)
    x0 = torch.from_numpy(synth.synth_noise(521, (R * B, H, D))) * 0.5
    a = model.sample_step(x0.clone().cuda(), hc, -1, seed=SEED_HIGH, noise_std_extra_schedule_fn=_half, n_robots=R)
    b = model.sample_step(x0.clone().cuda(), hc, -1, seed=123, noise_std_extra_schedule_fn=_half, n_robots=R)
    assert torch.isfinite(a).all() and torch.equal(a, b)
