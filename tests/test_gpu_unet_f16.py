"""-m gpu: TemporalUnet(precision="f16") -- the opt-in mixed-precision form of the fused forward (unet_f16.hip: one fp16 piece per conv
operand, one MFMA per product, fp32 accumulation; mmd_unet_options.precision).  It is NOT held to the fp32 parity bars: it is
held to the CPU emulation of the same rounding (tests/test_unet_precision_host.py), to itself across its three launch forms, to the f32
mode through the algebra of the shared DDPM step, to the reference's output distribution, and through the planners."""
import os
from math import ceil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases                             # noqa: E402
import parity_log                        # noqa: E402
import test_unet_precision_host as emu   # noqa: E402  (the emulation helpers; its tests are not collected through this name)
from cases import GOLDEN, H, D, rel_l2   # noqa: E402
from mmd_amd import _lib, synth          # noqa: E402
from mmd_amd.diffusion_model import GaussianDiffusionModel, ddpm_sample_fn   # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet                               # noqa: E402
from oracle import mmd_oracle as O       # noqa: E402

_MODELS = {}


def _model(precision, T=100, sd_np=None, key=0, **unet_kw):
    k = (precision, T, key, tuple(sorted(unet_kw.items())))
    if k not in _MODELS:
        unet = TemporalUnet(state_dim=4, n_support_points=64, unet_input_dim=32, dim_mults=(1, 2, 4), precision=precision, **unet_kw)
        unet.load_state_dict(sd_np if sd_np is not None else synth.synth_unet_state_dict(0))
        _MODELS[k] = GaussianDiffusionModel(model=unet, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True)
    return _MODELS[k]


def _wide_state_dict():
    """the "wide" weight set of test_unet_forward_accuracy_against_fp64: k = 5 conv kernels spread over five orders of magnitude"""
    wide = synth.synth_unet_state_dict(2)
    rng = np.random.Generator(np.random.PCG64(9))
    for k, v in wide.items():
        if k.endswith(".block.0.weight"):
            wide[k] = (v * np.exp(rng.uniform(-6.0, 2.0, size=v.shape))).astype(np.float32)
    return wide


def test_f16_mode_is_on_and_within_twice_its_emulation():
    """err16 = f16 kernels vs the float64 oracle; emu = the float64 oracle with the SAME operands rounded once to fp16 vs the float64
    oracle.  err16 <= 2 emu: the factor covers what the emulation does not share with the kernels (summation order, the exact scale
    exponents), it is a margin and not a measurement.  And the mode is really on: its output differs from the f32 mode's."""
    t = torch.full((16,), 41, dtype=torch.long)
    lib = _lib.load()
    for name, sd_np, scales in (("seed0", synth.synth_unet_state_dict(0), (1.0, 1e-3, 8.0)), ("wide", _wide_state_dict(), (1.0,))):
        m16, m32 = _model("f16", sd_np=sd_np, key=name), _model("f32", sd_np=sd_np, key=name)
        assert lib.mmd_unet_precision(m16.model.handle(100, "cuda")) == 1 and lib.mmd_unet_precision(m32.model.handle(100, "cuda")) == 0
        assert m16.model.handle(100, "cuda").value != m32.model.handle(100, "cuda").value
        sd64 = {k: v.double() for k, v in O.state_dict_to_torch(sd_np).items()}
        for scale in scales:
            x = torch.from_numpy(synth.synth_noise(300, (16, H, D))) * scale
            ref64 = O.unet_forward(sd64, x.double(), t)
            e_emu = emu.rel64(emu.f16_emulated_forward(sd64, x.double(), t), ref64)
            out16, out32 = m16.model(x.cuda(), 41).cpu(), m32.model(x.cuda(), 41).cpu()
            assert torch.isfinite(out16).all()
            err16, err32, diff = emu.rel64(out16, ref64), emu.rel64(out32, ref64), rel_l2(out16, out32)
            print(f"unet_f16_vs_fp64 {name} scale={scale:g}: err16 {err16:.3e} emu {e_emu:.3e} ratio {err16 / e_emu:.2f} err32 {err32:.3e} "
                  f"f16-vs-f32 {diff:.3e}")
            parity_log.record("unet_f16_vs_fp64", f"{name} scale={scale:g}", None, err16, sens=e_emu, bound=2 * e_emu, err_f32=err32,
                              f16_vs_f32=diff, note="sens = the float64 oracle with conv operands rounded once to fp16 (CPU emulation of the mode)")
            assert diff > 1e-5, (name, scale, diff)
            assert err16 <= 2 * e_emu, (name, scale, err16, e_emu)


def test_f16_launch_forms_agree_bitwise():
    """The same 5 trajectories through unet_kernel<1> (a batch of 5), <2> (the first 5 of 257: odd tail) and <4> (a batch of 7 with
    two_per_workgroup_max = -1: one full and one partial workgroup) of the f16 build: identical eps rows, as in f32 mode."""
    x = torch.from_numpy(synth.synth_noise(91, (257, H, D))).cuda()
    m = _model("f16")
    one = m.model(x[:5].contiguous(), 41)
    two = m.model(x, 41)
    four = _model("f16", two_per_workgroup_max=-1).model(x[:7].contiguous(), 41)
    assert torch.isfinite(two).all()
    assert torch.equal(one, two[:5]) and torch.equal(one, four[:5])
    assert torch.equal(two[5:7], four[5:7])
    assert not torch.equal(one, _model("f32").model(x[:5].contiguous(), 41))


def test_f16_step_algebra_is_the_shared_one():
    """One unguided DDPM step at i = 20 of T = 25 from the same x with the same injected noise in both precisions: ddpm_mean1 is
    c1 clamp(a x - b eps) + c2 x and the clamp is 1-Lipschitz, so |x_next,f16 - x_next,f32| <= c1 b |eps_f16 - eps_f32| elementwise
    (+ fp32 rounding); pinned rows are the hard conditions.  Through the separate step kernel (sample_step) and through the fused tail
    (the first step of a p_sample_loop that starts at i = 20: chain row 1), bitwise the same in f16."""
    T, i, B, R = 25, 20, 8, 2
    n = B * R
    starts, goals = synth.start_goal_circle(6, 0.8)
    hc = {0: torch.stack([cases.hard_conds_for(starts[r], goals[r])[0] for r in range(R)]),
          H - 1: torch.stack([cases.hard_conds_for(starts[r], goals[r])[H - 1] for r in range(R)])}
    x = torch.from_numpy(synth.synth_noise(70, (n, H, D))) * 0.7
    x[:, 0], x[:, -1] = hc[0].repeat_interleave(B, 0), hc[H - 1].repeat_interleave(B, 0)
    noise = torch.from_numpy(synth.synth_noise(71, (i + 1, n, H, D)))
    nfn = lambda t: 0.5                                                           # noqa: E731
    tb = O.schedule_tables(T)
    c1b = float(tb["posterior_mean_coef1"][i]) * float(tb["sqrt_recipm1_alphas_cumprod"][i])
    res = {}
    for prec in ("f32", "f16"):
        m = _model(prec, T)
        eps = m.model(x.cuda(), i).cpu()
        y = m.sample_step(x.clone().cuda(), hc, i, noise_std_extra_schedule_fn=nfn, n_robots=R, noise=noise[0].cuda()).cpu()
        _, chain = m.p_sample_loop((n, H, D), hc, i + 1, return_chain=True, warm_start_path_b=x.cuda(), n_robots=R,
                                   noise_std_extra_schedule_fn=nfn, step_noise=noise.cuda())
        res[prec] = (eps, y, chain[:, 1].cpu(), chain[:, 0].cpu())
    for prec in res:
        eps, y, y_loop, x0 = res[prec]
        assert torch.equal(x0, x) and torch.isfinite(y).all()
        assert torch.equal(y, y_loop), prec                                      # step kernel == fused tail
        assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(y[:, -1], x[:, -1])  # pinned rows: the hard conditions
    d_eps = (res["f16"][0] - res["f32"][0]).abs()[:, 1:-1]
    d_x = (res["f16"][1] - res["f32"][1]).abs()[:, 1:-1]
    slack = d_x - (c1b * d_eps * (1 + 1e-5) + 1e-6)
    print(f"step algebra: c1*b {c1b:.4f}, max |d eps| {float(d_eps.max()):.3e}, max |d x| {float(d_x.max()):.3e}, max slack {float(slack.max()):.3e}")
    assert float(d_eps.max()) > 0 and float(slack.max()) <= 0, float(slack.max())


def test_f16_guided_sampling_keeps_the_reference_distribution():
    """The first case of tests/test_gpu_distribution.py with the f16 model: the same five z-statistics against the reference's own
    sample (the golden), each below Z_MAX."""
    from mmd_amd import postprocess as post
    import gpu_common
    name = cases.DIST_CASES[0]
    g = np.load(os.path.join(GOLDEN, f"g15_distribution_{name}.npz"))
    T, B, n_seeds, base = (int(v) for v in g["meta"])
    case = dict(cases.sample_case(name))
    assert case["T"] == T
    n = n_seeds * B
    xT, steps = cases.distribution_inputs(T, B, n_seeds, base)
    guide = gpu_common.hip_guide(case["map"], [case["cons"]], case.get("cutoff", 0.05))
    final = _model("f16", T).run_inference(None, cases.hard_conds_for(case["start"], case["goal"]), n_samples=n, horizon=64, return_chain=True,
                                           sample_fn=ddpm_sample_fn, guide=guide, n_guide_steps=20, t_start_guide=ceil(0.5 * T),
                                           noise_std_extra_schedule_fn=lambda x: 0.5, n_diffusion_steps_without_noise=1,
                                           warm_start_path_b=xT.cuda(), step_noise=steps.cuda())[-1]
    assert final.shape == (n, H, D) and torch.isfinite(final).all()
    ref = torch.from_numpy(g["finals"])
    pos_ref = cases.unnormalize(ref)[..., :2].numpy()
    pos_hip = cases.unnormalize(final.cpu())[..., :2].numpy()
    z_mean, z_cov = cases.distribution_z(pos_hip, pos_ref)
    r = post.postprocess_batch(gpu_common.hip_guide(case["map"], [case["cons"]]), cases.unnormalize(final.cpu()).cuda().contiguous(),
                               n_robots=1, smooth=False)
    free_hip, free_ref = int(r.free_mask.bool().sum()), int(g["free_mask"].sum())
    viol_hip, viol_ref = cases.violation_counts(pos_hip, case["cons"]), g["violations"]
    z_free = cases.proportion_z(free_hip, free_ref, n)
    z_viol = cases.proportion_z(int((viol_hip > 0).sum()), int((viol_ref > 0).sum()), n)
    z_pairs = cases.mean_z(viol_hip, viol_ref)
    per = np.array([rel_l2(final[j].cpu(), ref[j]) for j in range(n)])
    for key, val in (("z_mean", z_mean), ("z_cov", z_cov), ("z_free", z_free), ("z_violating", z_viol), ("z_violation_pairs", z_pairs)):
        print(f"f16 distribution {name} {key} {val:.3f}")
        parity_log.record("f16_distribution_vs_reference", f"{name}_{key}", None, val, bound=cases.Z_MAX)
    print(f"f16 distribution {name}: matched within 1e-3: {int((per < 1e-3).sum())} of {n}, median rel-L2 {np.median(per):.2e}")
    parity_log.record("f16_distribution_vs_reference", f"{name}_matched_within_1e-3", None, float((per < 1e-3).mean()),
                      note=f"f16 precision mode; free {free_hip} / {free_ref} of {n}; median matched rel-L2 {np.median(per):.2e}")
    assert z_mean < cases.Z_MAX and z_cov < cases.Z_MAX, (z_mean, z_cov)
    assert z_free < cases.Z_MAX, (free_hip, free_ref)
    assert z_viol < cases.Z_MAX and z_pairs < cases.Z_MAX, (z_viol, z_pairs)


def test_f16_planners():
    """MPD(unet_precision="f16") on EnvHighways2D, B = 64: finite, start / goal rows exact, the f32 call's shapes; plan_batched of two f16
    calls == the calls in sequence; an f32 and an f16 call in one list are not packed together (different device models) and equal their
    sequential results."""
    from mmd_amd.planners import MPD, _batch_key, plan_batched
    starts, goals = synth.start_goal_circle(10, 0.45)

    def mpd(r, seed, **over):
        kw = dict(model_id="EnvHighways2D-RobotPlanarDisk", planner_alg="mmd", start_state_pos=torch.as_tensor(starts[r]),
                  goal_state_pos=torch.as_tensor(goals[r]), device="cuda", seed=seed, n_samples=64,
                  model_state_dict=synth.synth_unet_state_dict(0), model_args=dict(n_diffusion_steps=25), trained_models_dir="")
        kw.update(over)
        return MPD(**kw)
    p16, q16, p32 = mpd(1, 18, unet_precision="f16"), mpd(4, 19, model_args=dict(n_diffusion_steps=25, unet_precision="f16")), mpd(1, 18)
    assert p16.model.model.precision == "f16" and q16.model.model.precision == "f16" and p32.model.model.precision == "f32"
    call = lambda p, r: (p, torch.from_numpy(starts[r]), torch.from_numpy(goals[r]))   # noqa: E731
    o16, o32 = p16(*call(p16, 1)[1:], seed=700), p32(*call(p32, 1)[1:], seed=700)
    assert torch.isfinite(o16.trajs_iters).all() and torch.isfinite(o16.trajs_final).all()
    assert o16.trajs_iters.shape == o32.trajs_iters.shape and o16.trajs_final.shape == o32.trajs_final.shape
    assert o16.trajs_iters.shape[1] == 64 and not torch.equal(o16.trajs_iters[-1], o32.trajs_iters[-1])
    for o in (o16, o32):                                                           # start and goal: the pinned rows, whatever the precision
        last = o.trajs_iters[-1]
        assert torch.equal(last[:, 0], o32.trajs_iters[-1][:, 0]) and torch.equal(last[:, -1], o32.trajs_iters[-1][:, -1])
        assert torch.equal(last[:, 0], last[:1, 0].expand_as(last[:, 0])) and torch.equal(last[:, -1], last[:1, -1].expand_as(last[:, -1]))
    # (and they are the start / goal up to the normaliser's fp32 round trip: the bound tests/test_gpu_planners.py holds the f32 planners to)
    pos = o16.trajs_iters[-1][..., :2].cpu()
    assert torch.allclose(pos[:, 0], torch.from_numpy(starts[1]).expand(64, 2), atol=1e-5)
    assert torch.allclose(pos[:, -1], torch.from_numpy(goals[1]).expand(64, 2), atol=1e-5)

    def same(a, b):
        assert torch.equal(a.trajs_iters, b.trajs_iters) and torch.equal(a.trajs_final, b.trajs_final)
        assert torch.equal(a.trajs_final_free_idxs, b.trajs_final_free_idxs)
    calls = [call(p16, 1), call(q16, 4)]
    assert _batch_key(calls[0]) == _batch_key(calls[1]) and _batch_key(calls[0]) != _batch_key(call(p32, 1))
    seq = [c[0](*c[1:], seed=s) for c, s in zip(calls, (801, 802))]
    for a, b in zip(seq, plan_batched(calls, seeds=(801, 802))):
        same(a, b)
    mixed = [call(p32, 1), call(q16, 4)]
    seqm = [c[0](*c[1:], seed=s) for c, s in zip(mixed, (803, 802))]
    for a, b in zip(seqm, plan_batched(mixed, seeds=(803, 802))):
        same(a, b)
    same(seqm[1], seq[1])
