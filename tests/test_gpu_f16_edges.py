"""-m gpu: TemporalUnet(precision="f16") -- the second build of csrc/unet_kernel.h (csrc/unet_f16.hip: one fp16 piece per operand) -- at
the edges the f32 build is held to, and on every launch path it has.

tests/test_gpu_unet_f16.py runs the mode on the two benign weight sets only.  Here it runs on the 20 weight sets of
tests/fused_edge_cases.py (static scales from 2^-4 to 2^8, pre-activations past the Mish's clamp, constant GroupNorm groups, all-zero
weight columns), the nine finite edge rows, every time step of the time-bias set, inf / NaN rows that share a workgroup with finite
ones, and through the sampler's persistent, fused and step-kernel paths, stream chunks, a captured graph, the torch op and DDIM.

What the mode is held to (tests/f16_edge_cases.py, checked on the references alone by tests/test_f16_edges_host.py): finite output;
the error against float64 at most f16_limit = max(bound(err_ref32), 2 x sens), sens the larger error of the one-piece CPU emulation in
float64 and in float32 arithmetic; rows that do not see their neighbours; and the same bits on all of its own paths.  A comparison of
the whole network against the emulation itself cannot be sharper than that (the two arithmetics of the emulation lie as far from each
other as from float64) and is not attempted.  Every forward has at most 6 rows but one launch of 257 per set (unet_kernel<2>)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, synth                                               # noqa: E402
from mmd_amd.diffusion_model import GaussianDiffusionModel, ddpm_sample_fn    # noqa: E402
from mmd_amd.schedules import SCHEDULE_KEYS                                   # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet                                # noqa: E402
from oracle import mmd_oracle as O                                            # noqa: E402
import cases                                                                  # noqa: E402
import f16_edge_cases as F                                                    # noqa: E402
import fused_edge_cases as E                                                  # noqa: E402
import layered_edge_cases as L                                                # noqa: E402
import parity_log                                                             # noqa: E402
from cases import H, D                                                        # noqa: E402

_UNETS, _MODELS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _unet(wset, T=E.T_STEPS, precision="f16", **options):
    key = (wset, T, precision, tuple(sorted(options.items())))
    if key not in _UNETS:
        u = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=E.UID, dim_mults=E.DM, precision=precision, **options)
        u.load_state_dict(E.state_dict(wset))
        h = u.handle(T, "cuda")                    # the static scales rest on the time biases of steps 0 .. T - 1
        assert _lib.load().mmd_unet_precision(h) == _lib.UNET_PRECISIONS[precision]
        _UNETS[key] = u
    return _UNETS[key]


def _model(T, precision="f16", schedule="exponential", **options):
    """GaussianDiffusionModel on the seed-0 weights; a model of its own per option set (sampler_flags is a field of the object)"""
    key = (T, precision, schedule, tuple(sorted(options.items())))
    if key not in _MODELS:
        unet = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=E.UID, dim_mults=E.DM, precision=precision, **options)
        unet.load_state_dict(synth.synth_unet_state_dict(0))
        _MODELS[key] = GaussianDiffusionModel(model=unet, variance_schedule=schedule, n_diffusion_steps=T, predict_epsilon=True)
        assert all(torch.isfinite(getattr(_MODELS[key], k)).all() for k in SCHEDULE_KEYS), (T, schedule)
    return _MODELS[key]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_case(test, case, out, out32=None):
    """finite, and within f16_limit of float64; the figures go to the parity table"""
    name = F.case_name(case)
    assert torch.isfinite(out).all(), name
    err16, sens, limit = F.err_against_fp64(out, case), F.sens(case), F.f16_limit(case)
    extra = {} if out32 is None else dict(err_f32=F.err_against_fp64(out32, case))
    print(f"{name}: err16 {err16:.3g} sens {sens:.3g} ratio {err16 / sens:.2f} limit {limit:.3g}"
          + "".join(f" {k} {v:.3g}" for k, v in extra.items()))
    parity_log.record(test, name, None, err16, sens=sens, bound=limit, err_ref32=F.reference_errors(case)[0],
                      note="sens = the one-piece CPU emulation against the same float64 forward, the larger of its float64- and float32-arithmetic forms",
                      **extra)
    assert err16 <= limit, (name, err16, sens, limit)


# ---- 1. accuracy against float64
@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_f16_forward_accuracy_against_fp64(wset):
    """f16 unet_kernel<1> at n = 6 on every set x inputs scaled by 1, 1e-3 and 8: finite, within f16_limit, and really the f16 build
    (its bits differ from the f32 build's on the same input).
    Measured (profiles/f16_edges_parity.json): err16 1.8e-5 (beta-8) .. 3.9e-3 (gamma_x64 at scale 1e-3), err16 / sens 0.94 .. 1.04 over the
    60 cases (edge rows 0.94 .. 1.05, time steps 0.96 .. 1.04); none above 1.5.  The f32 build on the same inputs: 2.5e-8 .. 9.1e-4."""
    u16, u32 = _unet(wset), _unet(wset, precision="f32")
    assert u16.handle(E.T_STEPS, "cuda").value != u32.handle(E.T_STEPS, "cuda").value
    for scale in E.SCALES:
        x = E.accuracy_input(scale).cuda()
        out16, out32 = u16(x, E.T_STEP).cpu(), u32(x, E.T_STEP).cpu()
        _check_case("f16_edges_vs_fp64", ("set", wset, scale), out16, out32)
        assert not same_bits(out16, out32), (wset, scale)


# ---- 2. the launch forms agree
def forward_forms(wset, x, t, precision="f16"):
    """x [n <= 6, H, D] (cpu) through unet_kernel<1> (one launch of n), <4> (two_per_workgroup_max = -1: at n = 6 a full workgroup and
    a ragged one) and <2> (one launch of 257: the rows + ordinary filler rows behind them)"""
    n = x.shape[0]
    filler = torch.from_numpy(synth.synth_noise(179, (257 - n, H, D)))
    one = _unet(wset, precision=precision)
    return {1: one(x.cuda(), t).cpu(), 4: _unet(wset, precision=precision, two_per_workgroup_max=-1)(x.cuda(), t).cpu(),
            2: one(torch.cat([x, filler]).cuda(), t).cpu()[:n]}


@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_f16_launch_forms_agree_bit_for_bit(wset):
    outs = forward_forms(wset, E.accuracy_input(1.0), E.T_STEP)
    assert all(torch.isfinite(o).all() for o in outs.values()), wset
    for i in range(E.N_ACC):
        assert same_bits(outs[1][i], outs[4][i]) and same_bits(outs[1][i], outs[2][i]), (wset, i)


# ---- 3. the edge rows
def test_f16_every_finite_edge_row_is_within_the_limit():
    """zero, -0.0, 2^-70, 2^-20, 1e-3, one, eight, 2^30 and neg_max of edge_batch() on seed 0 at T_EDGE, row by row"""
    x = E.edge_rows()
    unet = _unet("seed0")
    out = torch.cat([unet(x[i:i + 5].cuda(), E.T_EDGE).cpu() for i in (0, 5)])
    for j, name in enumerate(L.FINITE_ROWS):
        _check_case("f16_edges_rows_vs_fp64", ("row", name), out[j])


def forward_with(kernel, x):
    """x [N, H, D] (cpu) through f16 unet_kernel<kernel> at T_EDGE in the launches of tests/test_gpu_unet_scale_edges.py, whose row order
    puts the inf / NaN samples into workgroups with finite ones: launches of 3 (<1>), of 5 (<4>: rows 5 .. 8 are one workgroup), one
    launch of 257 (<2>: rows (5, 6) and (7, 8) are two workgroups)"""
    unet = _unet("seed0", two_per_workgroup_max=-1) if kernel == 4 else _unet("seed0")
    n = x.shape[0]
    if kernel == 2:
        filler = torch.from_numpy(synth.synth_noise(179, (257 - n, H, D)))
        return unet(torch.cat([x, filler]).cuda(), E.T_EDGE).cpu()[:n]
    per = 3 if kernel == 1 else 5
    out = []
    for i in range(0, n, per):
        rows = x[i:i + per]
        pad = per - rows.shape[0]
        if pad:
            rows = torch.cat([rows, x[:pad]])
        out.append(unet(rows.contiguous().cuda(), E.T_EDGE).cpu()[:per - pad])
    return torch.cat(out)


@pytest.fixture(scope="module")
def edge_outs():
    xe, xp = L.edge_batch(), L.plain_batch()
    return {"edge": {k: forward_with(k, xe) for k in (1, 2, 4)}, "plain": {k: forward_with(k, xp) for k in (1, 2, 4)}}


def test_f16_edge_batch_rows_identical_across_forms(edge_outs):
    for which in ("edge", "plain"):
        o = edge_outs[which]
        for i, name in enumerate(L.NAMES):
            assert same_bits(o[1][i], o[2][i]) and same_bits(o[1][i], o[4][i]), (which, name)


def test_f16_finite_rows_do_not_see_inf_nan_neighbours(edge_outs):
    """inf / NaN rows come out non-finite in every element, every other row finite and with the bits it has next to ordinary samples"""
    for k in (1, 2, 4):
        o, p = edge_outs["edge"][k], edge_outs["plain"][k]
        for i, name in enumerate(L.NAMES):
            if name in L.NON_FINITE:
                assert not torch.isfinite(o[i]).any(), (k, name)
            else:
                assert torch.isfinite(o[i]).all() and same_bits(o[i], p[i]), (k, name)


# ---- 4. every time step on the time-bias set
def test_f16_every_time_step_on_the_time_bias_set():
    unet = _unet(E.TIME_SET, T=E.TIME_T)
    xd = E.time_step_input().cuda()
    for t in range(E.TIME_T):
        _check_case("f16_edges_time_steps", ("t", t), unet(xd, t).cpu())


# ---- 5. the sampler's paths, bit for bit within f16
def _robots(R):
    starts, goals = synth.start_goal_circle(6, 0.8)
    paths = synth.straight_line_paths(starts, goals, H)
    hc = {0: torch.stack([cases.hard_conds_for(starts[r], goals[r])[0] for r in range(R)]),
          H - 1: torch.stack([cases.hard_conds_for(starts[r], goals[r])[H - 1] for r in range(R)])}
    return paths, hc


def _guide(paths, R):
    import gpu_common
    return gpu_common.hip_guide("EnvHighways2D", [[cases.soft_group(paths, r)] for r in range(R)], n_robots=R)


def _hard_rows_exact(chain, hc, B):
    """chain [rows, n, H, D]: the pinned support points of every row are the hard conditions, bit for bit"""
    for row in (0, H - 1):
        want = hc[row].repeat_interleave(B, 0).to(chain.device)
        if not torch.equal(chain[:, :, row], want[None].expand_as(chain[:, :, row])):
            return False
    return True


GUIDED = dict(horizon=H, return_chain=True, sample_fn=ddpm_sample_fn, n_guide_steps=20, t_start_guide=13,
              noise_std_extra_schedule_fn=lambda t: 0.5, n_diffusion_steps_without_noise=1)
FLAGS = (0, _lib.SAMPLER_PERSIST, _lib.SAMPLER_NO_FUSED_STEP)


@pytest.mark.parametrize("R,B,options", [(2, 8, {}), (1, 7, dict(two_per_workgroup_max=-1))], ids=["persist2_R2xB8", "persist4_n7"])
def test_f16_persistent_fused_and_step_kernel_chains_are_equal(R, B, options):
    """A guided T = 25 call (12 leading unguided steps, then 14 guided ones), in-kernel Philox noise, the whole chain: one launch per
    step with the step fused into the forward's tail (flags 0), the unguided run in ONE persistent launch (unet_persist_kernel<2> at
    16 trajectories, <4> on the two_per_workgroup_max = -1 model at 7: a full workgroup and a ragged one) and separate step-kernel
    launches give the same bits; the result differs from the f32 build's."""
    T = 25
    model = _model(T, **options)
    paths, hc = _robots(R)
    guide = _guide(paths, R)
    res = {}
    try:
        for flags in FLAGS:
            model.sampler_flags = flags
            res[flags] = model.run_inference(None, hc, n_samples=B, n_robots=R, guide=guide, seed=91, **GUIDED).cpu()
    finally:
        model.sampler_flags = 0
    assert res[0].shape == (T + 2, R * B, H, D) and torch.isfinite(res[0]).all()
    for flags in FLAGS:
        assert same_bits(res[0], res[flags]), flags
        assert _hard_rows_exact(res[flags], hc, B), flags
    ref32 = _model(T, "f32", **options).run_inference(None, hc, n_samples=B, n_robots=R, guide=guide, seed=91, **GUIDED).cpu()
    assert same_bits(res[0][0], ref32[0]) and not same_bits(res[0][1], ref32[1])          # the same x_T, another eps


def test_f16_prior_only_persistent_runs_of_64_and_7_steps():
    """A prior-only call on a T = 70 model with injected noise: 71 unguided steps, under MMD_SAMPLER_PERSIST a run of 64 steps and one
    of 7 (PERSIST_MAX_STEPS = 64), against the launch-per-step forms.  The cosine schedule: the exponential one's last beta rounds to
    1 + 2^-23 in fp32 for T = 64 .. 75 (as the reference's does), alpha goes negative and four of its tables are NaN whatever the
    precision."""
    T, R, B = 70, 2, 8
    model = _model(T, schedule="cosine")
    _, hc = _robots(R)
    xT = torch.from_numpy(synth.synth_noise(130, (R * B, H, D))).cuda()
    st = torch.from_numpy(synth.synth_noise(131, (T + 1, R * B, H, D))).cuda()
    res = {}
    try:
        for flags in FLAGS:
            model.sampler_flags = flags
            res[flags] = model.run_inference(None, hc, n_samples=B, n_robots=R, horizon=H, return_chain=True, sample_fn=ddpm_sample_fn,
                                             guide=None, noise_std_extra_schedule_fn=lambda t: 0.5, n_diffusion_steps_without_noise=1,
                                             warm_start_path_b=xT, step_noise=st).cpu()
    finally:
        model.sampler_flags = 0
    assert res[0].shape == (T + 2, R * B, H, D) and torch.isfinite(res[0]).all()
    for flags in FLAGS:
        assert same_bits(res[0], res[flags]), flags
        assert _hard_rows_exact(res[flags], hc, B), flags


def test_f16_stream_chunks_are_bit_identical():
    """n_streams = 1, 2, 3 with R = 3: each chunk's f16 forwards on a stream of its own, the unsplit call's bits"""
    T, R, B = 25, 3, 8
    model = _model(T)
    paths, hc = _robots(R)
    guide = _guide(paths, R)
    outs = {ns: model.run_inference(None, hc, n_samples=B, n_robots=R, guide=guide, seed=77, n_streams=ns, **GUIDED).cpu() for ns in (1, 2, 3)}
    assert torch.isfinite(outs[1]).all() and _hard_rows_exact(outs[1], hc, B)
    for ns in (2, 3):
        assert same_bits(outs[1], outs[ns]), ns


def test_f16_forward_and_loop_replay_from_a_captured_graph():
    """torch.ops.mmd_amd.unet_forward and .p_sample_loop on an f16 model, eagerly and captured into a graph and replayed, against the
    method calls: the same bits (the f32 form: test_option1_sampling_loop_captures_into_a_hip_graph)."""
    from mmd_amd import ops
    T, R, B = 25, 2, 8
    model = _model(T)
    paths, hc = _robots(R)
    guide = _guide(paths, R)
    hard = torch.stack([hc[0], hc[H - 1]], dim=1).cuda().contiguous()
    tm, tg, tu = ops.register(model), ops.register(guide), ops.register(model.model)
    sg = _lib.signed64(_lib.HARD_ROWS_START_GOAL)
    ref = model.run_inference(None, hc, n_samples=B, n_robots=R, guide=guide, seed=77, **GUIDED)
    x = torch.from_numpy(synth.synth_noise(70, (R * B, H, D))).cuda()
    eps = model.model(x, 7)
    assert torch.isfinite(ref).all() and _hard_rows_exact(ref, hc, B)
    # the ops, eagerly
    xe = torch.empty((R * B, H, D), device="cuda")
    ce = torch.ops.mmd_amd.p_sample_loop(xe, hard, sg, tm, tg, R, T, 1, True, None, 77, 20, 13, 0.5, 0, True)
    assert same_bits(ce, ref) and same_bits(xe, ref[-1])
    assert same_bits(torch.ops.mmd_amd.unet_forward(x, 7, T, tu), eps)
    # captured and replayed
    xg = torch.empty((R * B, H, D), device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eg = torch.ops.mmd_amd.unet_forward(x, 7, T, tu)
        cg = torch.ops.mmd_amd.p_sample_loop(xg, hard, sg, tm, tg, R, T, 1, True, None, 77, 20, 13, 0.5, 0, True)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(eg, eps) and same_bits(cg, ref) and same_bits(xg, ref[-1])
    assert not same_bits(eps, _model(T, "f32").model(x, 7))


# ---- 6. DDIM
def test_f16_ddim_step_algebra_and_chain():
    """ddim_sample (eta = 0) from the same x in both precisions, T = 25: times 24, 19, 14, 9, 4, 0, -1.  The first pair (t = 24,
    t_next = 19) is ddim_update (csrc/guide_dev.h) with make_ddim_step's coefficients (csrc/api.hip): a = sqrt_recip_alphas_cumprod[t],
    b = sqrt_recipm1_alphas_cumprod[t], c1 = sqrtf(alphas_cumprod[t_next]), c2 = sqrtf(1 - alphas_cumprod[t_next]) and

        x' = fma(c1, fma(a, x, -(b eps)), c2 eps)  =  c1 a x + (c2 - c1 b) eps  + rounding,

    affine in eps with NO clamp, so from the same x:  x'_f16 - x'_f32 = (c2 - c1 b)(eps_f16 - eps_f32) + rounding.  Each of the three
    terms c1 a x, c1 b eps, c2 eps passes through at most three fp32 roundings (u = 2^-24 each), so per element and precision the
    rounding is at most 4 u (c1 (a |x| + b |eps|) + c2 |eps|) =: r(eps), and

        |x'_f16 - x'_f32|  <=  |c2 - c1 b| |eps_f16 - eps_f32| + r(eps_f16) + r(eps_f32).

    Pinned rows are the hard conditions exactly, in every chain row; the whole f16 chain is finite."""
    T, R, B = 25, 2, 3
    n = R * B
    _, hc = _robots(R)
    x = torch.from_numpy(synth.synth_noise(72, (n, H, D))) * 0.7
    x[:, 0], x[:, -1] = hc[0].repeat_interleave(B, 0), hc[H - 1].repeat_interleave(B, 0)
    assert GaussianDiffusionModel.ddim_times(T)[:2] == [24, 19]
    t, tn = 24, 19
    tb = O.schedule_tables(T)
    f32 = lambda v: np.float32(float(v))                                                   # noqa: E731
    a, b = float(tb["sqrt_recip_alphas_cumprod"][t]), float(tb["sqrt_recipm1_alphas_cumprod"][t])
    c1 = float(np.sqrt(f32(tb["alphas_cumprod"][tn])))
    c2 = float(np.sqrt(np.float32(1.0) - f32(tb["alphas_cumprod"][tn])))
    k = abs(c2 - c1 * b)
    res = {}
    for prec in ("f32", "f16"):
        m = _model(T, prec)
        eps = m.model(x.cuda(), t).cpu()
        _, chain = m.ddim_sample((n, H, D), hc, T, return_chain=True, n_robots=R, x_init=x.cuda())
        res[prec] = (eps, chain.transpose(0, 1).cpu())
    for prec, (eps, chain) in res.items():
        assert chain.shape == (7, n, H, D) and torch.isfinite(chain).all(), prec
        assert same_bits(chain[0], x) and _hard_rows_exact(chain, hc, B), prec
    u = 2.0 ** -24
    xd = x.double().abs()
    r = sum(4 * u * (c1 * (a * xd + b * res[p][0].double().abs()) + c2 * res[p][0].double().abs()) for p in res)
    d_eps = (res["f16"][0].double() - res["f32"][0].double()).abs()[:, 1:-1]
    d_x = (res["f16"][1][1].double() - res["f32"][1][1].double()).abs()[:, 1:-1]
    slack = d_x - (k * d_eps + r[:, 1:-1])
    print(f"ddim step algebra: |c2 - c1 b| {k:.4f} (a {a:.3f} b {b:.3f} c1 {c1:.4f} c2 {c2:.4f}), max |d eps| {float(d_eps.max()):.3e}, "
          f"max |d x| {float(d_x.max()):.3e}, max rounding term {float(r.max()):.3e}, max slack {float(slack.max()):.3e}")
    assert float(d_eps.max()) > 0 and float(slack.max()) <= 0, float(slack.max())
