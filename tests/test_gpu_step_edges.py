"""-m gpu: the arithmetic that turns a network output into the next x -- ddpm_mean1, ddim_update, ddim_update_x0, add_step_noise and hard_row
(mmd_amd/csrc/guide_dev.h), model_update, step_finish, init_kernel, q_sample_kernel and cross_condition_kernel (guide.hip), fused_ddpm_row
(unet_kernel.h), make_step and make_ddim_step (api.hip) -- at its edges, on the inputs of tests/step_edge_cases.py, against the definition
tests/step_model.py (held to float64 and to the oracle by tests/test_step_edges_host.py).

eps is read back from the model's own mmd_unet_forward at the same (x, t) and the step is compared with the definition fed that eps, row
by row of the chain: the fp32 WORDS must be equal (a NaN wherever the definition has one; a pinned row to the payload of its NaN), and the
distance from the float64 form goes to the parity log next to its bound.  Every family runs through the step kernel (mmd_ddpm_step), the
sampling loop with the step in the UNet launch's tail, with MMD_SAMPLER_NO_FUSED_STEP, with MMD_SAMPLER_PERSIST and in two stream chunks
(asserted to be two); a layered model (its step-kernel launches) and an fp16-precision model (its own fused tail, its persistent run and
its own forward as the source of eps)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, synth                                               # noqa: E402
from mmd_amd.diffusion_model import GaussianDiffusionModel                    # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet                                # noqa: E402
import parity_log                                                             # noqa: E402
import step_edge_cases as E                                                   # noqa: E402
import step_model as M                                                        # noqa: E402

H, D, F32, T = M.H, M.D, np.float32, E.T_STEPS
_MODELS = {}
UNET_KINDS = {"f32": {}, "layered": dict(layered=True), "f16": dict(precision="f16")}
LOOP_PATHS = {"fused": dict(flags=0), "step_kernel": dict(flags=_lib.SAMPLER_NO_FUSED_STEP), "persist": dict(flags=_lib.SAMPLER_PERSIST),
              "two_chunks": dict(flags=0, n_streams=2)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _model(kind="f32", weights="seed0", predict_epsilon=True):
    """a GaussianDiffusionModel of this module's own (its `_tables` are overwritten in place by some tests)"""
    key = (kind, weights, predict_epsilon)
    if key not in _MODELS:
        unet = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=32, dim_mults=(1, 2, 4), **UNET_KINDS[kind])
        unet.load_state_dict(synth.synth_unet_state_dict(0) if weights == "seed0" else E.bias_only_state_dict() if weights == "bias_only"
                             else E.nonfinite_state_dict(float(weights)))
        _MODELS[key] = GaussianDiffusionModel(model=unet, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=predict_epsilon)
    return _MODELS[key]


def _eps(model, x, t):
    return model.model(torch.from_numpy(np.ascontiguousarray(x, F32)).cuda(), int(t)).cpu().numpy()


def _step(model, x, hc, R, i, z=None, seed=None, **kw):
    """mmd_ddpm_step at loop index i"""
    y = torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()
    model.sample_step(y, hc, i, noise_std_extra_schedule_fn=E.noise_extra_fn, n_robots=R, noise=None if z is None else torch.from_numpy(z).cuda(),
                      seed=seed, **kw)
    return y.cpu().numpy()


def _loop(model, x, hc, R, n_steps, n_extra, z=None, flags=0, n_streams=0, seed=5, draw_xT=False):
    """mmd_p_sample_loop from x over the loop indices n_steps - 1 .. -n_extra: the chain [n_steps + n_extra + 1, B, H, D]"""
    model.sampler_flags = flags
    try:
        _, chain = model.p_sample_loop(tuple(x.shape), hc, n_steps, return_chain=True, n_diffusion_steps_without_noise=n_extra,
                                       warm_start_path_b=None if draw_xT else torch.from_numpy(np.ascontiguousarray(x, F32)).cuda(),
                                       noise_std_extra_schedule_fn=E.noise_extra_fn, n_robots=R, seed=seed, n_streams=n_streams,
                                       step_noise=None if z is None else torch.from_numpy(z).cuda())
    finally:
        model.sampler_flags = 0
    return chain.transpose(0, 1).contiguous().cpu().numpy()


def _same(tag, got, want):
    diffs, n = M.first_word_differences(got, want)
    assert n == 0, f"{tag}: {n} words differ from the definition, first (index, kernel, definition): {diffs}"


def _check_chain(tag, model, chain, n_steps, n_extra, z, rows=(), hard=None, spr=1, predicts_x0=False, x=None):
    """every row of a DDPM chain against the definition fed the model's own eps at the row before: the words, and the float64 bound"""
    idx = list(range(n_steps - 1, -n_extra - 1, -1))
    assert chain.shape[0] == len(idx) + 1
    if x is not None:
        _same(f"{tag} chain[0]", chain[0], M.pin(x, rows, hard, spr) if len(rows) else x)
    worst = 0.0
    for k, i in enumerate(idx):
        co = M.ddpm_coeffs(model._tables, i, E.EXTRA_BY_T, predicts_x0)
        eps = _eps(model, chain[k], max(i, 0))
        zk = None if z is None else z[k]
        _same(f"{tag} step {k} (i = {i})", chain[k + 1], M.step32(co, chain[k], eps, zk, rows, hard, spr))
        with np.errstate(all="ignore"):
            y64, bound = M.step64(co, chain[k], eps, zk, rows, hard, spr), M.value_bound(co, chain[k], eps, zk)
            ok = np.isfinite(y64) & np.isfinite(bound) & np.isfinite(chain[k + 1])
            if ok.any():
                worst = max(worst, float((np.abs(chain[k + 1].astype(np.float64) - y64)[ok] / np.maximum(bound[ok], 1e-300)).max()))
    parity_log.record("step_edges", tag, None, worst, bound=1.0, note="worst |kernel - float64| / derived bound over the chain's finite elements")
    print(f"step_edges/{tag}: worst error / bound against float64 {worst:.3f}")
    assert worst <= 1.0, (tag, worst)


def _every_ddpm_path(tag, x, hc, R, n_steps, n_extra, z, rows=(), hard=None, spr=1, weights="seed0", kinds=("f32", "layered", "f16"),
                     predict_epsilon=True, first=None):
    """the family through mmd_ddpm_step and every form of the loop; first(kind, path, x, eps, y): the family's own assertions on the first step"""
    i0 = n_steps - 1 if n_steps else -1
    failed = []

    def attempt(kind, path, fn):                                      # (every path runs: a failure names all the paths it is on)
        try:
            fn()
        except AssertionError as e:
            failed.append(f"{kind}/{path}: {str(e)[:300]}")

    for kind in kinds:
        model = _model(kind, weights, predict_epsilon)
        co = M.ddpm_coeffs(model._tables, i0, E.EXTRA_BY_T, not predict_epsilon)
        x0 = M.pin(x, rows, hard, spr) if len(rows) else x
        eps = _eps(model, x0, max(i0, 0))

        def one_step():
            y = _step(model, x0, hc, R, i0, None if z is None else z[0])
            _same(f"{tag}/{kind}/mmd_ddpm_step", y, M.step32(co, x0, eps, None if z is None else z[0], rows, hard, spr))
            if first:
                first(kind, "mmd_ddpm_step", x0, eps, y)

        def loop(path, kw):
            chain = _loop(model, x, hc, R, n_steps, n_extra, z, **kw)
            if first:
                first(kind, path, chain[0], eps, chain[1])
            _check_chain(f"{tag}/{kind}/{path}", model, chain, n_steps, n_extra, z, rows, hard, spr, not predict_epsilon, x)

        if kind == "f32":
            attempt(kind, "mmd_ddpm_step", one_step)
        # the layered model has no fused tail (unet_fused_step_supported is false): every form of its loop is the same step-kernel launch,
        # run once; the f16 model: its tail and its persistent run (the chunked loop is the f32 one's on other streams)
        paths = {"f32": tuple(LOOP_PATHS), "layered": ("step_kernel",), "f16": ("fused", "persist")}[kind]
        for path in paths:
            kw = LOOP_PATHS[path]
            if path == "two_chunks":                                  # (the chunk count is capped at the robots: the split must be real)
                assert _lib.load().mmd_sampler_stream_chunks(2, R, len(x) // R) == 2, (tag, R)
            attempt(kind, path, lambda: loop(path, kw))
    assert not failed, f"{tag}: {len(failed)} path(s) fail:\n" + "\n".join(failed)


def _noise(n, B):
    """step noise [n, B, H, D] with the planted values (step_edge_cases.noise_input) in every row"""
    z = np.stack([np.roll(E.noise_input(B), k, axis=1) for k in range(n)])
    return np.ascontiguousarray(z, F32)


# ---- 1. the clamp to the ulp
def test_clamp_ladder_on_every_path():
    """a = 1, b = 0, c1 = 1, c2 = 0: the step returns clamp(x) -- +-1 +- {0, 1, 2} ulp, +-0 and denormals as they are, beyond the bounds
    the bound; rows with +-FLT_MAX or +-inf have a non-finite eps (0 * inf = NaN, as torch has it) and the finite rows do not see them.
    One robot per trajectory, so that two stream chunks are two."""
    x = E.clamp_ladder()
    want = np.clip(x[:E.N_FINITE], -1, 1)

    def first(kind, path, x0, eps, y):
        assert np.isfinite(eps[:E.N_FINITE]).all() and not np.isfinite(eps[E.ROW_HUGE:]).all(axis=(1, 2)).any(), (kind, path)
        # (as values: -0 comes back as +0 where eps < 0 -- fma(1, -0, -(0 eps)) = -0 + +0 -- which the definition's words, checked by the caller, have)
        assert np.array_equal(y[:E.N_FINITE], want), (kind, path, M.first_word_differences(y[:E.N_FINITE], want))
        assert np.array_equal(y[:E.N_FINITE][want != 0].view(np.int32), want[want != 0].view(np.int32)), (kind, path)

    for kind in UNET_KINDS:
        model = _model(kind)
        with E.tables_set(model, **E.identity_tables()):
            clean = x.copy()
            clean[E.ROW_HUGE:] = 0.0
            e_all, e_clean = _eps(model, x, 0), _eps(model, clean, 0)
            assert np.array_equal(e_all[:E.N_FINITE].view(np.int32), e_clean[:E.N_FINITE].view(np.int32)), kind
            _every_ddpm_path("clamp_ladder", x, {}, len(x), 1, 2, None, kinds=(kind,), first=first)


# ---- 2. the clamp with the real schedule and network
@pytest.mark.parametrize("t", E.REAL_T)
def test_clamp_with_the_real_schedule_and_eps(t):
    """t = 0, 1, T - 1 of the exponential schedule, x scaled so that a x - b eps lies on both sides of both bounds: at least 32 elements at
    each bound and, at t = 0 and 1, 32 inside, counted from the device's own eps.  At t = T - 1 (a = b = 4.6e3) the inside of the clamp is
    |x - eps(x)| < 2.2e-4, which scaling x does not reach (step_edge_cases.real_eps_input): there the inside is held by
    test_clamp_inside_and_at_both_bounds_with_the_last_step_s_coefficients.  One robot per trajectory, so that two stream chunks are two."""
    x = E.real_eps_input(t)

    def first(kind, path, x0, eps, y):
        co = M.ddpm_coeffs(_model(kind)._tables, t, E.EXTRA_BY_T)
        lo, mid, hi = E.clamp_counts(x0, eps, co.a, co.b)
        print(f"clamp_real t = {t} {kind}/{path}: {lo} at -1, {mid} inside, {hi} at +1")
        assert lo >= 32 and hi >= 32 and (mid >= 32 or t == T - 1), (t, lo, mid, hi)          # (t = T - 1: step_edge_cases.real_eps_input)

    _every_ddpm_path(f"clamp_real_t{t}", x, {}, len(x), t + 1, 1, _noise(t + 2, len(x)), first=first)


def test_clamp_inside_and_at_both_bounds_with_the_last_step_s_coefficients():
    """t = T - 1 with a network whose final weights are zero (eps = its final bias, read back as everywhere): a x - b eps uniform in +-1.5"""
    x = E.constant_eps_input()

    def first(kind, path, x0, eps, y):
        co = M.ddpm_coeffs(_model(kind, "bias_only")._tables, T - 1, E.EXTRA_BY_T)
        lo, mid, hi = E.clamp_counts(x0, eps, co.a, co.b)
        print(f"clamp_constant_eps {kind}/{path}: {lo} at -1, {mid} inside, {hi} at +1")
        assert min(lo, mid, hi) >= 32, (lo, mid, hi)

    _every_ddpm_path("clamp_constant_eps", x, {}, len(x), T, 0, _noise(T, len(x)), weights="bias_only", first=first)


# ---- 3. a network output that is not finite
@pytest.mark.parametrize("value", ["nan", "inf"])
def test_non_finite_eps_keeps_what_torch_keeps(value):
    """final_conv.1.bias[0] = NaN / +inf: channel 0 of eps is that, channels 1 .. 3 are finite.  A NaN stays NaN in channel 0 of every row that
    is not pinned (x_recon.clamp_ keeps it); +inf clamps to the bound torch gives (x0 = -inf -> -1); channels 1 .. 3 and the pinned rows are
    the definition's words."""
    rows, spr, R = (0, 17, 40, 63), 2, E.N_ROBOTS
    hard = E.hard_values(rows, nan=False)
    hc = E.hard_conds(rows, hard)
    x = E.step_input(R * spr)
    free = np.asarray([t for t in range(H) if t not in rows])

    def first(kind, path, x0, eps, y):
        bad = np.isnan(eps[..., 0]) if value == "nan" else np.isposinf(eps[..., 0])
        assert bad.all() and np.isfinite(eps[..., 1:]).all(), (kind, path, "the weights do not give the eps this case is about")
        if value == "nan":
            assert np.isnan(y[:, free, 0]).all(), (kind, path, f"{int((~np.isnan(y[:, free, 0])).sum())} NaN outputs became finite samples")
        else:                                                        # (x0 = -inf -> -1: the words are the definition's, checked by the caller)
            assert np.isfinite(y[:, free, 0]).all(), (kind, path)
        assert np.isfinite(y[:, free, 1:]).all(), (kind, path)
        for t, slot in M.slots_of(rows).items():
            assert np.array_equal(y[:, t].view(np.int32), np.repeat(hard[:, slot], spr, axis=0).view(np.int32)), (kind, path, t)

    _every_ddpm_path(f"eps_{value}", x, hc, R, 3, 2, _noise(5, len(x)), rows, hard, spr, weights=value, first=first)


# ---- 4. noise
def test_noise_planted_values_and_the_table_of_t_on_every_path():
    """z with +-0, +-1e30 and denormals, noise_std_extra distinct per t, the whole T = 25 loop and its two steps at i < 0; pinned {1, 62}"""
    rows, spr, R = (1, 62), 2, E.N_ROBOTS
    hard = E.hard_values(rows, nan=False)
    x = E.step_input(R * spr)
    _every_ddpm_path("noise", x, E.hard_conds(rows, hard), R, T, 2, _noise(T + 2, len(x)), rows, hard, spr)


def test_steps_at_and_below_zero_ignore_noise_tensor_and_draw_index():
    """i = 0, -1, -2 (t = 0): the same bits whatever the noise tensor holds, whichever seed and draw index the in-kernel generator would use"""
    R, spr = E.N_ROBOTS, 2
    x = E.step_input(R * spr)
    model = _model()
    z = _noise(3, len(x))
    ref = _loop(model, x, {}, R, 1, 2, z)
    for path, kw in LOOP_PATHS.items():
        for name, zz, seed in (("nan_noise", np.full_like(z, np.nan), 5), ("seed_1", None, 1), ("seed_2", None, 2)):
            _same(f"t0/{path}/{name}", _loop(model, x, {}, R, 1, 2, zz, seed=seed, **kw), ref)
    ys = [_step(model, x, {}, R, i, zz, seed=seed) for i in (0, -1, -2) for zz, seed in ((z[0], 1), (None, 7), (np.full_like(z[0], np.inf), 3))]
    for y in ys:
        _same("t0/mmd_ddpm_step", y, ref[1])


# ---- 5. the pinned rows
@pytest.mark.parametrize("spr", E.SPRS)
@pytest.mark.parametrize("rows", E.MASKS, ids=E.MASK_IDS)
def test_pinned_row_masks_per_robot_values(rows, spr):
    """every mask x 3 robots with distinct values per robot and slot (-0 among them; a NaN payload at 8 samples a robot, whose robot 1 is
    then NaN outside its pinned rows) x samples_per_robot 1, 6 (a four-wave workgroup spans robots) and 8: the step kernel, every form of
    the loop, init_kernel's chain[0] with and without drawing x_T"""
    R = E.N_ROBOTS
    hard = E.hard_values(rows, nan=spr == 8)
    hc = E.hard_conds(rows, hard)
    x = E.step_input(R * spr)
    z = _noise(3, len(x))
    model = _model()
    _every_ddpm_path(f"mask_{E.MASK_IDS[E.MASKS.index(rows)]}_spr{spr}", x, hc, R, 2, 1, z, rows, hard, spr)
    want = np.repeat(hard, spr, axis=0)
    drawn, plain = _loop(model, x, hc, R, 1, 0, seed=11, draw_xT=True), _loop(model, x, {}, R, 1, 0, seed=11, draw_xT=True)
    slots = M.slots_of(rows)
    for t in range(H):
        if t in slots:
            assert np.array_equal(drawn[0][:, t].view(np.int32), want[:, slots[t]].view(np.int32)), (rows, spr, t)
        else:
            assert np.array_equal(drawn[0][:, t], plain[0][:, t]) and np.isfinite(drawn[0][:, t]).all(), (rows, spr, t)
    if len(rows) == H:
        assert np.array_equal(drawn[-1].view(np.int32), want.view(np.int32))


# ---- 6. the x0-predicting model and DDIM
def test_ddpm_step_of_the_x0_predicting_model():
    """predict_epsilon = False: a = 0, b = -1 -- x0 is the clamped network output itself"""
    rows, spr, R = (0, 63), 2, E.N_ROBOTS
    hard = E.hard_values(rows, nan=False)
    x = E.step_input(R * spr) * 3.0
    _every_ddpm_path("ddpm_x0_model", x, E.hard_conds(rows, hard), R, 3, 2, _noise(5, len(x)), rows, hard, spr, predict_epsilon=False)


def _ddim(model, x, hc, R, times, guide=None):
    """mmd_ddim_sample over `times`: the chain [len(times), B, H, D] (rows behind a pair that ends in -1 are not written)"""
    y = torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()
    hard, mask = model._hard_tensor(hc, R, H, y.device, D)
    s = model._sampler_desc(1, float("inf"), None, mask)
    tm = np.asarray(times, np.int32)
    acp = np.ascontiguousarray(model._tables["alphas_cumprod"], F32)
    chain = torch.zeros((len(times),) + tuple(y.shape), device="cuda")
    ws = model.model.workspace(len(x), y.device, sampler=True)
    _lib.launch("mmd_ddim_sample", y, model.model.handle(T, y.device), C.byref(s), acp.ctypes.data, tm.ctypes.data, len(tm), None, y.data_ptr(),
                hard.data_ptr(), R, len(x) // R, 0, C.c_uint64(0), chain.data_ptr(), ws.data_ptr(), ws.numel())
    return chain.cpu().numpy(), y.cpu().numpy()


@pytest.mark.parametrize("predict_epsilon", [True, False], ids=["eps_model", "x0_model"])
@pytest.mark.parametrize("times", [(24, 19, 14, 9, 4, 0, -1), (20, 7, -1), (12, 3), (1, 0, -1)], ids=["reference_times", "ends_in_-1", "two_times", "low"])
def test_ddim_pairs_and_the_last_pair(times, predict_epsilon):
    """every pair of a times list, the last pair (t_next = -1: c1 = 1, c2 = 0, the x0 model's 1 / b = 0) included, pinned {31, 32}"""
    rows, spr, R = (31, 32), 2, E.N_ROBOTS
    hard = E.hard_values(rows, nan=False)
    x = E.step_input(R * spr) * (1.0 if predict_epsilon else 0.05)
    for kind in ("f32", "layered", "f16"):
        model = _model(kind, predict_epsilon=predict_epsilon)
        chain, y = _ddim(model, x, E.hard_conds(rows, hard), R, times)
        _same(f"ddim/{kind} chain[0]", chain[0], M.pin(x, rows, hard, spr))
        worst = 0.0
        for k, (t, tn) in enumerate(zip(times[:-1], times[1:])):
            co = M.ddim_coeffs(model._tables, t, tn, not predict_epsilon)
            eps = _eps(model, chain[k], t)
            _same(f"ddim/{kind} pair ({t}, {tn})", chain[k + 1], M.step32(co, chain[k], eps, None, rows, hard, spr))
            err = np.abs(chain[k + 1].astype(np.float64) - M.step64(co, chain[k], eps, None, rows, hard, spr))
            worst = max(worst, float((err / np.maximum(M.value_bound(co, chain[k], eps, None), 1e-300)).max()))
        parity_log.record("step_edges", f"ddim/{kind}/{'eps' if predict_epsilon else 'x0'}/{times}", None, worst, bound=1.0)
        assert worst <= 1.0 and np.array_equal(y.view(np.int32), chain[-1].view(np.int32)), (kind, worst)


# ---- 7. the guided launch shapes
def _guide(R, binned=False):
    import gpu_common as gc
    import guide_edge_cases as G
    from mmd_amd.constraints import binned_constraints_from_paths
    if binned:
        from mmd_amd.guides import GuideManagerTrajectoriesWithVelocity
        g = GuideManagerTrajectoriesWithVelocity(gc.dataset(), env_id="EnvEmpty2D", n_robots=R, device="cuda")
        g.set_binned_constraints(binned_constraints_from_paths(torch.full((R, H, 2), 50.0, device="cuda"), 0, R, radius=float(G.R), weight=1.0))
        return g
    return gc.hip_guide("EnvEmpty2D", [[G.far_group()] for _ in range(R)], n_robots=R)


@pytest.mark.parametrize("rows", E.MASKS, ids=E.MASK_IDS)
def test_guided_launch_shapes_pin_the_same_rows_and_return_the_same_bits(rows):
    """one guided step (two guide iterations, guide_edge_cases.far_group: 41 slots that never act) as the cooperative kernel, the eight-wave
    kernel (guide_coop_max = -1, 8 samples a robot), the four-wave kernel (6 samples a robot: a workgroup spans robots) and the binned
    kernel: the same bits per (robot, sample), the pinned rows the hard words, also in every row of mmd_guide_steps' chain"""
    R = E.N_ROBOTS
    hard = E.hard_values(rows, nan=False)
    hc = E.hard_conds(rows, hard)
    model = _model()
    x8, z8 = E.step_input(R * 8).reshape(R, 8, H, D), E.noise_input(R * 8).reshape(R, 8, H, D)
    kw = dict(n_guide_steps=2, t_start_guide=10)
    out = {}
    try:
        for name, spr, coop, binned in (("coop", 8, 0, False), ("eight_wave", 8, -1, False), ("four_wave", 6, -1, False), ("binned", 8, 0, True)):
            model.guide_coop_max = coop
            xs, zs = (np.ascontiguousarray(v[:, :spr].reshape(R * spr, H, D)) for v in (x8, z8))
            out[name] = _step(model, xs, hc, R, 3, zs, guide=_guide(R, binned), **kw).reshape(R, spr, H, D)
    finally:
        model.guide_coop_max = 0
    slots = M.slots_of(rows)
    for name, y in out.items():
        _same(f"guided/{name}", y[:, :6], out["coop"][:, :6])
        for t, slot in slots.items():
            assert np.array_equal(y[:, :, t].view(np.int32), np.broadcast_to(hard[:, None, slot], y[:, :, t].shape).view(np.int32)), (name, t)
        free = [t for t in range(H) if t not in slots]
        assert np.isfinite(y[:, :, free]).all(), name
    # a guide-only launch with its chain
    xs = torch.from_numpy(np.ascontiguousarray(x8.reshape(R * 8, H, D))).cuda()
    hd, mask = model._hard_tensor(hc, R, H, xs.device, D)
    gd = _guide(R).desc()
    chain = torch.zeros((3,) + tuple(xs.shape), device="cuda")
    _lib.check(_lib.load().mmd_guide_steps(C.byref(gd), xs.data_ptr(), hd.data_ptr(), C.c_uint64(mask), R, 8, 3, chain.data_ptr(), _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    ch = chain.cpu().numpy().reshape(3, R, 8, H, D)
    assert np.array_equal(ch[-1].view(np.int32), xs.cpu().numpy().reshape(R, 8, H, D).view(np.int32))
    for t, slot in slots.items():
        assert np.array_equal(ch[:, :, :, t].view(np.int32), np.broadcast_to(hard[None, :, None, slot], ch[:, :, :, t].shape).view(np.int32)), t
    if len(rows) == H:
        want = np.broadcast_to(hard[:, None], (R, 8, H, D))
        assert np.array_equal(out["coop"].view(np.int32), want.view(np.int32)) and np.array_equal(ch[0].view(np.int32), want.view(np.int32))


# ---- 8. cross conditioning
@pytest.mark.parametrize("name", list(E.CROSS_RELS))
def test_cross_condition_at_the_boundary_and_with_non_finite_stitch_rows(name):
    """v2 + rel at boundary +- {0, 1, 2} ulp, a zero component (boundary 1e6), the reversed direction, ind1 / ind2 in {0, 63}, NaN and +-inf in
    the stitch row (NaN stays NaN in both tiles, as torch.min / torch.max have it), n_traj = 1, 255, 256, 257"""
    lib = _lib.load()
    for ind1, ind2 in ((63, 0), (0, 63), (0, 0), (63, 63)):
        x1, x2, rel, bnd = E.cross_input(E.CROSS_RELS[name], ind1, ind2)
        for n in E.CROSS_N:
            a, b = torch.from_numpy(x1[:n].copy()).cuda(), torch.from_numpy(x2[:n].copy()).cuda()
            _lib.check(lib.mmd_cross_condition(a.data_ptr(), b.data_ptr(), ind1, ind2, rel.ctypes.data_as(C.POINTER(C.c_float)),
                                               bnd.ctypes.data_as(C.POINTER(C.c_float)), n, _lib.current_stream_ptr()))
            torch.cuda.synchronize()
            w1, w2 = M.cross_condition(x1[:n], x2[:n], ind1, ind2, rel, bnd)
            _same(f"cross/{name}/{ind1}-{ind2}/n{n} tile 1", a.cpu().numpy(), w1)
            _same(f"cross/{name}/{ind1}-{ind2}/n{n} tile 2", b.cpu().numpy(), w2)
            if n >= 16:
                assert np.isnan(a.cpu().numpy()[:, ind1]).any() and np.isnan(b.cpu().numpy()[:, ind2]).any()


@pytest.mark.parametrize("spr", [3, 128])
def test_cross_condition_by_robot_table_and_chain_rows(spr):
    """mmd_p_sample_loop_ensemble with no steps: init_kernel, then the stitching of the pair with a per-robot table (two robots, different
    offsets); the tiles' chain rows 0 are the stitched x1 and x2"""
    model = _model()
    n = 2 * spr
    x1, x2, _, _ = E.cross_input(E.CROSS_RELS["fwd"], 63, 0, n=n)
    tab = E.by_robot_table()
    tab_dev = torch.from_numpy(tab).cuda()
    xs = [torch.from_numpy(v.copy()).cuda() for v in (x1, x2)]
    chains = [torch.zeros((1, n, H, D), device="cuda") for _ in range(2)]
    hard = torch.zeros(2, 1, D, device="cuda")
    s = model._sampler_desc(1, float("inf"), None, 0)
    tiles = (_lib.EnsembleTile * 2)()
    for m in range(2):
        tiles[m].unet, tiles[m].sampler, tiles[m].guide = model.model.handle(T, "cuda").value, C.pointer(s), None
        tiles[m].x_dev, tiles[m].hard_dev, tiles[m].step_noise_dev, tiles[m].chain_dev, tiles[m].seed = xs[m].data_ptr(), hard.data_ptr(), None, chains[m].data_ptr(), 0
    cc = _lib.CrossCond(0, 1, 63, 0, (C.c_float * 4)(9, 9, 9, 9), (C.c_float * 4)(9, 9, 9, 9), tab_dev.data_ptr())      # (the table overrides rel / boundary)
    ws = model.model.workspace(n, "cuda", sampler=True)
    _lib.check(_lib.load().mmd_p_sample_loop_ensemble(tiles, 2, C.byref(cc), 1, 2, spr, 0, 0, 0, ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    w1, w2 = M.cross_condition(x1, x2, 63, 0, None, None, by_robot=tab, spr=spr)
    for m, w in enumerate((w1, w2)):
        _same(f"cross/by_robot/spr{spr} tile {m}", xs[m].cpu().numpy(), w)
        _same(f"cross/by_robot/spr{spr} chain row of tile {m}", chains[m][0].cpu().numpy(), w)


# ---- 9. q_sample
@pytest.mark.parametrize("n", E.Q_N)
def test_q_sample_within_three_roundings_of_float64(n):
    model = _model()
    x0, z = E.q_input(n)
    for t in (0, 12, T - 1):
        y = model.q_sample(torch.from_numpy(x0).cuda(), t, noise=torch.from_numpy(z).cuda()).cpu().numpy()
        a, b = F32(float(model.sqrt_alphas_cumprod[t])), F32(float(model.sqrt_one_minus_alphas_cumprod[t]))
        err, bound = np.abs(y - M.q_sample64(x0, z, a, b)), M.q_sample_bound(x0, z, a, b)
        parity_log.record("step_edges", f"q_sample/n{n}/t{t}", None, float((err / np.maximum(bound, 1e-300)).max()), bound=1.0)
        assert np.all(err <= bound), (n, t, float(err.max()))


# ---- 10. calls the entry points refuse
def test_refused_calls_stay_refused():
    lib, model = _lib.load(), _model()
    a = torch.zeros(2, H, D, device="cuda")
    rel = (C.c_float * 4)(1, 0, 0, 0)
    for ind1, ind2 in ((64, 0), (0, 64), (-1, 0)):
        assert lib.mmd_cross_condition(a.data_ptr(), a.data_ptr(), ind1, ind2, rel, rel, 2, _lib.current_stream_ptr()) != 0
        assert "row index out of range" in lib.mmd_last_error().decode()
    x = E.step_input(2)
    with pytest.raises(RuntimeError, match="fewer than two times"):
        _ddim(model, x, {}, 1, (5,))
    for times in ((5, 5), (3, 7), (5, 2, 2)):
        with pytest.raises(RuntimeError, match="times must decrease"):
            _ddim(model, x, {}, 1, times)
    with pytest.raises(RuntimeError, match="times must decrease"):
        _ddim(model, x, {}, 1, (T, 3))
    with pytest.raises(ValueError, match="outside"):
        model._hard_tensor({64: torch.zeros(4)}, 1, H, "cuda", D)
