"""No GPU: the step definition (tests/step_model.py) against its float64 form and against the oracle, and the inputs of
tests/step_edge_cases.py against the edges they are meant to reach -- so that tests/test_gpu_step_edges.py can hold the kernels to the
definition bit for bit.

The oracle evaluates a x - b eps with three fp32 roundings and c1 x0 + c2 x with three more where the kernels use two each: it is held to
the same float64 form by the same formula with its own operation count (step_model.value_bound(extra_roundings=...)), not to the bits.  The
clamp is continuous, so no decision moves a result by more than the rounding."""
import numpy as np
import pytest
import torch

import step_edge_cases as E
import step_model as M
from oracle import mmd_oracle as O

H, D, F32 = M.H, M.D, np.float32
# the oracle's DDPM step: a x | b eps | - | c1 x0 | c2 x | + | exp (1 ulp) | std z | . extra | +  = 10 fp32 operations, 4 + 2 of them counted already
ORACLE_EXTRA = 4


def _tb(tables):
    return {k: torch.from_numpy(np.asarray(v, F32)) for k, v in tables.items()}


def test_fma_is_the_single_rounding_fma_also_at_the_ends_of_the_range():
    a = np.asarray([1.0, E.FLT_MAX, E.FLT_MAX, np.inf, 1e-30, 1.0 + 2.0 ** -23, np.nan, 0.0], F32)
    b = np.asarray([1.0, 2.0, 1.0, 0.0, 1e-30, 1.0 + 2.0 ** -23, 1.0, np.inf], F32)
    c = np.asarray([-0.0, -E.FLT_MAX, 0.0, 1.0, 0.0, -1.0, 1.0, 1.0], F32)
    got = M.fma_f32(a, b, c)
    want = np.asarray([1.0, E.FLT_MAX, E.FLT_MAX, np.nan, 1e-60, 2.0 ** -22 + 2.0 ** -46, np.nan, np.nan], np.float64).astype(F32)
    assert M.same_words(got, want), (got, want)
    # a tie of the product is broken by an addend far below half an ulp of it (a noise term of 1e30 next to a state of 1)
    p = np.nextafter(F32(2.0 ** 100), F32(np.inf))                   # odd last bit: 1.5 p lies half way between two fp32 values
    assert float(M.fma_f32(p, F32(1.5), F32(1.0))) == 1.5 * 2.0 ** 100 + 2.0 ** 78 and float(M.fma_f32(p, F32(1.5), F32(-1.0))) == 1.5 * 2.0 ** 100 + 2.0 ** 77
    assert M.fma_f32(F32(1), F32(-0.0), F32(0.0)).view(np.int32) == 0 and M.fma_f32(F32(1), F32(-0.0), F32(-0.0)).view(np.uint32) == 0x80000000


def test_expf32_is_libm_and_exact_where_it_can_be():
    assert M.expf32(0.0) == 1 and abs(float(M.expf32(-0.5)) - np.exp(-0.5)) < 2.0 ** -24
    tb = E.real_tables()
    for t in range(E.T_STEPS):
        lv = F32(0.5) * tb["posterior_log_variance_clipped"][t]
        assert abs(float(M.expf32(lv)) - np.exp(float(lv))) <= 2.0 ** -23 * np.exp(float(lv))


@pytest.mark.parametrize("predicts_x0", [False, True], ids=["eps_model", "x0_model"])
def test_ddpm_definition_within_the_bound_of_float64_and_of_the_oracle(predicts_x0):
    tb, sd = E.real_tables(), E.oracle_state_dict()
    for i in (E.T_STEPS - 1, 7, 1, 0, -1, -2):
        t = max(i, 0)
        x = E.real_eps_input(t) if t in E.REAL_T else E.step_input(E.N_REAL)
        z = E.noise_input(len(x))
        z[np.abs(z) > 1e20] = 3.0                                    # (finite products for the oracle's three-operation noise term)
        eps = E.oracle_eps(x, t)
        co = M.ddpm_coeffs(tb, i, E.EXTRA_BY_T, predicts_x0)
        assert co.do_noise == (t != 0)
        y32, y64 = M.step32(co, x, eps, z), M.step64(co, x, eps, z)
        err = np.abs(y32.astype(np.float64) - y64)
        assert np.all(err <= M.value_bound(co, x, eps, z)), (i, float(err.max()))
        ref = O.ddpm_sample_step(sd, _tb(tb), torch.from_numpy(x.copy()), {}, i, noise=torch.from_numpy(z), noise_std_extra=float(E.EXTRA_BY_T[t]),
                                 predict_epsilon=not predicts_x0).numpy()
        err_o = np.abs(ref.astype(np.float64) - y64)
        assert np.all(err_o <= M.value_bound(co, x, eps, z, extra_roundings=ORACLE_EXTRA)), (i, float(err_o.max()))
        if t == 0:                                                    # no noise at t = 0, whatever z holds
            assert M.same_words(y32, M.step32(co, x, eps, np.full_like(z, np.nan)))
        if not predicts_x0 and t in E.REAL_T:
            lo, mid, hi = E.clamp_counts(x, eps, co.a, co.b)
            # (the GPU test asserts >= 32 from the device's own eps; the inside at t = T - 1: step_edge_cases.real_eps_input)
            assert min(lo, hi) >= 64 and (mid >= 64 or t == E.T_STEPS - 1), (t, lo, mid, hi)


@pytest.mark.parametrize("predicts_x0", [False, True], ids=["eps_model", "x0_model"])
def test_ddim_definition_within_the_bound_of_float64_and_of_the_oracle_chain(predicts_x0):
    """every pair of the T = 25 times (24, 19, 14, 9, 4, 0, -1), the last pair included: each step from the oracle chain's own row"""
    tb, sd = E.real_tables(), E.oracle_state_dict()
    times = O.ddim_times(E.T_STEPS)
    assert times[-1] == -1 and times[-2] == 0
    x = E.step_input(4) * (0.05 if predicts_x0 else 1.0)              # (the x0 model divides by b: small at the low times)
    chain = O.ddim_sample(sd, _tb(tb), torch.from_numpy(x), {}, E.T_STEPS, predict_epsilon=not predicts_x0).numpy()
    assert chain.shape[0] == len(times)
    for k, (t, tn) in enumerate(zip(times[:-1], times[1:])):
        co = M.ddim_coeffs(tb, t, tn, predicts_x0)
        if tn < 0:
            assert co.c1 == 1 and co.c2 == 0 and (not predicts_x0 or co.b == 0)
        eps = E.oracle_eps(chain[k], t)
        y32, y64 = M.step32(co, chain[k], eps, None), M.step64(co, chain[k], eps, None)
        err = np.abs(y32.astype(np.float64) - y64)
        assert np.all(err <= M.value_bound(co, chain[k], eps, None)), (t, tn, float(err.max()))
        # the oracle: a x | b e | - | . sqrt(an) | c e | +, the x0 model a x | - | / b | c . | o sqrt(an) | +; sqrt(an), c rounded in fp32 as here
        err_o = np.abs(chain[k + 1].astype(np.float64) - y64)
        assert np.all(err_o <= M.value_bound(co, chain[k], eps, None, extra_roundings=3)), (t, tn, float(err_o.max()))
    if not predicts_x0:                                               # the last pair returns x_start itself: c2 of the pair before must not act
        co_prev = M.ddim_coeffs(tb, times[-3], times[-2])
        assert not M.same_words(M.step32(co, chain[-2], eps, None), M.step32(co._replace(c2=co_prev.c2), chain[-2], eps, None))


def test_clamp_ladder_reaches_both_sides_of_both_bounds_to_the_ulp():
    x = E.clamp_ladder()
    fin = x[:E.N_FINITE]
    assert np.isfinite(fin).all() and min(E.sides_of_unit(E.LADDER)) >= 1 and min(E.sides_of_unit(fin)) >= 64
    for s in (1.0, -1.0):
        for k in (-2, -1, 0, 1, 2):
            assert (fin == E.ulps(s, k)).sum() >= 16, (s, k)
    assert np.signbit(fin[fin == 0]).any() and not np.signbit(fin[fin == 0]).all()
    assert ((fin != 0) & (np.abs(fin) < np.finfo(F32).tiny)).sum() >= 64              # denormals
    assert (np.abs(x[E.ROW_HUGE]) == E.FLT_MAX).sum() == H * D // 2
    assert np.isposinf(x[E.ROW_PINF]).sum() == 4 and np.isneginf(x[E.ROW_NINF]).sum() == 4 and np.isfinite(x[:E.ROW_PINF]).all()
    # with the identity tables the step IS the clamp, zero signs included: fma(1, x, -(0 e)) and fma(1, x0, 0 x)
    co = M.Coeffs("ddpm", F32(1), F32(0), F32(1), F32(0), F32(1), F32(1), False)
    y = M.step32(co, fin, np.full_like(fin, 0.25), None)
    want = np.clip(fin, -1, 1)
    assert np.array_equal(y, want) and np.array_equal(y[np.abs(fin) < 1][fin[np.abs(fin) < 1] != 0], fin[(np.abs(fin) < 1) & (fin != 0)])
    # a non-finite eps under b = 0 is 0 * inf = NaN: such a row is NaN everywhere, as torch has it
    assert np.isnan(M.step32(co, fin, np.full_like(fin, np.inf), None)).all()


def test_constant_eps_input_reaches_the_inside_of_the_clamp_at_the_last_step():
    tb = E.real_tables()
    t = E.T_STEPS - 1
    x = E.constant_eps_input()
    sd = E.bias_only_state_dict()
    assert not sd["final_conv.1.weight"].any() and np.isfinite(sd["final_conv.1.bias"]).all()
    eps = np.broadcast_to(sd["final_conv.1.bias"].astype(F32), x.shape)
    lo, mid, hi = E.clamp_counts(x, eps, tb["sqrt_recip_alphas_cumprod"][t], tb["sqrt_recipm1_alphas_cumprod"][t])
    assert min(lo, mid, hi) >= 256, (lo, mid, hi)
    o = O.unet_forward(O.state_dict_to_torch(sd), torch.from_numpy(x[:2]), torch.full((2,), t, dtype=torch.long)).numpy()
    assert np.array_equal(o, eps[:2])                                # the oracle's eps IS the bias


def test_nan_semantics_of_the_reference_on_the_installed_torch():
    """x_recon.clamp_(-1., 1.), torch.min and torch.max propagate a NaN -- and so does the definition; +-inf clamps to the bound"""
    v = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.5])
    c = v.clone().clamp_(-1.0, 1.0)
    assert torch.isnan(c[0]) and c[1:].tolist() == [1.0, -1.0, 0.5]
    assert M.same_words(M.clamp_unit(v.numpy()), c.numpy())
    b = torch.tensor([1.0, 1.0, 1.0, 1.0])
    assert torch.isnan(torch.min(v, b)[0]) and torch.isnan(torch.max(v, -b)[0]) and torch.isnan(torch.min(b, v)[0])
    co = M.Coeffs("ddpm", F32(1.5), F32(0.5), F32(0.75), F32(0.25), F32(1), F32(1), False)
    x = np.full((1, H, D), 0.5, F32)
    e = np.zeros((1, H, D), F32)
    e[0, :, 0], e[0, :, 1], e[0, :, 2] = np.nan, np.inf, -np.inf
    y = M.step32(co, x, e, None)
    ref = 0.75 * (1.5 * torch.from_numpy(x) - 0.5 * torch.from_numpy(e)).clamp_(-1.0, 1.0) + 0.25 * torch.from_numpy(x)
    assert np.isnan(y[..., 0]).all() and M.same_words(y, ref.numpy())
    assert np.all(y[..., 1] == F32(-0.625)) and np.all(y[..., 2] == F32(0.875))
    # the stitching: a NaN stitch row is NaN in both tiles
    x1, x2, rel, bnd = E.cross_input(E.CROSS_RELS["fwd"], 63, 0, n=32)
    y1, y2 = M.cross_condition(x1, x2, 63, 0, rel, bnd)
    nan_in = np.isnan(x2[:, 0])
    assert nan_in.sum() >= 2 and np.array_equal(np.isnan(y1[:, 63]), nan_in) and np.array_equal(np.isnan(y2[:, 0]), nan_in)


@pytest.mark.parametrize("rows", E.MASKS, ids=E.MASK_IDS)
def test_slot_table_is_the_sorted_rows_and_pinning_matches_the_oracle(rows):
    slots = M.slots_of(rows)
    assert slots == {t: k for k, t in enumerate(sorted(rows))} and bin(M.mask_of(rows)).count("1") == len(rows)
    hard = E.hard_values(rows)
    assert len(np.unique(hard[~np.isnan(hard)])) == (~np.isnan(hard)).sum()                          # a distinct value per (robot, slot, dim)
    hc = E.hard_conds(rows, hard)
    assert sorted(hc) == sorted(rows)
    for spr in E.SPRS:
        B = E.N_ROBOTS * spr
        x = E.step_input(B)
        got = M.pin(x, rows, hard, spr)
        ref = O.apply_hard_conditioning(torch.from_numpy(x.copy()), {t: v.repeat_interleave(spr, 0) for t, v in hc.items()}).numpy()
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (rows, spr)
        if len(rows) == H:
            assert np.array_equal(got.view(np.int32), np.repeat(hard, spr, axis=0).view(np.int32))
    if rows:
        assert np.signbit(hard[0, 0, 0]) and hard[0, 0, 0] == 0 and hard[1, -1, 1:2].view(np.uint32)[0] == E.NAN_WORD


def test_noise_definition_pins_after_the_noise_and_reads_the_table_of_t():
    assert len(set(E.EXTRA_BY_T.tolist())) == E.T_STEPS and all(float(F32(v)) == float(v) for v in E.EXTRA_BY_T)
    z = E.noise_input(6)
    for v in E.Z_PLANTS:
        assert (z.view(np.int32) == F32(v).view(np.int32)).sum() >= (6 if abs(v) < 1 else 1)
    assert np.all(np.abs(z[:-1]) < 1e3)
    tb = E.real_tables()
    rows = (0, 17, 40, 63)
    hard = E.hard_values(rows)
    x, e = E.step_input(6), E.step_input(6, 341)
    co = M.ddpm_coeffs(tb, 7, E.EXTRA_BY_T)
    y = M.step32(co, x, e, z, rows, hard, 2)
    for t in rows:
        assert np.array_equal(y[:, t].view(np.int32), np.repeat(hard, 2, axis=0)[:, M.slots_of(rows)[t]].view(np.int32))
    assert not M.same_words(y, M.step32(co._replace(extra=E.EXTRA_BY_T[0]), x, e, z, rows, hard, 2))


def test_cross_ladders_reach_both_sides_of_both_bounds_and_match_the_oracle():
    for name, rel in E.CROSS_RELS.items():
        for ind1, ind2 in ((63, 0), (0, 63), (0, 0), (63, 63)):
            x1, x2, rel32, bnd = E.cross_input(rel, ind1, ind2)
            assert np.array_equal(bnd != 1e6, rel32 != 0) and (name != "rev" or bnd[0] == -1)
            with np.errstate(invalid="ignore"):
                s = x2[:, ind2] + rel32
                fin = np.isfinite(s)
                for c in range(D):
                    assert (s[fin[:, c], c] < bnd[c]).sum() >= 16 and (s[fin[:, c], c] > bnd[c]).sum() >= 8, (name, c)
                    if name != "diag" or c > 1:                        # (diag: -0.8 is no multiple of 1.2's ulp, the sum steps over it)
                        assert (s[fin[:, c], c] == bnd[c]).sum() >= 8, (name, c)
                    assert ((s - rel32)[fin[:, c], c] < -bnd[c]).sum() >= 8 or bnd[c] < 0, (name, c)
            assert np.isnan(x2[:, ind2]).any() and np.isposinf(x2[:, ind2]).any() and np.isneginf(x2[:, ind2]).any()
            for n in E.CROSS_N:
                y1, y2 = M.cross_condition(x1[:n], x2[:n], ind1, ind2, rel32, bnd)
                xs = {0: torch.from_numpy(x1[:n].copy()), 1: torch.from_numpy(x2[:n].copy())}
                O.apply_cross_conditioning(xs, {(0, 1): (ind1, ind2)}, {0: torch.zeros(2), 1: torch.from_numpy(rel32[:2].copy())})
                assert M.same_words(y1, xs[0].numpy()) and M.same_words(y2, xs[1].numpy()), (name, ind1, ind2, n)
    tab = E.by_robot_table()
    x1, x2, _, _ = E.cross_input(E.CROSS_RELS["fwd"], 63, 0, n=6)
    y1, y2 = M.cross_condition(x1, x2, 63, 0, None, None, by_robot=tab, spr=3)
    for r, k in enumerate(("fwd", "diag")):
        w1, w2 = M.cross_condition(x1[3 * r:3 * r + 3], x2[3 * r:3 * r + 3], 63, 0, E.CROSS_RELS[k], E.boundary_of(E.CROSS_RELS[k]))
        assert M.same_words(y1[3 * r:3 * r + 3], w1) and M.same_words(y2[3 * r:3 * r + 3], w2)


def test_q_sample_bound_holds_for_both_fp32_forms():
    tb = E.real_tables()
    for n in E.Q_N:
        x0, z = E.q_input(n)
        assert x0.size // D in (64, 256, 320)
        for t in (0, 12, E.T_STEPS - 1):
            a, b = tb["sqrt_alphas_cumprod"][t], tb["sqrt_one_minus_alphas_cumprod"][t]
            ref, bound = M.q_sample64(x0, z, a, b), M.q_sample_bound(x0, z, a, b)
            plain = (a * x0 + b * z).astype(F32)
            contracted = M.fma_f32(a, x0, b * z)
            assert np.all(np.abs(plain - ref) <= bound) and np.all(np.abs(contracted - ref) <= bound)
            assert np.all(np.abs(O.q_sample(_tb(tb), torch.from_numpy(x0), t, torch.from_numpy(z)).numpy() - ref) <= bound)
