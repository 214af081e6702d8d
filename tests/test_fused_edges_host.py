"""Host checks of tests/fused_edge_cases.py, on the ORACLE and the CPU emulation alone: every weight set that tests/test_gpu_fused_edges.py
holds the fused kernel to is one at which the fp32 reference is finite and well conditioned (so the device bound max(4e-6, 4 x its error)
is never loosened by a badly conditioned reference), the builders do to the weights what they say, the two-piece emulation of the
kernel's operand rounding puts the sets of IN_RANGE inside that bound and those of OUT_OF_RANGE outside it, and the sets discriminate:
three mutants of the emulation -- no low piece, no clamp in the Mish, a constant 2^6 for the static scales -- each trip the sets built
for them.  No GPU."""
import numpy as np
import pytest
import torch

import fused_edge_cases as E
import layered_edge_cases as L
from cases import H, D

WELL_CONDITIONED = 1e-5


def _err32(wset, scale):
    ref64, ref32 = E.accuracy_reference(wset, scale)
    return E.rel_err64(ref32, ref64)


@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_fp32_oracle_is_finite_and_well_conditioned_on_every_set(wset):
    for scale in E.SCALES:
        ref64, ref32 = E.accuracy_reference(wset, scale)
        assert ref32.shape == (E.N_ACC, H, D) and torch.isfinite(ref32).all() and float(ref64.norm()) > 1.0, (wset, scale)
        err = E.rel_err64(ref32, ref64)
        print(wset, scale, f"fp32 oracle against float64: {err:.3g}")
        assert err < WELL_CONDITIONED, (wset, scale, err)


def test_fp32_oracle_is_well_conditioned_on_every_finite_edge_row_and_time_step():
    ref64, ref32 = E.edge_reference()
    assert ref64.shape == (9, H, D) and torch.isfinite(ref32).all()
    for i, name in enumerate(L.FINITE_ROWS):
        assert E.rel_err64(ref32[i], ref64[i]) < WELL_CONDITIONED, name
    for t in range(E.TIME_T):
        ref64, ref32 = E.time_step_reference(t)
        assert torch.isfinite(ref32).all() and E.rel_err64(ref32, ref64) < WELL_CONDITIONED, t


# ---- the builders
def test_builders_are_seeded_and_come_from_the_layered_sets_where_they_can():
    for wset in E.ALL_SETS:
        a, b = E.state_dict(wset), E.state_dict(wset)
        assert list(a) == list(E.state_dict("seed0")), wset
        for k in a:
            assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]) and np.isfinite(a[k]).all(), (wset, k)
    for wset in E.LAYERED_SETS:
        a, b = E.state_dict(wset), L.state_dict(wset, 32, (1, 2, 4))
        assert all(np.array_equal(a[k], b[k]) for k in a), wset
    assert set(E.OUT_OF_RANGE) == {"in_spread16", "in_spread20"} and not set(E.OUT_OF_RANGE) & set(E.IN_RANGE)
    assert len(E.IN_RANGE) == 18 and len(set(E.IN_RANGE)) == 18


def test_builders_change_what_they_say_and_nothing_else():
    s0 = E.state_dict("seed0")

    def changed(sd):
        return {k for k in sd if not np.array_equal(sd[k], s0[k])}

    gammas = {k for k in s0 if k.endswith(".block.2.weight")}
    betas = {k for k in s0 if k.endswith(".block.2.bias")}
    assert len(gammas) == len(betas) == 25
    for k in (3, 6, 10):
        sd = E.gamma_scaled_state_dict(k)
        assert changed(sd) == gammas and all(np.array_equal(sd[g], s0[g] * np.float32(2.0 ** k)) for g in gammas)
    sd = E.gamma_spread_state_dict()
    assert changed(sd) == gammas
    for g in gammas:
        k = np.log2(sd[g] / s0[g])
        assert np.array_equal(k, np.round(k)) and k.min() == -12 and k.max() == 0, g            # exact powers of two, both ends present
    for shift in (-8, -30, 30, 200):
        sd = E.beta_shifted_state_dict(shift)
        kept = {"final_conv.0.block.2.bias"} if shift == -30 else set()
        assert changed(sd) == betas - kept and all(np.array_equal(sd[b], s0[b] + np.float32(shift)) for b in betas - kept)
    for k in (8, 12):
        sd = E.time_bias_scaled_state_dict(k)
        cond = {key for key in s0 if ".cond_mlp.1." in key}
        assert len(cond) == 24 and changed(sd) == cond and all(np.array_equal(sd[c], s0[c] * np.float32(2.0 ** k)) for c in cond)
    sd = E.zero_variance_state_dict()
    assert changed(sd) == {f"{b}.block.0.{p}" for b in E.CONV_BLOCKS for p in ("weight", "bias")}
    for b in E.CONV_BLOCKS:
        w, bias = sd[f"{b}.block.0.weight"], sd[f"{b}.block.0.bias"]
        cg = w.shape[0] // 8
        assert not w[:cg].any() and (bias[:cg] == bias[0]).all() and bias[0] != 0 and w[cg:].all(axis=(1, 2)).all(), b
        assert np.array_equal(w[cg:], s0[f"{b}.block.0.weight"][cg:]) and np.array_equal(bias[cg:], s0[f"{b}.block.0.bias"][cg:]), b
    for e in (8, 12, 16, 20):
        sd, ks = E.in_spread_state_dict(e), E.in_spread_exponents(e)
        for r, k in ks.items():
            assert k.min() == 0 and k.max() == e, (e, r)
            up = np.exp2(k.astype(np.float64)).astype(np.float32)
            assert np.array_equal(sd[f"{r}.blocks.1.block.0.weight"], s0[f"{r}.blocks.1.block.0.weight"] * up[None, :, None])
            for key in (f"{r}.blocks.0.block.2.weight", f"{r}.blocks.0.block.2.bias", f"{r}.cond_mlp.1.bias"):
                assert np.array_equal(sd[key] * up, s0[key]), (e, key)                            # (powers of two: exact both ways)
            assert np.array_equal(sd[f"{r}.cond_mlp.1.weight"] * up[:, None], s0[f"{r}.cond_mlp.1.weight"]), (e, r)
        assert len(changed(sd)) == 5 * 12


# B = max_c (max(0.31, 16 |gamma_c| + |beta_c|) + max_t |tb_c(t)|) over the thirteen convs with a static input scale, as (lowest, highest)
# brackets [lo, hi) each -- seed 0 gives 18 .. 22 (scale 2^6) everywhere
B_RANGE = {"gamma_x8": ((144, 176), (144, 176)), "gamma_x64": ((1152, 1408), (1152, 1408)), "gamma_x1024": ((18432, 22528), (18432, 22528)),
           "gamma_spread": ((9, 20), (18, 22)), "beta-8": ((26, 30), (26, 30)), "beta-30": ((18, 22), (48, 52)), "beta+30": ((48, 52), (48, 52)),
           "beta+200": ((218, 222), (218, 222)), "tb_x256": ((18, 22), (64, 128)), "tb_x4096": ((18, 22), (1024, 2048)),
           "in_spread8": ((7, 22), (18, 22)), "in_spread12": ((7, 22), (18, 22)), "in_spread16": ((7, 22), (18, 22)),
           "in_spread20": ((7, 22), (18, 22))}


@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_static_scale_bound_spans_what_the_set_is_built_for(wset):
    B = E.scale_bounds(E.state_dict(wset))
    assert len(B) == 13
    lo, hi = min(B.values()), max(B.values())
    print(wset, f"B {lo:.4g} .. {hi:.4g}")
    (lo0, lo1), (hi0, hi1) = B_RANGE.get(wset, ((18, 22), (18, 22)))
    assert lo0 <= lo < lo1 and hi0 <= hi < hi1, (wset, lo, hi)


def test_static_act_scale_restates_the_packer():
    """2^(10 - floor(log2 B)): the input stays below 2048 whatever the data; B = 20 gives 2^6, a power of two its own exponent; the time
    bias enters with its maximum over ALL steps and the 1.001 margin of the packer"""
    one, zero = np.ones(4, np.float32), np.zeros(4, np.float32)
    assert E.static_act_scale(one * 1.25, zero, zero) == 2.0 ** 6                       # B = 20
    assert E.static_act_scale(one, zero, zero) == 2.0 ** 6                              # B = 16: [16, 32) -> 2^6
    assert E.static_act_scale(one * np.float32(0.999), zero, zero) == 2.0 ** 7
    assert E.static_act_scale(zero, zero, zero) == 2.0 ** 12                            # B = 0.31
    assert E.static_act_scale(one, -one * 15, one) == 2.0 ** 5                          # 16 + 15 + 1.001
    assert E.static_act_scale(one * np.inf, zero, zero) == 1.0
    sd64 = {k: v.double() for k, v in E.O.state_dict_to_torch(E.state_dict("tb_x4096")).items()}
    tb25, tb100 = E.time_bias_absmax(sd64, 25), E.time_bias_absmax(sd64, 100)
    assert all((tb100[r] >= tb25[r]).all() for r in E.RTBS) and any((tb100[r] > tb25[r]).any() for r in E.RTBS)
    # ... and it is the maximum over the rows a forward can read: row t of the oracle's own time bias
    t = 17
    c = E.O.time_embedding(sd64, torch.tensor([float(t)], dtype=torch.float64))
    r = "mid_block1"
    tb = E.O.F.linear(E.O.F.mish(c), sd64[f"{r}.cond_mlp.1.weight"], sd64[f"{r}.cond_mlp.1.bias"])[0].abs()
    assert (tb <= tb25[r] * (1 + 1e-12)).all() and (tb25[r] > 100).any()       # (a batch of 25 rows rounds differently from one row)


def test_pre_activations_lie_where_the_sets_put_them():
    x = E.accuracy_input(1.0)
    for wset, check in (("seed0", lambda p: p.abs().max() < 20), ("gamma_x8", lambda p: p.max() > 20 and p.min() < -20),
                        ("gamma_x1024", lambda p: p.max() > 2000), ("beta+30", lambda p: p.min() > 20), ("beta+200", lambda p: p.min() > 20),
                        ("beta-8", lambda p: p.max() < 0), ("tb_x4096", lambda p: p.abs().max() < 20)):
        _, _, pre = E.traced_forward(E.state_dict(wset), x, E.T_STEP)
        for blk, p in zip(E.CONV_BLOCKS, pre):
            print(wset, blk, f"pre-Mish {float(p.min()):.4g} .. {float(p.max()):.4g}")
        assert all(check(p) for p in pre), wset
    _, _, pre = E.traced_forward(E.state_dict("beta-30"), x, E.T_STEP)
    assert E.CONV_BLOCKS[-1] == "final_conv.0" and all(p.max() < -20 for p in pre[:-1]) and pre[-1].max() > 0


def test_zero_variance_groups_are_constant_in_the_oracle():
    sd = E.state_dict("zerovar")
    for scale in E.SCALES:
        _, gn_in, pre = E.traced_forward(sd, E.accuracy_input(scale), E.T_STEP)
        for blk, g, p in zip(E.CONV_BLOCKS, gn_in, pre):
            cg = g.shape[1] // 8
            assert (g[:, :cg] == float(sd[f"{blk}.block.0.bias"][0])).all(), blk                 # one constant: variance exactly 0
            beta = torch.from_numpy(sd[f"{blk}.block.2.bias"][:cg]).double()
            # x_hat = 0 up to the rounding of the mean (times rstd = 316): the pre-activation is beta
            assert torch.allclose(p[:, :cg], beta[None, :, None].expand_as(p[:, :cg]), rtol=0.0, atol=1e-12), blk
            assert float(g[:, cg:2 * cg].var()) > 0


# ---- the range, pinned on the emulation
@pytest.mark.parametrize("wset", E.IN_RANGE)
def test_emulation_is_inside_the_bound_on_every_in_range_set(wset):
    for scale in E.SCALES:
        ref64, _ = E.accuracy_reference(wset, scale)
        emu = E.emulated_reference(wset, scale)
        assert torch.isfinite(emu).all()
        err, b = E.rel_err64(emu, ref64), E.bound(_err32(wset, scale))
        print(wset, scale, f"emulated {err:.3g} bound {b:.3g} ratio {err / b:.2f}")
        assert err < b, (wset, scale, err, b)


@pytest.mark.parametrize("wset", E.OUT_OF_RANGE)
def test_emulation_is_outside_the_bound_on_the_out_of_range_sets(wset):
    """one static scale per conv input: with conv B's input channels 2^16 (2^20) apart the small channels keep 2^-22 x 2^16 (2^20) of
    their own size, and the emulation -- a floor for the kernel -- lands 2 .. 9 (32 .. 86) times outside the bound"""
    for scale in E.SCALES:
        ref64, _ = E.accuracy_reference(wset, scale)
        emu = E.emulated_reference(wset, scale)
        assert torch.isfinite(emu).all()
        err, b = E.rel_err64(emu, ref64), E.bound(_err32(wset, scale))
        print(wset, scale, f"emulated {err:.3g} bound {b:.3g} ratio {err / b:.2f}")
        assert err > b, (wset, scale, err, b)


def test_edge_rows_and_time_steps_are_inside_the_bound_on_the_emulation():
    ref64, ref32 = E.edge_reference()
    emu = E.emulated_forward(E.state_dict("seed0"), E.edge_rows(), E.T_EDGE)
    for i, name in enumerate(L.FINITE_ROWS):
        assert E.rel_err64(emu[i], ref64[i]) < E.bound(E.rel_err64(ref32[i], ref64[i])), name
    sd = E.state_dict(E.TIME_SET)
    for t in (0, 1, 12, 24):
        ref64, ref32 = E.time_step_reference(t)
        emu = E.emulated_forward(sd, E.time_step_input(), t, T=E.TIME_T)
        assert E.rel_err64(emu, ref64) < E.bound(E.rel_err64(ref32, ref64)), t


# ---- the sets discriminate: mutants of the emulation
def _mutant(wset, **switches):
    ref64, _ = E.accuracy_reference(wset, 1.0)
    out = E.emulated_forward(E.state_dict(wset), E.accuracy_input(1.0), E.T_STEP, **switches)
    return (E.rel_err64(out, ref64) if torch.isfinite(out).all() else float("inf")), E.bound(_err32(wset, 1.0))


@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_without_the_low_piece_every_set_exceeds_its_bound(wset):
    err, b = _mutant(wset, low_piece=False)
    print(wset, f"one fp16 piece per operand: {err:.3g}, bound {b:.3g}")
    assert err > b, (wset, err, b)


def test_without_the_clamp_the_mish_goes_non_finite_on_large_gammas():
    """y n / (n + 2), n = e^y (e^y + 2): without min(y, 20) n overflows (in float64 from y = 355 on, in the kernel's fp32 from 44 on) and
    inf / inf is NaN.  With the clamp the restated Mish changes nothing that the bound could see, on any gamma set."""
    err, _ = _mutant("gamma_x1024", mish="kernel_noclamp")
    assert err == float("inf")
    for wset in ("gamma_x8", "gamma_x64", "gamma_x1024", "beta+200", "beta-30"):
        err, b = _mutant(wset, mish="kernel")
        print(wset, f"the kernel's Mish, clamped: {err:.3g}, bound {b:.3g}")
        assert err < b, (wset, err, b)
    y = torch.tensor([-800.0, -30.0, -1.0, 0.0, 1.0, 19.9, 20.0, 20.1, 300.0, 1e4], dtype=torch.float64)
    assert torch.allclose(E.kernel_mish(y), torch.nn.functional.mish(y), rtol=1e-12, atol=0.0)
    assert not torch.isfinite(E.kernel_mish(y, clamp=False)).all()


@pytest.mark.parametrize("wset", ["gamma_x1024", "tb_x4096"])
def test_with_a_constant_static_scale_the_large_bound_sets_fail(wset):
    """2^6 is what static_act_scale gives on seed 0 (B = 18 .. 22): at B = 2e4 or 1.5e3 an input times 2^6 leaves fp16"""
    err, b = _mutant(wset, static_scale=64.0)
    print(wset, f"static scale 2^6 everywhere: {err:.3g}, bound {b:.3g}")
    assert err > b, (wset, err, b)
    err, b = _mutant("seed0", static_scale=64.0)
    assert err < b
