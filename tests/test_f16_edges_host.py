"""Host checks of tests/f16_edge_cases.py, on the ORACLE and the CPU emulation alone: what tests/test_gpu_f16_edges.py asks of
TemporalUnet(precision="f16") -- finite, and within f16_limit = max(bound(err_ref32), 2 x sens) of the float64 forward -- is met by the
one-piece emulation itself in both arithmetics on every weight set, input scale, finite edge row and time step; the mutants the limit
catches (a constant 2^6 for the static scales, a Mish without its clamp) land outside it; and two mutants it does NOT catch are
measured and printed, so that a reader knows where the device test's detection floor lies.  The scales are the restated ones of
tests/fused_edge_cases.py (scale_bounds / static_act_scale, pinned by tests/test_fused_edges_host.py), used unchanged.  No GPU."""
import pytest
import torch

import f16_edge_cases as F
import fused_edge_cases as E
import layered_edge_cases as L


def _cases_of(wset):
    return [c for c in F.SET_CASES if c[1] == wset]


# ---- the references alone meet what the device is asked for
@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_both_emulations_are_finite_and_within_the_limit_on_every_set(wset):
    for case in _cases_of(wset):
        _, _, emu64, emu32 = F.references(case)
        assert torch.isfinite(emu64).all() and torch.isfinite(emu32).all(), case
        assert emu64.dtype == torch.float64 and emu32.dtype == torch.float32
        err_ref32, e64, e32 = F.reference_errors(case)
        print(f"{F.case_name(case)}: one piece, float64 arithmetic {e64:.3g}, float32 arithmetic {e32:.3g}, fp32 forward {err_ref32:.3g}, "
              f"limit {F.f16_limit(case):.3g}")
        assert F.sens(case) == max(e64, e32) and 0 < e64 <= F.f16_limit(case) and 0 < e32 <= F.f16_limit(case), case
        assert F.f16_limit(case) == max(E.bound(err_ref32), 2 * F.sens(case))           # (the margin is the project's 2)
        # one piece is a different regime from two: far outside the f32 build's bound on every set
        assert min(e64, e32) > E.bound(err_ref32), case


def test_both_emulations_are_finite_and_within_the_limit_on_every_edge_row_and_time_step():
    assert len(F.ROW_CASES) == 9 and len(F.TIME_CASES) == E.TIME_T == 25
    for case in F.ROW_CASES + F.TIME_CASES:
        _, _, emu64, emu32 = F.references(case)
        assert torch.isfinite(emu64).all() and torch.isfinite(emu32).all(), case
        _, e64, e32 = F.reference_errors(case)
        print(f"{F.case_name(case)}: {e64:.3g} / {e32:.3g}, limit {F.f16_limit(case):.3g}")
        assert 0 < e64 <= F.f16_limit(case) and 0 < e32 <= F.f16_limit(case), case


def test_the_two_arithmetics_differ_by_about_their_own_error():
    """Why no whole-network comparison of the device against the emulation can be sharper than the one against float64: the SAME
    roundings under the SAME scales, once with float64 and once with float32 arithmetic, lie as far apart as each lies from the float64
    forward (fp32 noise flips fp16 roundings, and a flipped rounding is a full fp16 half-ulp that travels through the convs behind it)."""
    ratios = []
    for case in F.SET_CASES:
        ref64, _, emu64, emu32 = F.references(case)
        ratios.append(float((emu32.double() - emu64).norm() / ref64.norm()) / F.sens(case))
    print(f"|emu32 - emu64| / sens over {len(ratios)} cases: {min(ratios):.3g} .. {max(ratios):.3g}")
    assert max(ratios) > 0.25 and min(ratios) > 1e-4


# ---- mutants the limit catches
def _mutant_err(case, **switches):
    assert case[0] == "set"
    out = E.emulated_forward(E.state_dict(case[1]), E.accuracy_input(case[2]), E.T_STEP, low_piece=False, **switches)
    return F.err_against_fp64(out, case) if torch.isfinite(out).all() else float("inf")


@pytest.mark.parametrize("wset", ["gamma_x1024", "tb_x4096"])
@pytest.mark.parametrize("dtype", F.ARITHMETICS)
def test_a_constant_static_scale_lands_outside_the_limit(wset, dtype):
    """2^6 is the static scale of seed 0; at B = 2e4 (gamma_x1024) or 1.5e3 (tb_x4096) conv B's input times 2^6 leaves fp16's range"""
    case = ("set", wset, 1.0)
    err = _mutant_err(case, static_scale=64.0, dtype=dtype)
    print(f"{wset} {dtype}: static scale 2^6 everywhere {err:.3g}, limit {F.f16_limit(case):.3g}")
    assert err > F.f16_limit(case), (wset, err)


@pytest.mark.parametrize("dtype", F.ARITHMETICS)
def test_a_mish_without_its_clamp_goes_non_finite(dtype):
    case = ("set", "gamma_x1024", 1.0)
    assert _mutant_err(case, mish="kernel_noclamp", dtype=dtype) == float("inf")
    err = _mutant_err(case, mish="kernel", dtype=dtype)                     # ... and with the clamp the restated Mish is harmless
    assert err <= F.f16_limit(case), err


# ---- mutants the limit does NOT catch: recorded, not asserted
def test_mutants_below_the_detection_floor_are_recorded():
    """What tests/test_gpu_f16_edges.py cannot see.  Each mutant's error against float64 as a ratio to sens (the limit is at 2):
      * operands rounded ONCE to 10 significant bits where fp16 keeps 11 (a lost mantissa bit in every operand): the error about
        doubles, ratio 1.34 (beta+30) .. 3.50 (contrast-20) over the 20 sets at scale 1, median 1.9 -- it straddles the limit: beyond
        2 on five sets (colspread 2.11, beta-8 2.02, tb_x256 2.67, tb_x4096 2.55, contrast-20 3.50), inside it on fifteen.  A device
        that loses a whole bit EVERYWHERE is caught by those five; a loss confined to a few convs is not caught at all;
      * ONE weight scale per tensor where the packer has one per output column, on `colspread` (columns up to 2^16 apart): ratio
        1.00 / 0.99 / 1.00 at the three input scales -- invisible.  One fp16 piece is a floating-point number: a column 2^16 below the
        tensor's largest still keeps its 11 bits (it goes denormal only 2^28 below); the per-column scales earn their keep in the
        f32 build's LOW piece, which this mode does not have.
    Nothing is asserted beyond finiteness: these figures are the floor, not a requirement."""
    for wset in E.ALL_SETS:
        case = ("set", wset, 1.0)
        err = _mutant_err(case, operand_bits=10)
        print(f"10 significant bits, {F.case_name(case)}: {err:.3g} = {err / F.sens(case):.2f} x sens")
        assert err < float("inf")
    for case in _cases_of("colspread"):
        err = _mutant_err(case, weight_scale="tensor")
        print(f"one weight scale per tensor, {F.case_name(case)}: {err:.3g} = {err / F.sens(case):.2f} x sens")
        assert err < float("inf")
