"""-m gpu: the fused TemporalUnet kernel (csrc/unet_kernel.h, packed by csrc/unet.hip) against the float64 forward at the edges of its
operands' range.

With the seed-0 / seed-1 / `wide` weights of test_unet_forward_accuracy_against_fp64 every GroupNorm gamma lies in [0.65, 1.33] and the
static scale bound B is 18 .. 22 for every block: static_act_scale is 2^6 everywhere, no pre-activation gets near the Mish's clamp at 20,
no GroupNorm group is constant or dominated by beta, no weight column is zero.  The weight sets of tests/fused_edge_cases.py (checked on
the oracle and on a CPU emulation of the kernel's operand rounding by tests/test_fused_edges_host.py) put B between 7 and 2e4, the
pre-activations between -30 and 1e4, gammas thirteen binades apart inside a group, and all-zero rows into the packs.  Every forward has
at most 6 trajectories but one launch of 257 per set (the smallest unet_kernel<2> runs at); the references are computed once
(fused_edge_cases.accuracy_reference / edge_reference / time_step_reference) and shared."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                          # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet     # noqa: E402
import fused_edge_cases as E                       # noqa: E402
import layered_edge_cases as L                     # noqa: E402
import parity_log                                  # noqa: E402
from cases import H, D                             # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _unet(wset, T=E.T_STEPS, **options):
    u = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=E.UID, dim_mults=E.DM, **options)
    u.load_state_dict(E.state_dict(wset))
    u.handle(T, "cuda")                            # the static scales rest on the time biases of steps 0 .. T - 1
    return u


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def forward_forms(wset, x, t):
    """x [n <= 6, H, D] (cpu) through the three launch forms, rows kept adjacent: unet_kernel<1> (one launch of n), unet_kernel<4>
    (two_per_workgroup_max = -1: at n = 6 a full workgroup and a ragged one), unet_kernel<2> (one launch of 257: the rows + ordinary
    filler rows behind them, as tests/test_gpu_unet_scale_edges.py does)"""
    n = x.shape[0]
    filler = torch.from_numpy(synth.synth_noise(179, (257 - n, H, D)))
    one = _unet(wset)
    return {1: one(x.cuda(), t).cpu(), 4: _unet(wset, two_per_workgroup_max=-1)(x.cuda(), t).cpu(),
            2: one(torch.cat([x, filler]).cuda(), t).cpu()[:n]}


# ---- 1. accuracy against float64
@pytest.mark.parametrize("wset", E.IN_RANGE)
def test_fused_forward_accuracy_against_fp64(wset):
    """unet_kernel<1> at n = 6 on every in-range set x inputs scaled by 1, 1e-3 and 8: the error against the float64 forward below
    max(4e-6, 4 x the fp32 reference's own error against it), the bound of test_unet_forward_accuracy_against_fp64."""
    unet = _unet(wset)
    for scale in E.SCALES:
        ref64, ref32 = E.accuracy_reference(wset, scale)
        out = unet(E.accuracy_input(scale).cuda(), E.T_STEP).cpu()
        assert torch.isfinite(out).all(), (wset, scale)
        err_ref32, err_hip = E.rel_err64(ref32, ref64), E.rel_err64(out, ref64)
        print(f"{wset} scale={scale:g}: err_hip {err_hip:.3g} err_ref32 {err_ref32:.3g} ratio {err_hip / err_ref32:.2f}")
        parity_log.record("fused_edges_vs_fp64", f"{wset} scale={scale:g}", None, err_hip, sens=err_ref32, bound=E.bound(err_ref32),
                          note="sens = the fp32 reference forward against the same float64 forward")
        assert err_hip < E.bound(err_ref32), (wset, scale, err_hip, err_ref32)


# ---- 2. the launch forms agree
@pytest.mark.parametrize("wset", E.ALL_SETS)
def test_launch_forms_agree_bit_for_bit(wset):
    """the six rows through unet_kernel<1>, <4> and <2>: the same bits -- the GroupNorm statistics of a whole sample (<1>, <4>) and
    the pairwise combine of two half samples (<2>: rw_half_stat + gn_combine) included, on constant groups, beta-dominated groups and
    gammas spread over binades"""
    outs = forward_forms(wset, E.accuracy_input(1.0), E.T_STEP)
    assert torch.isfinite(outs[1]).all()
    for i in range(E.N_ACC):
        assert same_bits(outs[1][i], outs[4][i]) and same_bits(outs[1][i], outs[2][i]), (wset, i)


# ---- 3. every finite edge row
def test_every_finite_edge_row_meets_the_fp64_bound():
    """zero, -0.0, 2^-70, 2^-20, 1e-3, one, eight, 2^30 and neg_max of edge_batch() on seed 0 at t = 63, row by row, to the bound of the
    accuracy test against float64 (tests/test_gpu_unet_scale_edges.py holds five of them to the fp32 oracle at 2e-5 and shows that
    the three launch forms agree on all of them)."""
    ref64, ref32 = E.edge_reference()
    x = E.edge_rows()
    unet = _unet("seed0")
    out = torch.cat([unet(x[i:i + 5].cuda(), E.T_EDGE).cpu() for i in (0, 5)])
    for j, name in enumerate(L.FINITE_ROWS):
        assert torch.isfinite(out[j]).all(), name
        err_ref32, err_hip = E.rel_err64(ref32[j], ref64[j]), E.rel_err64(out[j], ref64[j])
        print(f"{name}: err_hip {err_hip:.3g} err_ref32 {err_ref32:.3g} ratio {err_hip / err_ref32:.2f}")
        parity_log.record("fused_edges_rows_vs_fp64", name, None, err_hip, sens=err_ref32, bound=E.bound(err_ref32))
        assert err_hip < E.bound(err_ref32), (name, err_hip, err_ref32)


# ---- 4. every time step on the time-bias set
def test_every_time_step_on_the_time_bias_set():
    """cond_mlp.1 x 2^12, T = 25: conv B's static scale rests on the largest |time bias| over the 25 rows of the table; each t against
    float64 to the same bound."""
    unet = _unet(E.TIME_SET, T=E.TIME_T)
    xd = E.time_step_input().cuda()
    for t in range(E.TIME_T):
        ref64, ref32 = E.time_step_reference(t)
        out = unet(xd, t).cpu()
        assert torch.isfinite(out).all(), t
        err_ref32, err_hip = E.rel_err64(ref32, ref64), E.rel_err64(out, ref64)
        parity_log.record("fused_edges_time_steps", f"t{t}", None, err_hip, sens=err_ref32, bound=E.bound(err_ref32))
        assert err_hip < E.bound(err_ref32), (t, err_hip, err_ref32)


# ---- 5. beyond the range
EMULATION_MARGIN = E.EMULATION_MARGIN


@pytest.mark.parametrize("wset", E.OUT_OF_RANGE)
def test_beyond_the_range_the_error_follows_the_emulation(wset):
    """in_spread16 / in_spread20: conv B's input channels 2^16 / 2^20 apart under ONE static scale.  The output is finite and the error
    against float64 at most max(bound, 2 x the emulated error) -- the margin test_f16_mode_is_on_and_within_twice_its_emulation gives the
    same kind of emulation (float64 accumulation: a floor for the kernel).
    Measured err_hip / emulated (profiles/fused_edges_parity.json): in_spread16 1.00 / 1.01 / 0.99 at scales 1 / 1e-3 / 8 (err_hip 1.72e-5,
    9.97e-5, 8.02e-6: 17 .. 38 x the fp32 reference's error), in_spread20 0.97 / 1.01 / 0.97 (2.48e-4, 9.12e-4, 1.24e-4: 253 .. 348 x) --
    the operand rounding the emulation models is all of the kernel's error there, and the margin 2 stands."""
    unet = _unet(wset)
    for scale in E.SCALES:
        ref64, ref32 = E.accuracy_reference(wset, scale)
        out = unet(E.accuracy_input(scale).cuda(), E.T_STEP).cpu()
        assert torch.isfinite(out).all(), (wset, scale)
        err_ref32, err_hip, err_emu = E.rel_err64(ref32, ref64), E.rel_err64(out, ref64), E.rel_err64(E.emulated_reference(wset, scale), ref64)
        limit = max(E.bound(err_ref32), EMULATION_MARGIN * err_emu)
        print(f"{wset} scale={scale:g}: err_hip {err_hip:.3g} emulated {err_emu:.3g} ratio {err_hip / err_emu:.2f}; "
              f"err_ref32 {err_ref32:.3g} ratio {err_hip / err_ref32:.1f}")
        parity_log.record("fused_edges_beyond_range", f"{wset} scale={scale:g}", None, err_hip, sens=err_emu, bound=limit,
                          err_ref32=err_ref32, note="sens = the two-piece CPU emulation against the same float64 forward")
        assert err_hip <= limit, (wset, scale, err_hip, err_emu, err_ref32)
