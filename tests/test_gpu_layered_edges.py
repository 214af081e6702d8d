"""-m gpu: the layer-by-layer TemporalUnet (csrc/unet_layers.hip, mconv_dev.h, layers_valu_dev.h) against the float64 forward at the edges
of its operands' range.

mconv_kernel keeps more scale bookkeeping than the fused kernel: a dynamic power-of-two scale per sample AND per 128-channel chunk (from
LDS-atomic maxima), an exact rescale of the live accumulators when a new chunk starts, per-column weight scales undone in the epilogue, a
second dynamic scale for the hidden tensor of a one-launch residual block (KIND 4), and up to eight samples in one workgroup item.  With the
seed-0 weights and inputs of magnitude 1 the scales of neighbouring chunks, columns and samples sit within a binade or two of each other,
where a wrong ratio can hide under 2e-5 or cancel in a bitwise self-comparison; the weight sets and inputs of tests/layered_edge_cases.py
(checked on the oracle alone by tests/test_layered_edges_host.py) put them 2^16 .. 2^40 apart.  Every forward here has at most 16
trajectories; the references are computed once (layered_edge_cases.accuracy_reference / edge_reference) and shared."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                          # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet     # noqa: E402
from oracle import mmd_oracle as O                 # noqa: E402
import layered_edge_cases as E                     # noqa: E402
import parity_log                                  # noqa: E402
from cases import H, D, rel_l2                     # noqa: E402

T_STEP = E.T_STEP


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _unet(net, wset, **more):
    uid, dm, options = E.NETS[net]
    u = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=uid, dim_mults=dm, **{**options, **more})
    u.load_state_dict(E.state_dict(wset, uid, dm))
    return u


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. accuracy against float64
@pytest.mark.parametrize("wset", E.WEIGHT_SETS)
@pytest.mark.parametrize("net", list(E.NETS))
def test_layered_forward_accuracy_against_fp64(net, wset):
    """Both matrix-pipe networks (32 and 64 x (1, 2, 4, 8): up to four input chunks, KIND 4 blocks of 32 / 64 channels) and both
    vector-ALU ones (32 x (1, 2, 4) forced, 40 x (1, 2, 4)) x six weight sets x inputs scaled by 1, 1e-3 and 8: the error against the
    float64 forward below max(4e-6, 4 x the fp32 reference's own error against it) -- the fused kernel's bound
    (test_unet_forward_accuracy_against_fp64); the factor 4 is a margin over the reference's rounding error, not a measurement."""
    unet = _unet(net, wset)
    for scale in E.SCALES:
        ref64, ref32 = E.accuracy_reference(net, wset, scale)
        out = unet(E.accuracy_input(scale).cuda(), T_STEP).cpu()
        assert torch.isfinite(out).all(), (net, wset, scale)
        err_ref32, err_hip = E.rel_err64(ref32, ref64), E.rel_err64(out, ref64)
        print(f"{net} {wset} scale={scale:g}: err_hip {err_hip:.3g} err_ref32 {err_ref32:.3g} ratio {err_hip / err_ref32:.2f}")
        parity_log.record("layered_edges_vs_fp64", f"{net} {wset} scale={scale:g}", None, err_hip, sens=err_ref32, bound=E.bound(err_ref32),
                          note="sens = the fp32 reference forward against the same float64 forward")
        assert err_hip < E.bound(err_ref32), (net, wset, scale, err_hip, err_ref32)


# ---- 2. the launch forms agree on these weights
@pytest.mark.parametrize("wset", ("colspread",) + E.CONTRAST_SETS)
def test_launch_forms_agree_on_spread_and_contrast_weights(wset):
    """test_one_launch_residual_blocks_equal_the_two_launch_form's properties where the scales are far apart, at n = 13 (partial items
    at every level): rtb_fused 0, 64 and 128 give equal bits; rows 0 .. 4 equal a batch of those five rows alone, bit for bit (other
    neighbours in every item); slices of at most 32 columns and the vector-ALU form of every layer stay within 6e-6 of the default."""
    net = "mfma_d32_1248"
    x = torch.from_numpy(synth.synth_noise(301, (13, H, D))).cuda()
    outs = {f: _unet(net, wset, rtb_fused=f)(x, T_STEP) for f in (0, 64, 128)}
    assert torch.isfinite(outs[64]).all()
    assert same_bits(outs[0], outs[64]) and same_bits(outs[128], outs[64])
    default = _unet(net, wset)
    whole = default(x, T_STEP)
    assert same_bits(whole, outs[64])
    assert same_bits(default(x[:5].contiguous(), T_STEP), whole[:5])
    for name, other in (("mconv_max_cs=32", _unet(net, wset, mconv_max_cs=32)), ("layered_valu", _unet(net, wset, layered_valu=True))):
        err = rel_l2(other(x, T_STEP).cpu(), whole.cpu())
        print(f"{wset} {name} against the default: {err:.3g}")
        parity_log.record("layered_edges_forms", f"{wset} {name}", None, err, bound=6e-6)
        assert err < 6e-6, (wset, name, err)


# ---- 3. input-scale edges
EDGE_RUNS = (("mfma_d32_1248", 0), ("mfma_d32_1248", 64), ("valu_d40_124", -1))      # (net, rtb_fused; -1: the option's default)


@pytest.fixture(scope="module")
def edge_outs():
    xe, xp = E.edge_batch().cuda(), E.plain_batch().cuda()
    outs = {}
    for net, fused in EDGE_RUNS:
        unet = _unet(net, "seed0", rtb_fused=fused)
        outs[net, fused] = {"edge": unet(xe, T_STEP).cpu(), "plain": unet(xp, T_STEP).cpu()}
    return outs


def test_edge_rows_do_not_see_their_neighbours(edge_outs):
    """The 11 rows of edge_batch() -- zero, -0.0, 2^-70, 2^-20, 1e-3, one, inf, eight, nan, 2^30, neg_max -- as ONE batch, so that
    consecutive samples share a workgroup item of mconv_kernel (and its per-sample LDS maxima, taken with fmaxf, which drops NaN):
      L = 32 (pairs):  inf (row 6) with eight (7);  nan (8) with 2^30 (9)
      L = 16 (fours):  inf with 1e-3, one, eight (rows 4 .. 7);  nan with 2^30, neg_max (rows 8 .. 10)
      L = 8 (eights):  inf with zero, -0.0, 2^-70, 2^-20, 1e-3, one, eight (rows 0 .. 7);  nan with 2^30, neg_max (rows 8 .. 10)
    (L = 64: one sample per item).  Every finite row has the bits it has next to ordinary samples (plain_batch()), in the two-launch
    and the one-launch form of the residual blocks and on the vector-ALU network, and the two forms give the same bits."""
    for (net, fused), o in edge_outs.items():
        for i, name in enumerate(E.NAMES):
            if name not in E.NON_FINITE:
                assert same_bits(o["edge"][i], o["plain"][i]), (net, fused, name)
    for which in ("edge", "plain"):
        a, b = edge_outs["mfma_d32_1248", 0][which], edge_outs["mfma_d32_1248", 64][which]
        for i, name in enumerate(E.NAMES):
            if name not in E.NON_FINITE:
                assert same_bits(a[i], b[i]), (which, name)


def test_inf_nan_rows_are_non_finite_and_the_others_finite(edge_outs):
    """(a non-finite value reaches every element of its sample through the first GroupNorm's statistics; the all-zero row and the rows at
    2^-70 and 2^30 are finite)"""
    for key, o in edge_outs.items():
        assert torch.isfinite(o["plain"]).all(), key
        for i, name in enumerate(E.NAMES):
            if name in E.NON_FINITE:
                assert not torch.isfinite(o["edge"][i]).any(), (key, name)
            else:
                assert torch.isfinite(o["edge"][i]).all(), (key, name)


def test_every_finite_edge_row_meets_the_fp64_bound(edge_outs):
    """zero, -0.0, 2^-70, 2^-20, 1e-3, one, eight, 2^30 and neg_max, row by row, to the bound of the accuracy test against float64.  (The
    fused kernel's test leaves 2^-70 and 2^30 out of its oracle rows; the fp32 reference is well conditioned at both -- 1.3e-6 and 3.6e-7
    against float64 on the four-level network, pinned by tests/test_layered_edges_host.py.)"""
    for (net, fused), o in edge_outs.items():
        ref64, ref32 = E.edge_reference(net)
        for j, name in enumerate(E.FINITE_ROWS):
            i = E.NAMES.index(name)
            err_ref32, err_hip = E.rel_err64(ref32[j], ref64[j]), E.rel_err64(o["edge"][i], ref64[j])
            print(f"{net} rtb_fused={fused} {name}: err_hip {err_hip:.3g} err_ref32 {err_ref32:.3g} ratio {err_hip / err_ref32:.2f}")
            parity_log.record("layered_edges_rows_vs_fp64", f"{net} rtb_fused={fused} {name}", None, err_hip, sens=err_ref32,
                              bound=E.bound(err_ref32))
            assert err_hip < E.bound(err_ref32), (net, fused, name, err_hip, err_ref32)


# ---- 4. every time step
def test_every_time_step_against_the_oracle():
    """T = 25: the layered path's time table has one row of tb_total biases per step, each block's at its own offset; every row, the
    first and the last included, against the fp32 oracle at 2e-5 on the four-level network."""
    T, n = 25, 3
    unet = _unet("mfma_d32_1248", "seed0")
    unet.handle(T, "cuda")
    sd = O.state_dict_to_torch(E.state_dict("seed0", 32, (1, 2, 4, 8)))
    x = torch.from_numpy(synth.synth_noise(302, (n, H, D)))
    xd = x.cuda()
    for t in range(T):
        err = rel_l2(unet(xd, t).cpu(), O.unet_forward(sd, x, torch.full((n,), t, dtype=torch.long)))
        parity_log.record("layered_edges_time_steps", f"t{t}", None, err, bound=2e-5)
        assert err < 2e-5, (t, err)
