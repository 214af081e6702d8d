"""-m gpu: the fused UNet kernel's dynamic per-sample input scales at the edges of their range, in all three launch forms.

dyn_scale (csrc/f16x2.h) reads the biased exponent of a sample's largest |x|, which reaches it through maxima taken on the bit patterns
(csrc/unet_kernel.h, max_nn): valid for operands whose sign bit is clear, which the kernel guarantees by taking |x| first.  The batch
below puts the cases that could break that into ONE batch, so that they also share workgroups: an all-zero sample, -0.0 entries, a
largest |x| that is a negative value, magnitudes from 2^-70 to 2^30, +inf and NaN.  One forward per kernel at the smallest sizes that
reach it: n = 3 per launch -> unet_kernel<1>; n = 5 with two_per_workgroup_max = -1 -> unet_kernel<4> (a full workgroup + a ragged one);
n = 257 -> unet_kernel<2> (the smallest size it runs at)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import synth                          # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet     # noqa: E402
from oracle import mmd_oracle as O                 # noqa: E402
from cases import H, D, rel_l2                     # noqa: E402

T_STEP = 63
# the rows of the edge batch (tests/layered_edge_cases.py, shared with the layer-by-layer path's tests), in an order that puts the inf / NaN
# samples into workgroups with finite ones: rows 5 .. 8 are one workgroup of unet_kernel<4> (launches of five rows: 0-4, 5-9, 10-14), rows
# (5, 6) and (7, 8) two workgroups of unet_kernel<2>
from layered_edge_cases import NAMES, ORACLE_ROWS, NON_FINITE, edge_batch, plain_batch     # noqa: E402


def forward_with(kernel, x):
    """x [N, H, D] (cpu) through unet_kernel<kernel>, rows kept adjacent: launches of 3 (<1>), of 5 (<4>), one launch of 257 (<2>: the
    rows + ordinary filler rows behind them)"""
    sd = synth.synth_unet_state_dict(0)
    unet = TemporalUnet(two_per_workgroup_max=-1) if kernel == 4 else TemporalUnet()
    unet.load_state_dict(sd)
    n = x.shape[0]
    if kernel == 2:
        filler = torch.from_numpy(synth.synth_noise(179, (257 - n, H, D)))
        return unet(torch.cat([x, filler]).cuda(), T_STEP).cpu()[:n]
    per = 3 if kernel == 1 else 5
    out = []
    for i in range(0, n, per):
        rows = x[i:i + per]
        pad = per - rows.shape[0]
        if pad:
            rows = torch.cat([rows, x[:pad]])
        out.append(unet(rows.contiguous().cuda(), T_STEP).cpu()[:per - pad])
    return torch.cat(out)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def outs():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    xe, xp = edge_batch(), plain_batch()
    return {"edge": {k: forward_with(k, xe) for k in (1, 2, 4)}, "plain": {k: forward_with(k, xp) for k in (1, 2, 4)}}


def test_rows_identical_across_kernels(outs):
    for which in ("edge", "plain"):
        o = outs[which]
        for i, name in enumerate(NAMES):
            assert same_bits(o[1][i], o[2][i]) and same_bits(o[1][i], o[4][i]), (which, name)


def test_finite_rows_do_not_see_inf_nan_neighbours(outs):
    """rows `one` and `eight` share a workgroup of unet_kernel<4> with the inf and the NaN sample, and one of unet_kernel<2> with one of
    them each: the same bits as next to ordinary samples"""
    for k in (1, 2, 4):
        for i, name in enumerate(NAMES):
            if name not in NON_FINITE:
                assert same_bits(outs["edge"][k][i], outs["plain"][k][i]), (k, name)


def test_rows_in_the_covered_range_meet_the_oracle_bound(outs):
    sd = O.state_dict_to_torch(synth.synth_unet_state_dict(0))
    x = edge_batch()
    rows = [NAMES.index(k) for k in ORACLE_ROWS]
    ref = O.unet_forward(sd, x[rows], torch.full((len(rows),), T_STEP, dtype=torch.long))
    errs = {name: rel_l2(outs["edge"][4][i], ref[j]) for j, (i, name) in enumerate(zip(rows, ORACLE_ROWS))}
    print("rel_l2 against the oracle:", errs)
    for name, e in errs.items():
        assert e < 2e-5, (name, e)


def test_inf_nan_rows_are_non_finite_and_the_others_finite(outs):
    """(a non-finite value reaches every element of its sample through the first GroupNorm's statistics)"""
    for k in (1, 2, 4):
        o = outs["edge"][k]
        for i, name in enumerate(NAMES):
            if name in NON_FINITE:
                assert not torch.isfinite(o[i]).any(), (k, name)
            else:
                assert torch.isfinite(o[i]).all(), (k, name)
