"""Host checks of tests/layered_edge_cases.py, on the ORACLE alone: every weight set and input that tests/test_gpu_layered_edges.py holds
the layer kernels to is one at which the fp32 reference itself is finite and well conditioned (relative L2 error against the float64
forward below 4e-6 -- so the device bound max(4e-6, 4 x that error) is never loosened by a badly conditioned reference), the builders do
to the weights what they say, and the contrast sets do put the two halves of an up block's input 2^15 or more apart.  No GPU."""
import numpy as np
import pytest
import torch

import layered_edge_cases as E
from cases import H, D

WELL_CONDITIONED = 4e-6


@pytest.mark.parametrize("net", list(E.NETS))
def test_fp32_oracle_is_finite_and_well_conditioned_on_every_case(net):
    for wset in E.WEIGHT_SETS:
        for scale in E.SCALES:
            ref64, ref32 = E.accuracy_reference(net, wset, scale)
            assert ref32.shape == (E.N_ACC, H, D) and torch.isfinite(ref32).all() and float(ref64.norm()) > 1.0, (net, wset, scale)
            err = E.rel_err64(ref32, ref64)
            print(net, wset, scale, f"fp32 oracle against float64: {err:.3g}")
            assert err < WELL_CONDITIONED, (net, wset, scale, err)


@pytest.mark.parametrize("net", ["mfma_d32_1248", "valu_d40_124"])
def test_fp32_oracle_is_well_conditioned_on_every_finite_edge_row(net):
    """the rows the fused kernel's test left out of its oracle rows included: at 2^-70 (the all-zero row's bits but for the first conv) and
    at 2^30 the four-level seed-0 forward is as well conditioned as at 1 (measured 1.3e-6 and 3.6e-7)"""
    ref64, ref32 = E.edge_reference(net)
    assert torch.isfinite(ref32).all()
    for i, name in enumerate(E.FINITE_ROWS):
        err = E.rel_err64(ref32[i], ref64[i])
        print(net, name, f"fp32 oracle against float64: {err:.3g}")
        assert err < WELL_CONDITIONED, (net, name, err)


@pytest.mark.parametrize("net", list(E.NETS))
@pytest.mark.parametrize("wset", E.CONTRAST_SETS)
def test_contrast_sets_put_the_halves_of_an_up_blocks_input_far_apart(net, wset):
    """the oracle's input to ups.1.0 (and ups.2.0 of a four-level net): max |x| and max |skip| at least 2^15 apart, in the direction of e;
    ups.0.0, which no scaled upsample feeds, within 2^4"""
    uid, dm, _ = E.NETS[net]
    e = E.contrast_exponent(wset)
    for scale in E.SCALES:
        halves = E.ups_input_halves(E.state_dict(wset, uid, dm), E.accuracy_input(scale), E.T_STEP)
        assert len(halves) == len(dm) - 1
        ratios = [np.log2(a / b) for a, b in halves]
        print(net, wset, scale, "log2(max |x| / max |skip|) per up level:", np.round(ratios, 1))
        assert abs(ratios[0]) < 4
        for r in ratios[1:]:
            assert r * np.sign(e) >= 15, (net, wset, scale, ratios)


def test_builders_are_seeded_and_do_what_they_say():
    base = E.synth.synth_unet_state_dict(3, unet_input_dim=32, dim_mults=(1, 2, 4, 8))
    cs = E.column_spread_state_dict(32, (1, 2, 4, 8))
    again = E.column_spread_state_dict(32, (1, 2, 4, 8))
    spread = []
    for k, v in cs.items():
        assert np.array_equal(v, again[k]) and v.dtype == np.float32, k
        if v.ndim != 3 or E._is_upsample(k):
            assert np.array_equal(v, base[k]), k
            continue
        zero_out = [c for c in range(v.shape[0]) if not v[c].any()]
        zero_in = [c for c in range(v.shape[1]) if not v[:, c].any()]
        assert len(zero_out) == (v.shape[0] >= 32) and len(zero_in) == (v.shape[1] >= 32), k
        live = v[:, [c for c in range(v.shape[1]) if c not in zero_in]]
        for c in range(v.shape[0]):
            if c in zero_out:
                continue
            ks = np.log2(live[c] / base[k][c][[j for j in range(v.shape[1]) if j not in zero_in]])
            assert (ks == ks.flat[0]).all() and ks.flat[0] == int(ks.flat[0]) and -12 <= ks.flat[0] <= 4, (k, c)     # one exact power of two
            spread.append(int(ks.flat[0]))
    assert min(spread) == -12 and max(spread) == 4
    for e in (20, -20):
        cc = E.chunk_contrast_state_dict(32, (1, 2, 4, 8), e)
        s0 = E.synth.synth_unet_state_dict(0, unet_input_dim=32, dim_mults=(1, 2, 4, 8))
        ups = [k for k in cc if E._is_upsample(k)]
        assert len(ups) == 6                                                       # weight and bias of ups.0 .. 2
        inner = E.chunk_contrast_state_dict(32, (1, 2, 4, 8), e, last=False)
        for k in cc:
            assert np.array_equal(cc[k], s0[k] * np.float32(2.0 ** e) if k in ups else s0[k]), k
            assert np.array_equal(inner[k], s0[k] if k.startswith("ups.2.4.") else cc[k]), k
    # the `wide` set at the fused kernel's configuration is the one test_unet_forward_accuracy_against_fp64 builds
    wide = E.synth.synth_unet_state_dict(2)
    rng = np.random.Generator(np.random.PCG64(9))
    for k, v in wide.items():
        if k.endswith(".block.0.weight"):
            wide[k] = (v * np.exp(rng.uniform(-6.0, 2.0, size=v.shape))).astype(np.float32)
    mine = E.wide_state_dict(32, (1, 2, 4))
    assert all(np.array_equal(wide[k], mine[k]) for k in wide)


def test_edge_batch_rows_are_what_their_names_say():
    x, p = E.edge_batch(), E.plain_batch()
    row = {k: i for i, k in enumerate(E.NAMES)}
    assert x.shape == (11, H, D) and not x[row["zero"]].any() and torch.isinf(x[row["inf"]]).sum() == 1 and torch.isnan(x[row["nan"]]).sum() == 1
    assert 2.0 ** -72 < float(x[row["2^-70"]].abs().max()) < 2.0 ** -67 and 2.0 ** 30 < float(x[row["2^30"]].abs().max()) < 2.0 ** 33
    assert torch.isfinite(p).all()
    for k in E.FINITE_ROWS:
        assert torch.equal(x[row[k]].view(torch.int32), p[row[k]].view(torch.int32)), k
    # the neighbours the layer kernels give the non-finite rows (consecutive samples share an item: 2 at L = 32, 4 at L = 16, 8 at L = 8)
    assert row["inf"] == 6 and row["nan"] == 8 and E.NAMES[7] == "eight" and E.NAMES[9] == "2^30"
