"""Seeded builders for the layer-by-layer TemporalUnet's edge tests (tests/test_layered_edges_host.py on the oracle alone,
tests/test_gpu_layered_edges.py on the device): weight sets and inputs that put the matrix-pipe kernel's scale bookkeeping
(csrc/mconv_dev.h: a dynamic power-of-two scale per sample and 128-channel chunk, the rescale of the live accumulators between chunks,
per-column weight scales undone in the epilogue, the second dynamic scale of a one-launch residual block) far from the ratios near 1 that
the seed-0 weights give, and the float64 / fp32 oracle forwards of each case, computed once and shared.  No GPU."""
import functools

import numpy as np
import torch

from mmd_amd import synth
from oracle import mmd_oracle as O
from cases import H, D

# ---- the input batch at the edges of the dynamic scales' range (shared with tests/test_gpu_unet_scale_edges.py, whose docstring says what
# the order does for the fused kernel).  The layer kernels run the batch as ONE launch per layer, in which consecutive samples share a
# workgroup item: pairs at L = 32, fours at L = 16, eights at L = 8 (tests/test_gpu_layered_edges.py names the neighbours)
NAMES = ["zero", "neg_zero", "2^-70", "2^-20", "1e-3", "one", "inf", "eight", "nan", "2^30", "neg_max"]
ORACLE_ROWS = ["neg_zero", "1e-3", "one", "eight", "neg_max"]    # within the scales test_unet_forward_input_range covers (1e-3 .. 8)
NON_FINITE = ["inf", "nan"]
FINITE_ROWS = [k for k in NAMES if k not in NON_FINITE]          # the layered tests hold every one of them to the float64 forward


def edge_batch():
    x = synth.synth_noise(177, (len(NAMES), H, D))
    row = {k: i for i, k in enumerate(NAMES)}
    x[row["zero"]] = 0.0
    x[row["neg_zero"]].reshape(-1)[::3] = -0.0
    for k, s in (("2^-70", 2.0 ** -70), ("2^-20", 2.0 ** -20), ("1e-3", 1e-3), ("eight", 8.0), ("2^30", 2.0 ** 30)):
        x[row[k]] *= np.float32(s)
    x[row["neg_max"], 40, 2] = -(np.abs(x[row["neg_max"]]).max() + 1.0)      # the largest |x| is a negative value
    x[row["inf"], 9, 1] = np.inf
    x[row["nan"], 33, 0] = np.nan
    assert np.signbit(x[row["neg_zero"]].reshape(-1)[::3]).all() and x[row["neg_max"]].min() == -np.abs(x[row["neg_max"]]).max()
    return torch.from_numpy(x)


def plain_batch():
    """the edge batch with the inf / NaN samples replaced by ordinary ones"""
    x = edge_batch()
    fill = torch.from_numpy(synth.synth_noise(178, (len(NON_FINITE), H, D)))
    for j, k in enumerate(NON_FINITE):
        x[NAMES.index(k)] = fill[j]
    return x


# ---- weight sets
def _is_upsample(key):
    return key.startswith("ups.") and ".4.conv." in key


def wide_state_dict(uid=32, dm=(1, 2, 4)):
    """the `wide` set of test_unet_forward_accuracy_against_fp64 for any width and level count: every k5 conv weight times
    exp(U(-6, 2)) per element -- kernels that span five orders of magnitude, so that every piece of the fp16 split carries signal"""
    sd = synth.synth_unet_state_dict(2, unet_input_dim=uid, dim_mults=dm)
    rng = np.random.Generator(np.random.PCG64(9))
    for k, v in sd.items():
        if k.endswith(".block.0.weight"):
            sd[k] = (v * np.exp(rng.uniform(-6.0, 2.0, size=v.shape))).astype(np.float32)
    return sd


def column_spread_state_dict(uid=32, dm=(1, 2, 4, 8)):
    """every 3-D conv weight but the upsample convs': output channel c times 2^k(c), k an integer drawn from [-12, 4] (the per-column
    weight scales of the packs then differ by up to 2^16 between neighbouring columns); a conv with >= 32 output channels has one
    all-zero output channel (f16_scale_for's m = 0 branch; a constant channel inside a GroupNorm group), one with >= 32 input channels
    one all-zero input channel"""
    sd = synth.synth_unet_state_dict(3, unet_input_dim=uid, dim_mults=dm)
    rng = np.random.Generator(np.random.PCG64(11))
    for k, v in sd.items():
        if v.ndim != 3 or _is_upsample(k):
            continue
        w = v * np.exp2(rng.integers(-12, 5, size=v.shape[0]).astype(np.float64))[:, None, None]
        co, ci = int(rng.integers(v.shape[0])), int(rng.integers(v.shape[1]))      # (drawn for every conv: the stream does not depend on the widths)
        if v.shape[0] >= 32:
            w[co] = 0.0
        if v.shape[1] >= 32:
            w[:, ci] = 0.0
        sd[k] = w.astype(np.float32)
    return sd


def chunk_contrast_state_dict(uid=32, dm=(1, 2, 4, 8), e=20, last=True):
    """seed 0 with weight and bias of every ups.*.4.conv times 2^e.  The upsample has no norm, so the first half of the next level's
    cat(x, skip) scales exactly by 2^e (for e > 0 the residual stream carries the factor on: 2^2e at the level after): the input
    chunks that hold x and those that hold the skip differ by about 2^|e|, and the accumulators pass from one to the other with a ratio
    far from 1 -- upward for e < 0, downward for e > 0.
    last=False (the `inner` sets) leaves the LAST upsample alone, the one that feeds final_conv and no cat: with it scaled by 2^-20 the
    final Conv1dBlock's input sits far below its GroupNorm's eps and eps out is little more than that block's beta (the fp32 reference's
    error drops to 1.6e-7), so that an error made in the up blocks hardly reaches the output; with last=False it does."""
    sd = synth.synth_unet_state_dict(0, unet_input_dim=uid, dim_mults=dm)
    ups = sorted({k.rsplit(".", 1)[0] for k in sd if _is_upsample(k)})
    for conv in ups if last else ups[:-1]:
        for k in (conv + ".weight", conv + ".bias"):
            sd[k] = (sd[k] * np.float32(2.0 ** e)).astype(np.float32)
    return sd


CONTRAST_SETS = ("contrast+20", "contrast-20", "contrast_inner+20", "contrast_inner-20")
WEIGHT_SETS = ("seed0", "seed1", "wide", "colspread") + CONTRAST_SETS


def state_dict(name, uid, dm):
    if name in ("seed0", "seed1"):
        return synth.synth_unet_state_dict(int(name[-1]), unet_input_dim=uid, dim_mults=dm)
    if name == "wide":
        return wide_state_dict(uid, dm)
    if name == "colspread":
        return column_spread_state_dict(uid, dm)
    assert name in CONTRAST_SETS, name
    return chunk_contrast_state_dict(uid, dm, contrast_exponent(name), last="inner" not in name)


def contrast_exponent(name):
    return int(name[-3:])


# ---- the networks: tag -> (unet_input_dim, dim_mults, TemporalUnet options)
# (layered=True where the width would otherwise select the fused kernel)
NETS = {"mfma_d32_1248": (32, (1, 2, 4, 8), {}), "mfma_d64_1248": (64, (1, 2, 4, 8), {}),
        "valu_d32_124": (32, (1, 2, 4), dict(layered=True, layered_valu=True)), "valu_d40_124": (40, (1, 2, 4), {})}
SCALES = (1.0, 1e-3, 8.0)
T_STEP = 11
N_ACC = 6


def accuracy_input(scale):
    return torch.from_numpy(synth.synth_noise(300, (N_ACC, H, D))) * scale


def rel_err64(out, ref64):
    """relative L2 error against a float64 tensor, taken in float64"""
    return float((out.double() - ref64).norm() / ref64.norm())


def _forwards(sd_np, x, t):
    sd = O.state_dict_to_torch(sd_np)
    tt = torch.full((x.shape[0],), t, dtype=torch.long)
    ref64 = O.unet_forward({k: v.double() for k, v in sd.items()}, x.double(), tt)
    return ref64, O.unet_forward(sd, x, tt)


@functools.lru_cache(maxsize=None)
def accuracy_reference(net, wset, scale):
    """(float64 oracle forward, fp32 oracle forward) of accuracy_input(scale) at T_STEP -- computed once, never written to"""
    uid, dm, _ = NETS[net]
    return _forwards(state_dict(wset, uid, dm), accuracy_input(scale), T_STEP)


@functools.lru_cache(maxsize=None)
def edge_reference(net):
    """the same two forwards of the finite rows of edge_batch() on the seed-0 weights, [len(FINITE_ROWS), H, D]"""
    uid, dm, _ = NETS[net]
    rows = [NAMES.index(k) for k in FINITE_ROWS]
    return _forwards(synth.synth_unet_state_dict(0, unet_input_dim=uid, dim_mults=dm), edge_batch()[rows], T_STEP)


def bound(err_ref32):
    """the project's bound for a two-piece fp16 forward against float64 (test_unet_forward_accuracy_against_fp64): four times the fp32
    reference's own rounding error, floored at 4e-6"""
    return max(4e-6, 4 * err_ref32)


def ups_input_halves(sd_np, x, t):
    """the fp32 oracle's input to ups.i.0, i = 0 .., as (max |x|, max |skip|) over the batch: O.unet_forward's walk, stopped at each cat"""
    sd = O.state_dict_to_torch(sd_np)
    n_levels = O.unet_levels(sd)
    c = O.time_embedding(sd, torch.full((x.shape[0],), t, dtype=torch.long).to(x.dtype))
    x = x.transpose(1, 2)
    skips, out = [], []
    for ind in range(n_levels):
        x = O._rtb(sd, f"downs.{ind}.1", O._rtb(sd, f"downs.{ind}.0", x, c), c)
        skips.append(x)
        if ind < n_levels - 1:
            x = torch.nn.functional.conv1d(x, sd[f"downs.{ind}.4.conv.weight"], sd[f"downs.{ind}.4.conv.bias"], stride=2, padding=1)
    x = O._rtb(sd, "mid_block2", O._rtb(sd, "mid_block1", x, c), c)
    for ind in range(n_levels - 1):
        skip = skips.pop()
        out.append((float(x.abs().max()), float(skip.abs().max())))
        x = O._rtb(sd, f"ups.{ind}.1", O._rtb(sd, f"ups.{ind}.0", torch.cat((x, skip), dim=1), c), c)
        x = torch.nn.functional.conv_transpose1d(x, sd[f"ups.{ind}.4.conv.weight"], sd[f"ups.{ind}.4.conv.bias"], stride=2, padding=1)
    return out
