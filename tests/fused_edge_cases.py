"""Seeded builders for the fused TemporalUnet kernel's edge tests (tests/test_fused_edges_host.py on the oracle and a CPU emulation alone,
tests/test_gpu_fused_edges.py on the device): weight sets, at the fused configuration unet_input_dim = 32, dim_mults = (1, 2, 4), that
put the kernel's operands where the seed-0 weights never put them -- the static power-of-two scale of every conv B input and of the final
1x1 conv (csrc/unet.hip: static_act_scale, from B = max_c (max(0.31, 16 |gamma_c| + |beta_c|) + max_t |tb_c(t)|), always 2^6 at
B ~ 20), the clamp at 20 inside the Mish of csrc/gn_mish.h, the GroupNorm statistics on constant, beta-dominated and binade-spread
groups, per-column weight scales with all-zero rows -- the float64 / fp32 oracle forwards of each case, computed once and shared, and
the CPU emulation of the kernel's operand rounding: the oracle forward in float64 with every conv input and weight rounded to TWO fp16
pieces under the kernel's scales (accumulation stays in float64: a floor for the kernel, not a forecast), with switches for the mutants
the host test needs.  No GPU."""
import contextlib
import functools
import types

import numpy as np
import torch

from mmd_amd import synth
from oracle import mmd_oracle as O
import layered_edge_cases as L
from layered_edge_cases import accuracy_input, rel_err64, bound, SCALES, N_ACC      # noqa: F401  (shared with the layered tests)

UID, DM = 32, (1, 2, 4)
T_STEP, T_STEPS = 41, 100             # the step and the step count of test_unet_forward_accuracy_against_fp64
T_EDGE = 63                           # the step of tests/test_gpu_unet_scale_edges.py
RTBS = ["downs.0.0", "downs.0.1", "downs.1.0", "downs.1.1", "downs.2.0", "downs.2.1", "ups.0.0", "ups.0.1", "ups.1.0", "ups.1.1",
        "mid_block1", "mid_block2"]                                   # state_dict order, as csrc/unet.hip packs them
CONV_BLOCKS = [f"{r}.blocks.{i}" for r in RTBS for i in (0, 1)] + ["final_conv.0"]
LAYERED_SETS = ("colspread",) + L.CONTRAST_SETS
EMULATION_MARGIN = 2.0                # a kernel against the emulation of its own operand rounding (test_f16_mode_is_on_and_within_twice_its_emulation)


def _seed0():
    return synth.synth_unet_state_dict(0, unet_input_dim=UID, dim_mults=DM)


# ---- weight sets (all on seed 0)
def gamma_scaled_state_dict(k):
    """every GroupNorm gamma times 2^k: the pre-Mish values reach 2^k x |x_hat| (beyond the softplus threshold 20 from k = 3 on) and the
    static scale bound B grows by 2^k (the scale falls from 2^6 to 2^(6 - k))"""
    sd = _seed0()
    for key in sd:
        if key.endswith(".block.2.weight"):
            sd[key] = (sd[key] * np.float32(2.0 ** k)).astype(np.float32)
    return sd


def gamma_spread_state_dict():
    """gamma_c times 2^k(c), k an integer drawn from [-12, 0] per channel (both ends present in every GroupNorm): gammas spread over
    thirteen binades inside one group, channels whose affine output is all beta next to channels at full swing"""
    sd = _seed0()
    rng = np.random.Generator(np.random.PCG64(21))
    for key in sd:
        if key.endswith(".block.2.weight"):
            k = rng.integers(-12, 1, size=sd[key].shape[0])
            k[:2] = (0, -12)
            sd[key] = (sd[key] * np.exp2(rng.permutation(k).astype(np.float64))).astype(np.float32)
    return sd


def beta_shifted_state_dict(shift):
    """shift added to every GroupNorm beta.  -8: every Mish on its negative tail; +30 / +200: every pre-activation beyond the softplus
    threshold (Mish = identity) and B up to 221; -30: every pre-activation below -20, every activation ~ -3e-12 -- there the final
    Conv1dBlock keeps its seed-0 beta: with it shifted too, eps out is final_conv.1's bias to eleven digits whatever the rest of the
    network computes (the fp32 reference's error against float64: 6e-11) and no error made anywhere could show"""
    sd = _seed0()
    for key in sd:
        if key.endswith(".block.2.bias") and not (shift == -30 and key.startswith("final_conv.")):
            sd[key] = (sd[key] + np.float32(shift)).astype(np.float32)
    return sd


def time_bias_scaled_state_dict(k):
    """weight and bias of every cond_mlp.1 times 2^k: the time bias, which conv B's input carries unnormalised, dominates B (up to 1510
    at k = 12) and the static scale rests on time_bias_absmax's maximum over all steps"""
    sd = _seed0()
    for key in sd:
        if ".cond_mlp.1." in key:
            sd[key] = (sd[key] * np.float32(2.0 ** k)).astype(np.float32)
    return sd


def zero_variance_state_dict():
    """the first GroupNorm group of every Conv1dBlock (cout / 8 channels): conv weights 0 and equal biases, so that the group is one
    constant over channels and positions -- variance exactly 0, rstd = eps^-1/2 -- and its columns' weight scales take f16_scale_for's
    m = 0 branch"""
    sd = _seed0()
    for blk in CONV_BLOCKS:
        w, b = sd[f"{blk}.block.0.weight"].copy(), sd[f"{blk}.block.0.bias"].copy()
        cg = w.shape[0] // 8
        w[:cg] = 0.0
        b[:cg] = b[0]
        sd[f"{blk}.block.0.weight"], sd[f"{blk}.block.0.bias"] = w, b
    return sd


def in_spread_exponents(e):
    """{residual block: integer k(c) in [0, e] per channel of conv B's input, 0 and e both present}"""
    rng = np.random.Generator(np.random.PCG64(31))
    sd = _seed0()
    out = {}
    for r in RTBS:
        c = sd[f"{r}.blocks.0.block.2.weight"].shape[0]
        k = rng.integers(0, 21, size=c) * e // 20                    # (one stream for every e: the same channels are the small ones)
        k[:2] = (0, e)
        out[r] = rng.permutation(k)
    return out


def in_spread_state_dict(e):
    """per residual block: conv A's gamma_c, beta_c and the block's cond_mlp.1 row c times 2^-k(c), conv B's input channel c times
    2^k(c).  The channels of conv B's input then lie up to 2^e apart while every product keeps its size: the fp32 reference does not
    care, the kernel's ONE static scale per conv input does -- a channel's precision is relative to the largest channel's."""
    sd = _seed0()
    for r, k in in_spread_exponents(e).items():
        down, up = np.exp2(-k.astype(np.float64)), np.exp2(k.astype(np.float64))
        for key in (f"{r}.blocks.0.block.2.weight", f"{r}.blocks.0.block.2.bias", f"{r}.cond_mlp.1.bias"):
            sd[key] = (sd[key] * down).astype(np.float32)
        sd[f"{r}.cond_mlp.1.weight"] = (sd[f"{r}.cond_mlp.1.weight"] * down[:, None]).astype(np.float32)
        sd[f"{r}.blocks.1.block.0.weight"] = (sd[f"{r}.blocks.1.block.0.weight"] * up[None, :, None]).astype(np.float32)
    return sd


_BUILDERS = {
    "gamma_x8": lambda: gamma_scaled_state_dict(3), "gamma_x64": lambda: gamma_scaled_state_dict(6),
    "gamma_x1024": lambda: gamma_scaled_state_dict(10), "gamma_spread": gamma_spread_state_dict,
    "beta-8": lambda: beta_shifted_state_dict(-8), "beta-30": lambda: beta_shifted_state_dict(-30),
    "beta+30": lambda: beta_shifted_state_dict(30), "beta+200": lambda: beta_shifted_state_dict(200),
    "tb_x256": lambda: time_bias_scaled_state_dict(8), "tb_x4096": lambda: time_bias_scaled_state_dict(12),
    "zerovar": zero_variance_state_dict,
    "in_spread8": lambda: in_spread_state_dict(8), "in_spread12": lambda: in_spread_state_dict(12),
    "in_spread16": lambda: in_spread_state_dict(16), "in_spread20": lambda: in_spread_state_dict(20),
}
OUT_OF_RANGE = ("in_spread16", "in_spread20")
IN_RANGE = LAYERED_SETS + tuple(k for k in _BUILDERS if k not in OUT_OF_RANGE)
ALL_SETS = IN_RANGE + OUT_OF_RANGE


def state_dict(name):
    if name == "seed0":
        return _seed0()
    if name in LAYERED_SETS:
        return L.state_dict(name, UID, DM)
    return _BUILDERS[name]()


# ---- the host-chosen static scales, restated (csrc/unet.hip)
def time_bias_absmax(sd64, T):
    """{residual block: max over t = 0 .. T - 1 of |time bias| per channel} -- time_bias_absmax, in float64 through the oracle"""
    c = O.time_embedding(sd64, torch.arange(T, dtype=torch.float64))
    m = O.F.mish(c)
    return {r: O.F.linear(m, sd64[f"{r}.cond_mlp.1.weight"], sd64[f"{r}.cond_mlp.1.bias"]).abs().amax(dim=0) for r in RTBS}


def scale_bound(gamma, beta, tbmax):
    """B of static_act_scale, in its fp32 arithmetic"""
    g, b, tb = (np.asarray(v, dtype=np.float32) for v in (gamma, beta, tbmax))
    return float(np.max(np.maximum(np.float32(0.31), np.float32(16.0) * np.abs(g) + np.abs(b)) + tb * np.float32(1.001)))


def static_act_scale(gamma, beta, tbmax):
    """2^(10 - floor(log2 B)); 1 where B is not finite"""
    B = scale_bound(gamma, beta, tbmax)
    if not np.isfinite(B):
        return 1.0
    return float(2.0 ** (10 - (np.frexp(np.float32(B))[1] - 1)))


def scale_bounds(sd_np, T=T_STEPS):
    """{conv whose input has a static scale: B} -- blocks.1 of the twelve residual blocks and final_conv.1"""
    sd64 = {k: v.double() for k, v in O.state_dict_to_torch(sd_np).items()}
    tb = time_bias_absmax(sd64, T)
    out = {f"{r}.blocks.1": scale_bound(sd_np[f"{r}.blocks.0.block.2.weight"], sd_np[f"{r}.blocks.0.block.2.bias"], tb[r].numpy())
           for r in RTBS}
    out["final_conv.1"] = scale_bound(sd_np["final_conv.0.block.2.weight"], sd_np["final_conv.0.block.2.bias"], np.zeros(32))
    return out


# ---- the emulation
def _dyn_scale(x):
    """per sample 2^(10 - floor(log2 M)), M the sample's largest |x|, at most 2^73 (dyn_scale, csrc/f16x2.h); the exponent is read in
    float64 whatever x's type (a power of two: exact in either)"""
    m = x.abs().amax(dim=(1, 2), keepdim=True).double()
    m = torch.where(m > 0, m, torch.full_like(m, 2.0 ** -80))
    return torch.exp2(torch.clamp(10 - torch.floor(torch.log2(m)), max=73.0)).to(x.dtype)


def _col_scale(w, dims):
    """per output channel the power of two that puts its largest |w| into [2^14, 2^15); 1 for an all-zero one (f16_scale_for)"""
    m = w.abs().amax(dim=dims, keepdim=True).double()
    s = torch.where(m > 0, torch.exp2(14 - torch.floor(torch.log2(torch.where(m > 0, m, torch.ones_like(m))))), torch.ones_like(m))
    return s.to(w.dtype)


def _keep_bits(v, bits):
    """v rounded to `bits` significant bits (to nearest; 0, inf and NaN pass)"""
    m, e = torch.frexp(v)
    return torch.where(torch.isfinite(v), torch.ldexp(torch.round(torch.ldexp(m, torch.tensor(bits))), e - bits), v)


def _two_pieces(v, s, low_piece, bits=11):
    hi = (v * s).half().to(v.dtype)
    if bits != 11:            # ONE rounding of v s to `bits` bits (not a second one behind fp16's) wherever fp16 holds it as a normal number
        hi = torch.where(torch.isfinite(hi) & (hi.abs() >= 2.0 ** -14), _keep_bits(v * s, bits), hi)
    if not low_piece:
        return hi / s
    return (hi + (v * s - hi).half().to(v.dtype)) / s


def kernel_mish(y, clamp=True):
    """csrc/gn_mish.h: y n / (n + 2), n = e^y (e^y + 2), the exponent clamped at 20 (torch's softplus threshold)"""
    e = torch.exp(torch.clamp(y, max=20.0) if clamp else y)
    n = e * (e + 2)
    return y * (n / (n + 2))


@contextlib.contextmanager
def _oracle_functional(**swapped):
    real = O.F
    proxy = types.SimpleNamespace(**{k: getattr(real, k) for k in dir(real) if not k.startswith("__")})
    for k, v in swapped.items():
        setattr(proxy, k, v)
    O.F = proxy
    try:
        yield
    finally:
        O.F = real


def emulated_forward(sd_np, x, t, T=T_STEPS, low_piece=True, mish="torch", static_scale=None, dtype=torch.float64, operand_bits=11,
                     weight_scale="column"):
    """The float64 oracle forward with every conv's input and weight rounded to two fp16 pieces under the kernel's scales: the input per
    sample by dyn_scale, but for conv B of every residual block and final_conv.1, whose inputs carry static_act_scale; the weights
    per output channel (a ConvTranspose1d per output channel and parity, as its two packs).
    The mutants: low_piece=False drops the second piece of both operands; mish="kernel" restates Mish as gn_mish.h does,
    "kernel_noclamp" the same without the clamp at 20; static_scale=s uses the constant s wherever the packer computes one;
    operand_bits=b keeps b significant bits of the high piece where fp16 keeps 11; weight_scale="tensor" scales a weight by ONE power
    of two where the packer has one per output channel.  dtype=torch.float32: the same roundings under the same scales (they are
    powers of two, chosen in float64) with the state dict, the input and every operation of the forward in float32."""
    assert weight_scale in ("column", "tensor"), weight_scale
    sd64 = {k: v.double() for k, v in O.state_dict_to_torch(sd_np).items()}
    sd = sd64 if dtype == torch.float64 else {k: v.to(dtype) for k, v in sd64.items()}
    tb = time_bias_absmax(sd64, T)
    static = {}
    for r in RTBS:
        static[sd[f"{r}.blocks.1.block.0.weight"].data_ptr()] = static_act_scale(
            sd_np[f"{r}.blocks.0.block.2.weight"], sd_np[f"{r}.blocks.0.block.2.bias"], tb[r].numpy())
    static[sd["final_conv.1.weight"].data_ptr()] = static_act_scale(
        sd_np["final_conv.0.block.2.weight"], sd_np["final_conv.0.block.2.bias"], np.zeros(32))
    real = O.F

    def pieces(v, s):
        return _two_pieces(v, s, low_piece, operand_bits)

    def conv1d(x, w, *args, **kw):
        s = static.get(w.data_ptr())
        sx = _dyn_scale(x) if s is None else (s if static_scale is None else static_scale)
        return real.conv1d(pieces(x, sx), pieces(w, _col_scale(w, (1, 2) if weight_scale == "column" else (0, 1, 2))), *args, **kw)

    def conv_transpose1d(x, w, *args, **kw):                     # [cin, cout, 4]: taps (3, 1) make the even outputs, (2, 0) the odd ones
        sw = torch.empty_like(w)
        for taps in ((1, 3), (0, 2)):
            sw[:, :, taps] = _col_scale(w[:, :, taps], (0, 2) if weight_scale == "column" else (0, 1, 2)).expand(w.shape[0], w.shape[1], 2)
        return real.conv_transpose1d(pieces(x, _dyn_scale(x)), pieces(w, sw), *args, **kw)

    swapped = dict(conv1d=conv1d, conv_transpose1d=conv_transpose1d)
    if mish != "torch":
        assert mish in ("kernel", "kernel_noclamp"), mish
        swapped["mish"] = lambda y: kernel_mish(y, clamp=mish == "kernel") if y.ndim == 3 else real.mish(y)   # (the time MLP: mish_exact)
    with _oracle_functional(**swapped):
        return O.unet_forward(sd, x.to(dtype), torch.full((x.shape[0],), t, dtype=torch.long))


def traced_forward(sd_np, x, t):
    """the float64 oracle forward, with what every Conv1dBlock's GroupNorm reads and what its Mish reads, in CONV_BLOCKS order:
    (out, [GroupNorm inputs], [pre-Mish values])"""
    sd64 = {k: v.double() for k, v in O.state_dict_to_torch(sd_np).items()}
    real = O.F
    gn_in, pre = [], []

    def group_norm(x, *args, **kw):
        gn_in.append(x)
        return real.group_norm(x, *args, **kw)

    def mish(y):
        if y.ndim == 3:
            pre.append(y)
        return real.mish(y)

    with _oracle_functional(group_norm=group_norm, mish=mish):
        out = O.unet_forward(sd64, x.double(), torch.full((x.shape[0],), t, dtype=torch.long))
    assert len(gn_in) == len(pre) == len(CONV_BLOCKS)
    # O.unet_forward walks downs, mid, ups, final; CONV_BLOCKS lists the middle blocks last, as the packer does
    walk = [f"{r}.blocks.{i}" for r in RTBS[:6] + RTBS[10:] + RTBS[6:10] for i in (0, 1)] + ["final_conv.0"]
    order = [walk.index(b) for b in CONV_BLOCKS]
    return out, [gn_in[i] for i in order], [pre[i] for i in order]


# ---- references, computed once and never written to
@functools.lru_cache(maxsize=None)
def accuracy_reference(wset, scale):
    """(float64 oracle forward, fp32 oracle forward) of accuracy_input(scale) at T_STEP"""
    return L._forwards(state_dict(wset), accuracy_input(scale), T_STEP)


@functools.lru_cache(maxsize=None)
def emulated_reference(wset, scale):
    return emulated_forward(state_dict(wset), accuracy_input(scale), T_STEP)


def edge_rows():
    return L.edge_batch()[[L.NAMES.index(k) for k in L.FINITE_ROWS]]


@functools.lru_cache(maxsize=None)
def edge_reference():
    """the same two forwards of the nine finite rows of edge_batch() on the seed-0 weights at T_EDGE, [9, H, D]"""
    return L._forwards(_seed0(), edge_rows(), T_EDGE)


TIME_SET, TIME_T, TIME_N = "tb_x4096", 25, 3


def time_step_input():
    return torch.from_numpy(synth.synth_noise(303, (TIME_N, L.H, L.D)))


@functools.lru_cache(maxsize=None)
def time_step_reference(t):
    return L._forwards(state_dict(TIME_SET), time_step_input(), t)
