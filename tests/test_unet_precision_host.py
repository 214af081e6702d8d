"""No GPU: the host side of TemporalUnet's opt-in fp16 precision (mmd_unet_options.precision, ABI v9) -- the options struct, the argument
checks of mmd_unet_create (they return before any device call) and the CPU emulation of the mode that tests/test_gpu_unet_f16.py holds
the kernels against: the oracle forward in float64 with every conv's input and weight rounded to ONE fp16 value under power-of-two
scales, as the kernels round them."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest
import torch

from mmd_amd import _lib, synth
from mmd_amd.temporal_unet import TemporalUnet
from oracle import mmd_oracle as O


# ---- the emulation ------------------------------------------------------------------------------------------------------------
def _pow2_scale_to(m, top):
    """power of two s with m * s in [2^(top - 1), 2^top) (1 where m is 0)"""
    m = torch.where(m > 0, m, torch.ones_like(m))
    return torch.exp2(top - 1 - torch.floor(torch.log2(m)))


def _round_f16(v, s):
    return (v * s).half().to(v.dtype) / s


def _emulated(fn, transposed):
    def conv(x, w, *args, **kw):
        sx = _pow2_scale_to(x.abs().amax(dim=(1, 2), keepdim=True), 11)          # per sample: below 2048 (the kernels' dyn_scale)
        out_dim = 1 if transposed else 0                                          # ConvTranspose1d weights are [cin, cout, k]
        sw = _pow2_scale_to(w.abs().amax(dim=tuple(d for d in range(3) if d != out_dim), keepdim=True), 15)   # per output channel: [2^14, 2^15)
        return fn(_round_f16(x, sx), _round_f16(w, sw), *args, **kw)
    return conv


@contextlib.contextmanager
def f16_operand_rounding():
    """Inside: the oracle's convs (F.conv1d / F.conv_transpose1d as the oracle module sees them) round input and weight through .half()."""
    real = O.F
    proxy = types.SimpleNamespace(**{k: getattr(real, k) for k in dir(real) if not k.startswith("__")})
    proxy.conv1d = _emulated(real.conv1d, False)
    proxy.conv_transpose1d = _emulated(real.conv_transpose1d, True)
    O.F = proxy
    try:
        yield
    finally:
        O.F = real


def f16_emulated_forward(sd64, x64, t):
    with f16_operand_rounding():
        return O.unet_forward(sd64, x64, t)


def rel64(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_options_struct_has_precision_last():
    assert _lib.ABI_VERSION == 9
    assert _lib.UnetOptions._fields_[-1][0] == "precision" and [f[0] for f in _lib.UnetOptions._fields_[:4]] == \
        ["flags", "rtb_fused", "mconv_max_cs", "two_per_workgroup_max"]
    assert C.sizeof(_lib.UnetOptions) == 16 + 4 and _lib.UnetOptions.precision.offset == 16
    assert _lib.UnetOptions(0, -1, 0, 0).precision == 0           # the four-field form keeps meaning f32
    assert (_lib.UNET_PRECISION_F32, _lib.UNET_PRECISION_F16) == (0, 1)


def test_temporal_unet_precision_argument():
    assert TemporalUnet().precision == "f32" and TemporalUnet().options[-1] == 0
    u = TemporalUnet(precision="f16")
    assert u.precision == "f16" and u.options[-1] == 1 and u.options != TemporalUnet().options     # (part of the device-model key)
    for bad in ("bf16", "fp16", 1, None):
        with pytest.raises(ValueError, match="precision"):
            TemporalUnet(precision=bad)


def test_planners_pass_the_precision_on():
    import inspect
    from mmd_amd import planners
    for f in (planners._load_model, planners.MPD.__init__, planners.MPDEnsemble.__init__):
        assert inspect.signature(f).parameters["unet_precision"].default == "f32"
    sd = synth.synth_unet_state_dict(0)
    assert planners._load_model("", "", sd, None, "cpu")[0].model.precision == "f32"
    assert planners._load_model("", "", sd, None, "cpu", "f16")[0].model.precision == "f16"
    assert planners._load_model("", "", sd, dict(unet_precision="f16"), "cpu")[0].model.precision == "f16"
    with pytest.raises(ValueError, match="precision"):
        planners._load_model("", "", sd, dict(unet_precision="bf16"), "cpu")


def _create(opt, dim_mults=(1, 2, 4)):
    lib = _lib.load()
    sd = synth.synth_unet_state_dict(0, dim_mults=dim_mults)
    vals = [np.ascontiguousarray(v, dtype=np.float32) for v in sd.values()]
    n = len(vals)
    assert n == lib.mmd_unet_num_tensors(32, len(dim_mults))
    ptrs = (C.c_void_p * n)(*[v.ctypes.data for v in vals])
    numels = (C.c_int64 * n)(*[v.size for v in vals])
    h = C.c_void_p()
    rc = lib.mmd_unet_create(C.byref(h), 32, len(dim_mults), 25, ptrs, numels, n, C.byref(opt), None)
    return rc, lib.mmd_last_error().decode(), h


def test_create_rejects_bad_precision_before_any_device_call():
    for opt, mults in ((_lib.UnetOptions(0, -1, 0, 0, 7), (1, 2, 4)),
                       (_lib.UnetOptions(0, -1, 0, 0, -1), (1, 2, 4)),
                       (_lib.UnetOptions(0, -1, 0, 0, 1), (1, 2, 4, 8)),
                       (_lib.UnetOptions(_lib.UNET_LAYERED, -1, 0, 0, 1), (1, 2, 4))):
        rc, err, h = _create(opt, mults)
        assert rc != 0 and "precision" in err and not h.value, (opt.precision, mults, rc, err)
    assert "MMD_UNET_PRECISION_F16" in _create(_lib.UnetOptions(0, -1, 0, 0, 1), (1, 2, 4, 8))[1]
    lib = _lib.load()
    assert lib.mmd_unet_precision(None) == -1


def test_f16_emulation_rounds_what_it_should():
    """The helper against the plain float64 forward: one fp16 rounding (2^-11 relative, uniform: rms 2^-11 / sqrt 3 = 2.8e-4 per operand)
    of every conv's input and weight across the network's 27 convs lands near 1e-3; below 2e-4 it rounds nothing, above 1e-2 it rounds
    wrongly (a missing scale: overflow or fp16 denormals)."""
    sd64 = {k: v.double() for k, v in O.state_dict_to_torch(synth.synth_unet_state_dict(0)).items()}
    x = torch.from_numpy(synth.synth_noise(300, (16, 64, 4))).double()
    t = torch.full((16,), 41, dtype=torch.long)
    ref = O.unet_forward(sd64, x, t)
    emu = f16_emulated_forward(sd64, x, t)
    d = rel64(emu, ref)
    print(f"f16 emulation vs float64: rel-L2 {d:.3e}")
    assert 2e-4 <= d <= 1e-2, d
    assert O.F is torch.nn.functional and torch.equal(O.unet_forward(sd64, x, t), ref)      # the wrapper is gone afterwards
    # the scales are powers of two that put the maxima where the kernels put them
    m = torch.tensor([3.0, 0.0, 1e-9, 2047.9])
    assert torch.equal(_pow2_scale_to(m, 11) * torch.tensor([3.0, 1.0, 1e-9, 2047.9]) // 1024, torch.ones(4))
