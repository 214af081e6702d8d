"""Shared by tests/test_unet_param_records_host.py (CPU) and tests/test_gpu_unet_param_records.py (device): the ramped weight set, the
fused kernel's packed block as the host builds it (mmd_debug_unet_pack, include/mmd_amd_debug.h) with the directory of its parameter-record
tables, and what every field of every record has to hold, restated in numpy from the state dict.  No GPU."""
import ctypes as C
import functools

import numpy as np

from mmd_amd import _lib, synth
from mmd_amd.unet_spec import unet_param_spec
import fused_edge_cases as E

UID, DM, T_STEPS = E.UID, E.DM, 25
# the packer's block names (state_dict order) and what the fused kernel's stage bodies make of them: channels per record (the lane's
# adjacent pair; ups.0: one channel per lane), first block of a stage (its conv A record carries the 1x1 residual conv's fields)
BLOCKS = dict(zip(("d00", "d01", "d10", "d11", "d20", "d21", "u00", "u01", "u10", "u11", "mid1", "mid2"), E.RTBS))
CPR = {b: 1 if b in ("u00", "u01") else 2 for b in BLOCKS}
FIRST = ("d00", "d10", "d20", "u00", "u10")
EPI, EPI_RES, TAIL_DOWN, TAIL_UP, OUT = range(5)                   # MMD_UNET_REC_*


class RecordTable(C.Structure):                                    # mmd_unet_record_table
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("kind", C.c_int32), ("channels", C.c_int32),
                ("channels_per_record", C.c_int32), ("n_fields", C.c_int32), ("record_floats", C.c_int32), ("reserved", C.c_int32)]


@functools.lru_cache(maxsize=None)
def ramped_state_dict():
    """synth seed 0 with EVERY parameter array times a per-channel ramp of its own (array j of the state dict: lo_j .. hi_j, linear over
    the output channels): no two channels of an array and no two arrays share a factor, so a record read from the wrong channel unit or
    the wrong field gives other numbers.  Vectors: factors within [0.6, 1.7]; weight matrices: [0.45, 1.9], more than a factor two
    from end to end, so the power-of-two weight scales differ across the channels of every conv.  The network remains an ordinary one
    for the float64 bound."""
    sd = synth.synth_unet_state_dict(0, unet_input_dim=UID, dim_mults=DM)
    for j, (k, v) in enumerate(sd.items()):
        axis = 1 if k.startswith("ups.") and k.endswith(".4.conv.weight") else 0      # ConvTranspose1d: [in, out, k]
        n = v.shape[axis]
        lo, hi = (0.6 + 0.002 * j, 1.7 - 0.003 * j) if v.ndim == 1 else (0.45 + 0.001 * j, 1.9 - 0.002 * j)
        ramp = (lo + (hi - lo) * np.arange(n) / max(n - 1, 1)).astype(np.float32)
        shape = [1] * v.ndim
        shape[axis] = n
        sd[k] = (v * ramp.reshape(shape)).astype(np.float32)
    return sd


def pack(sd, T=T_STEPS):
    """(blob float32 [n], {table name: RecordTable}) of the host packer"""
    lib = _lib.load()
    spec = unet_param_spec(4, UID, DM)
    arrs = [np.ascontiguousarray(sd[k], dtype=np.float32) for k in spec]
    n = len(arrs)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    numels = (C.c_int64 * n)(*[a.size for a in arrs])
    nf, nt = C.c_size_t(), C.c_int()
    _lib.check(lib.mmd_debug_unet_pack(UID, len(DM), T, ptrs, numels, n, None, 0, C.byref(nf), None, 0, C.byref(nt)))
    blob = np.full(nf.value, np.nan, dtype=np.float32)
    tables = (RecordTable * nt.value)()
    nf2, nt2 = C.c_size_t(), C.c_int()
    _lib.check(lib.mmd_debug_unet_pack(UID, len(DM), T, ptrs, numels, n, blob.ctypes.data, blob.size, C.byref(nf2), tables, nt.value,
                                       C.byref(nt2)))
    assert (nf2.value, nt2.value) == (nf.value, nt.value)
    return blob, {t.name.decode(): t for t in tables}


def inverse_scale(w, axes, in_scale=1.0):
    """1 / (f16_scale_for(max |w| over `axes`) x in_scale) per output channel (csrc/f16x2.h): the power of two that puts the channel's
    largest weight into [2^14, 2^15), 1 for an all-zero channel"""
    m = np.abs(np.asarray(w, np.float32)).max(axis=axes)
    ex = np.frexp(m)[1]
    sc = np.where((m > 0) & np.isfinite(m), np.exp2((15 - ex).astype(np.float64)), 1.0)
    return (1.0 / (sc * in_scale)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _tbmax(T):
    import torch  # noqa: F401
    from oracle import mmd_oracle as O
    sd64 = {k: v.double() for k, v in O.state_dict_to_torch(ramped_state_dict()).items()}
    return {r: v.numpy() for r, v in E.time_bias_absmax(sd64, T).items()}


def expected_fields(sd, T=T_STEPS):
    """{table name: (kind, channels per record, [field arrays [C]])}: every record table the packer has to write, from the state dict"""
    assert sd is ramped_state_dict()                               # (_tbmax is computed for it)
    tb = _tbmax(T)
    out = {}
    for b, r in BLOCKS.items():
        ka, kb = f"{r}.blocks.0", f"{r}.blocks.1"
        fa = [sd[f"{ka}.block.0.bias"], sd[f"{ka}.block.2.weight"], sd[f"{ka}.block.2.bias"], inverse_scale(sd[f"{ka}.block.0.weight"], (1, 2))]
        if b in FIRST:
            fa += [sd[f"{r}.residual_conv.bias"], inverse_scale(sd[f"{r}.residual_conv.weight"], (1, 2))]
        out[f"{b}.a"] = (EPI_RES if b in FIRST else EPI, CPR[b], fa)
        act = E.static_act_scale(sd[f"{ka}.block.2.weight"], sd[f"{ka}.block.2.bias"], tb[r])
        out[f"{b}.b"] = (EPI, CPR[b], [sd[f"{kb}.block.0.bias"], sd[f"{kb}.block.2.weight"], sd[f"{kb}.block.2.bias"],
                                       inverse_scale(sd[f"{kb}.block.0.weight"], (1, 2), act)])
    for i in range(2):
        out[f"down{i}"] = (TAIL_DOWN, 2, [sd[f"downs.{i}.4.conv.bias"], inverse_scale(sd[f"downs.{i}.4.conv.weight"], (1, 2))])
        w = sd[f"ups.{i}.4.conv.weight"]                           # [in, out, 4]: taps (3, 1) make the even outputs, (2, 0) the odd ones
        out[f"up{i}"] = (TAIL_UP, 2 if i == 1 else 1, [sd[f"ups.{i}.4.conv.bias"], inverse_scale(w[:, :, [3, 1]], (0, 2)),
                                                       inverse_scale(w[:, :, [2, 0]], (0, 2))])
    out["final"] = (EPI, 2, [sd["final_conv.0.block.0.bias"], sd["final_conv.0.block.2.weight"], sd["final_conv.0.block.2.bias"],
                             inverse_scale(sd["final_conv.0.block.0.weight"], (1, 2))])
    act = E.static_act_scale(sd["final_conv.0.block.2.weight"], sd["final_conv.0.block.2.bias"], np.zeros(32, np.float32))
    out["final.out"] = (OUT, 1, [sd["final_conv.1.bias"], inverse_scale(sd["final_conv.1.weight"], (1, 2), act)])
    return out


def read_field(blob, t, f):
    """field f of every channel of table t, as the kernels address it: blob[offset + (c / cpr) * record_floats + f * cpr + c % cpr]"""
    c = np.arange(t.channels)
    cpr = t.channels_per_record
    return blob[t.offset + (c // cpr) * t.record_floats + f * cpr + c % cpr]
