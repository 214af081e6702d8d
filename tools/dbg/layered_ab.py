"""A/B of the layer-by-layer TemporalUnet forward (csrc/unet_layers.hip, mconv_dev.h, layers_valu_dev.h) against another build of the
library, needs one GPU:

    python tools/dbg/layered_ab.py OTHER.so COPY_OF_OTHER.so [--no-time] [--no-results] [--new-first]       results, then time
    python tools/dbg/layered_ab.py --trace SOME.so                             the forwards whose launches are compared (run it under
                                                                               rocprofv3 --kernel-trace -f csv, once per side)
    python tools/dbg/layered_ab.py --compare-traces A_kernel_trace.csv B_kernel_trace.csv

Three libraries in ONE process: OTHER.so ("parent"), a second copy of that file under another name (its own dlopen handle: the
parent/parent yardstick of the session's spread) and this tree's.  Every library gets its own device model through the C entry points
(mmd_unet_create), all of them read the same input and use the same workspace.
RESULTS: eps word for word, every library against parentA, and mmd_unet_weight_bytes -- the networks (unet_input_dim, levels) (32, 4),
(32, 3 layered), (64, 4), (16, 1), (8, 2), (40, 3), (56, 2) and on (32, 4) rtb_fused = 0, layered_valu, mconv_max_cs = 32, each at n = 1, 13,
191, 192, 767, 768, 769, 1536, 3100.  Any difference exits 1.
LAUNCHES: equal bits do not show an unchanged launch rule (the bits do not depend on the slicing by design), so --trace runs two forwards
of (32, 4), (64, 4), (40, 3) at n = 64, 768, 3100 on ONE library, and --compare-traces holds the two runs' sequences of (kernel, grid,
workgroup, LDS bytes) of the layer kernels against each other; exits 1 unless they are equal.
TIME: option 1 = (32, 4), option 0 layered = (32, 3 layered) and (40, 3) at n = 64, 256, 1024, 4096: two HIP events around 200 forwards after
a warm-up, the three sides alternating with the order rotated, five repetitions.  Per line: median of the parent's ten figures, their
spread (largest - smallest), the median of the new side's five; gate: new median - parent median <= spread.  Beside it the host's own
time to issue a forward (the calls return before the GPU is done): where it is close to the events' figure the line measures the host."""
import csv
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mmd_amd import _lib, synth                                           # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet                             # noqa: E402

H, D, T, T_ROW = 64, 4, 25, 7
ARGS = [v for v in sys.argv[1:] if not v.startswith("--")]
LAYER_KERNELS = ("mconv_kernel", "conv5_block_kernel", "conv_plain_kernel")


def say(s):
    print(s, flush=True)


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in list(_lib._SIGNATURES.items()) + list(_lib._DEBUG_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.mmd_abi_version() == _lib.ABI_VERSION
    return lib


class Model:
    """one device model of one library: (unet_input_dim, levels, TemporalUnet options) on synthetic weights"""
    def __init__(self, lib, uid, levels, **options):
        u = TemporalUnet(unet_input_dim=uid, dim_mults=(1, 2, 4, 8)[:levels], **options)
        u.load_state_dict(synth.synth_unet_state_dict(0, unet_input_dim=uid, dim_mults=u.dim_mults))
        sd = list(u._sd.values())
        ptrs = (C.c_void_p * len(sd))(*[v.ctypes.data for v in sd])
        numels = (C.c_int64 * len(sd))(*[v.size for v in sd])
        self.lib, self.h = lib, C.c_void_p()
        opt = _lib.UnetOptions(*u.options)
        rc = lib.mmd_unet_create(C.byref(self.h), uid, levels, T, ptrs, numels, len(sd), C.byref(opt), _lib.current_stream_ptr())
        assert rc == 0, lib.mmd_last_error().decode()

    def forward(self, x, out, ws):
        rc = self.lib.mmd_unet_forward(self.h, x.data_ptr(), T_ROW, out.data_ptr(), x.shape[0], ws.data_ptr(), ws.numel(), _lib.current_stream_ptr())
        assert rc == 0, self.lib.mmd_last_error().decode()

    def close(self):
        self.lib.mmd_unet_destroy(self.h)


def workspace(models, n):
    return torch.empty(max(m.lib.mmd_unet_workspace_bytes(m.h, n) for m in models), dtype=torch.uint8, device="cuda")


RESULT_NETS = [((32, 4), {}), ((32, 3), dict(layered=True)), ((64, 4), {}), ((16, 1), {}), ((8, 2), {}), ((40, 3), {}), ((56, 2), {}),
               ((32, 4), dict(rtb_fused=0)), ((32, 4), dict(layered_valu=True)), ((32, 4), dict(mconv_max_cs=32))]
RESULT_NS = (1, 13, 191, 192, 767, 768, 769, 1536, 3100)
TRACE_NETS, TRACE_NS = ((32, 4), (64, 4), (40, 3)), (64, 768, 3100)
TIME_NETS = [("option 1 (32, 4 levels)", (32, 4), {}), ("option 0 layered (32, 3 levels)", (32, 3), dict(layered=True)), ("(40, 3 levels)", (40, 3), {})]
TIME_NS = (64, 256, 1024, 4096)


def results(libs):
    x = (torch.from_numpy(synth.synth_noise(909, (max(RESULT_NS), H, D))) * 0.7).cuda()
    differ = 0
    for (uid, levels), options in RESULT_NETS:
        models = {name: Model(lib, uid, levels, **options) for name, lib in libs.items()}
        wb = {name: m.lib.mmd_unet_weight_bytes(m.h) for name, m in models.items()}
        bad = [] if len(set(wb.values())) == 1 else [f"weight bytes {wb}"]
        for n in RESULT_NS:
            xn, ws = x[:n].contiguous(), workspace(models.values(), n)
            outs = {}
            for name, m in models.items():
                outs[name] = torch.full((n, H, D), float("nan"), device="cuda")
                m.forward(xn, outs[name], ws)
            torch.cuda.synchronize()
            assert torch.isfinite(outs["parentA"]).all(), (uid, levels, options, n)
            bad += [f"n={n}: {name} differs from parentA" for name in outs if not torch.equal(outs[name].view(torch.int32), outs["parentA"].view(torch.int32))]
        differ += len(bad)
        say(f"({uid}, {levels} levels) {options or ''}: weight bytes {wb['new']}; n = {', '.join(map(str, RESULT_NS))}: "
            + ("eps equal word for word in every library" if not bad else "DIFFERENT: " + "; ".join(bad)))
        for m in models.values():
            m.close()
    say(f"# => results: {differ} differences")
    return differ


def timing(libs, reps=5, forwards=200):
    names = list(libs)
    say(f"# us per forward: two HIP events around {forwards} forwards, sides alternating, {reps} repetitions; spread = largest - smallest of the "
        "parent's ten figures; gate: new median - parent median <= spread")
    say(f"{'figure':42s} | parent median  spread  |med A - med B|  new median  new - parent")
    outside = 0
    for label, (uid, levels), options in TIME_NETS:
        models = {name: Model(lib, uid, levels, **options) for name, lib in libs.items()}
        for n in TIME_NS:
            x = torch.randn(n, H, D, device="cuda")
            out, ws = torch.empty_like(x), workspace(models.values(), n)
            for m in models.values():
                for _ in range(10):
                    m.forward(x, out, ws)
            torch.cuda.synchronize()
            figs, host = {name: [] for name in names}, {name: [] for name in names}
            for rep in range(reps):
                for name in names[rep % 3:] + names[:rep % 3]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    t0 = time.perf_counter()
                    for _ in range(forwards):
                        models[name].forward(x, out, ws)
                    host[name].append(1e6 * (time.perf_counter() - t0) / forwards)
                    e1.record()
                    torch.cuda.synchronize()
                    figs[name].append(1e3 * e0.elapsed_time(e1) / forwards)
            ten = figs["parentA"] + figs["parentB"]
            pm, spread, nm = float(np.median(ten)), max(ten) - min(ten), float(np.median(figs["new"]))
            ab = abs(float(np.median(figs["parentA"])) - float(np.median(figs["parentB"])))
            ok = nm - pm <= spread
            outside += 0 if ok else 1
            say(f"{label + ' n=%d' % n:42s} | {pm:13.1f} {spread:7.1f} {ab:15.1f} {nm:11.1f} {nm - pm:+12.1f}  {'ok' if ok else 'OUTSIDE'}"
                f"   A {' '.join('%.1f' % v for v in figs['parentA'])} | B {' '.join('%.1f' % v for v in figs['parentB'])} | new {' '.join('%.1f' % v for v in figs['new'])}"
                f" | the host's time to issue a forward (median): " + " ".join(f"{k} {np.median(v):.1f}" for k, v in host.items()))
        for m in models.values():
            m.close()
    say(f"# => figures outside the spread: {outside} of {len(TIME_NETS) * len(TIME_NS)}")
    return outside


def trace(path):
    lib = load(path)
    for uid, levels in TRACE_NETS:
        m = Model(lib, uid, levels)
        for n in TRACE_NS:
            x = torch.randn(n, H, D, device="cuda")
            out, ws = torch.empty_like(x), workspace([m], n)
            for _ in range(2):
                m.forward(x, out, ws)
            torch.cuda.synchronize()
        m.close()
    say(f"{path}: {len(TRACE_NETS)} networks x n = {TRACE_NS} x 2 forwards")


def launches(path):
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in LAYER_KERNELS)]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = [k for k in (rows[0] if rows else {}) if k.startswith("LDS")]          # LDS_Block_Size
    assert not rows or len(lds) == 1, f"{path}: no LDS column among {list(rows[0])}"
    return [(r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Workgroup_Size_X"]), int(r[lds[0]])) for r in rows]


def compare_traces(a, b):
    la, lb = launches(a), launches(b)
    say(f"{a}: {len(la)} layer-kernel launches, {len(set(la))} distinct (kernel, grid, workgroup, LDS bytes); {b}: {len(lb)}, {len(set(lb))}")
    first = next((i for i, (p, q) in enumerate(zip(la, lb)) if p != q), None)
    if first is None and len(la) == len(lb) and la:
        say("# => launches: the two sequences are equal")
        return 0
    say(f"# => launches DIFFER at launch {first if first is not None else min(len(la), len(lb))}: {la[first] if first is not None else None} | {lb[first] if first is not None else None}")
    return 1


if __name__ == "__main__":
    if "--compare-traces" in sys.argv and len(ARGS) == 2:
        sys.exit(compare_traces(*ARGS))
    if "--trace" in sys.argv and len(ARGS) == 1:
        sys.exit(trace(ARGS[0]))
    if len(ARGS) != 2:
        sys.exit(__doc__)
    # (--new-first: this tree's library is loaded, and takes its turn, ahead of the parent's two: figures a microsecond apart follow the
    # order in which identical libraries were loaded -- parentB against parentA shows by how much)
    order = ("new", "parentA", "parentB") if "--new-first" in sys.argv else ("parentA", "parentB", "new")
    LIBS = {name: load({"parentA": ARGS[0], "parentB": ARGS[1], "new": _lib.LIB_PATH}[name]) for name in order}
    say(f"# device: {torch.cuda.get_device_name(0)}; libraries loaded in the order {', '.join(order)}")
    bad = 0 if "--no-results" in sys.argv else results(LIBS)
    if "--no-time" not in sys.argv:
        bad += timing(LIBS)
    sys.exit(1 if bad else 0)
