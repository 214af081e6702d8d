"""References and limits for the edge tests of TemporalUnet(precision="f16") (tests/test_f16_edges_host.py on the CPU,
tests/test_gpu_f16_edges.py on the device): on the weight sets, edge rows and time steps of tests/fused_edge_cases.py the ONE-piece
emulation of the fused kernel's operand rounding (fused_edge_cases.emulated_forward(low_piece=False): every conv input and weight rounded
once to fp16 under the packer's true scales), once with float64 arithmetic and once with the state dict, the input and every operation
in float32, each computed once and shared; and the limit the f16 build is held to.

A case is ("set", wset, scale), ("row", name of a finite edge row) or ("t", time step of the time-bias set).
    sens(case)       the larger of the two emulations' relative L2 errors against the float64 forward
    f16_limit(case)  max(bound(err_ref32), EMULATION_MARGIN x sens): below fused_edge_cases.bound the f32 build's own limit applies
Both are made of references alone; nothing the device computes enters them.  No GPU."""
import functools

import torch

import fused_edge_cases as E
import layered_edge_cases as L

ARITHMETICS = (torch.float64, torch.float32)


# ---- the two one-piece emulations, computed once and never written to
@functools.lru_cache(maxsize=None)
def one_piece_reference(wset, scale, dtype=torch.float64):
    """accuracy_input(scale) at T_STEP through the one-piece emulation of `wset`, arithmetic in `dtype`"""
    return E.emulated_forward(E.state_dict(wset), E.accuracy_input(scale), E.T_STEP, low_piece=False, dtype=dtype)


def one_piece_reference32(wset, scale):
    """the fp32-arithmetic twin: the same operand rounding under the same scales, nothing in float64"""
    return one_piece_reference(wset, scale, torch.float32)


@functools.lru_cache(maxsize=None)
def one_piece_edge_reference(dtype=torch.float64):
    """the nine finite rows of edge_batch() on the seed-0 weights at T_EDGE, [9, H, D]"""
    return E.emulated_forward(E.state_dict("seed0"), E.edge_rows(), E.T_EDGE, low_piece=False, dtype=dtype)


@functools.lru_cache(maxsize=None)
def one_piece_time_step_reference(t, dtype=torch.float64):
    """time_step_input() on the time-bias set at step t of TIME_T"""
    return E.emulated_forward(E.state_dict(E.TIME_SET), E.time_step_input(), t, T=E.TIME_T, low_piece=False, dtype=dtype)


# ---- cases
SET_CASES = tuple(("set", wset, scale) for wset in E.ALL_SETS for scale in E.SCALES)
ROW_CASES = tuple(("row", name) for name in L.FINITE_ROWS)
TIME_CASES = tuple(("t", t) for t in range(E.TIME_T))
ALL_CASES = SET_CASES + ROW_CASES + TIME_CASES


def case_name(case):
    return {"set": lambda: f"{case[1]} scale={case[2]:g}", "row": lambda: f"row {case[1]}", "t": lambda: f"t{case[1]}"}[case[0]]()


def references(case):
    """(float64 forward, fp32 forward, one-piece emulation in float64, one-piece emulation in float32) of the case"""
    if case[0] == "set":
        return E.accuracy_reference(*case[1:]) + tuple(one_piece_reference(*case[1:], dtype=d) for d in ARITHMETICS)
    if case[0] == "row":
        j = L.FINITE_ROWS.index(case[1])
        return tuple(v[j] for v in E.edge_reference() + tuple(one_piece_edge_reference(d) for d in ARITHMETICS))
    assert case[0] == "t", case
    return E.time_step_reference(case[1]) + tuple(one_piece_time_step_reference(case[1], d) for d in ARITHMETICS)


def err_against_fp64(out, case):
    return E.rel_err64(out, references(case)[0])


@functools.lru_cache(maxsize=None)
def reference_errors(case):
    """(err_ref32, err of the float64-arithmetic emulation, err of the float32-arithmetic one) against the float64 forward; inf for
    an emulation that is not finite"""
    ref64, ref32, emu64, emu32 = references(case)
    return (E.rel_err64(ref32, ref64),) + tuple(E.rel_err64(v, ref64) if torch.isfinite(v).all() else float("inf") for v in (emu64, emu32))


def sens(case):
    return max(reference_errors(case)[1:])


def f16_limit(case):
    return max(E.bound(reference_errors(case)[0]), E.EMULATION_MARGIN * sens(case))
