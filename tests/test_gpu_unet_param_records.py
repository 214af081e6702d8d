"""-m gpu: the fused UNet kernels read their epilogue constants from the packer's record tables (csrc/unet_kernel.h, rec_load; laid out by
csrc/unet.hip, push_records; tests/test_unet_param_records_host.py holds the tables to the state dict on the CPU).  Here the kernels
themselves, on the ramped weight set of tests/unet_record_cases.py -- every parameter array times a per-channel ramp of its own, so a
record read from the wrong channel unit or field changes the output -- at batches of 1, 2, 5 and 9 trajectories (a lone sample, a full
unet_kernel<2> workgroup, a full and a ragged unet_kernel<4> workgroup), at t = 0 and t = T - 1, through unet_kernel<1> (the launch as it
is), <4> (two_per_workgroup_max = -1) and <2> (one launch of 257: the rows + filler rows behind them), through the unguided step fused
into the launch's tail, the persistent run, and the f16 build of the same source: the same bits on every kernel, and the float64 bound of
test_unet_forward_accuracy_against_fp64.  The references are computed once, for the nine rows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmd_amd import _lib, synth                                               # noqa: E402
from mmd_amd.diffusion_model import GaussianDiffusionModel                    # noqa: E402
from mmd_amd.temporal_unet import TemporalUnet                                # noqa: E402
import fused_edge_cases as E                                                  # noqa: E402
import layered_edge_cases as L                                                # noqa: E402
import unet_record_cases as R                                                 # noqa: E402
from cases import H, D                                                        # noqa: E402

T = R.T_STEPS
BATCHES = (1, 2, 5, 9)
STEPS = (0, T - 1)
_UNETS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _unet(precision="f32", **options):
    key = (precision, tuple(sorted(options.items())))
    if key not in _UNETS:
        u = TemporalUnet(state_dim=4, n_support_points=H, unet_input_dim=R.UID, dim_mults=R.DM, precision=precision, **options)
        u.load_state_dict(R.ramped_state_dict())
        u.handle(T, "cuda")
        _UNETS[key] = u
    return _UNETS[key]


def _rows():
    return torch.from_numpy(synth.synth_noise(411, (9, H, D)))


@functools.lru_cache(maxsize=None)
def _references(t):
    """(float64 forward, fp32 forward) of the nine rows at step t -- computed once, never written to"""
    return L._forwards(R.ramped_state_dict(), _rows(), t)


@functools.lru_cache(maxsize=None)
def _one_piece_errors(t):
    """the one-piece emulation of the f16 build's operand rounding (float64 and float32 arithmetic) against the float64 forward, per
    batch size: what tests/f16_edge_cases.py calls sens"""
    ref64, _ = _references(t)
    emu = [E.emulated_forward(R.ramped_state_dict(), _rows(), t, T=T, low_piece=False, dtype=d) for d in (torch.float64, torch.float32)]
    return {n: max(E.rel_err64(e[:n], ref64[:n]) for e in emu) for n in BATCHES}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _forms(precision, x, t):
    """x [n, H, D] (cpu) through unet_kernel<1>, <4> and <2>, rows kept adjacent"""
    n = x.shape[0]
    filler = torch.from_numpy(synth.synth_noise(179, (257 - n, H, D)))
    one, four = _unet(precision), _unet(precision, two_per_workgroup_max=-1)
    return {1: one(x.cuda(), t).cpu(), 4: four(x.cuda(), t).cpu(), 2: one(torch.cat([x, filler]).cuda(), t).cpu()[:n]}


def test_block_size_is_the_host_packer_s():
    blob, tables = R.pack(R.ramped_state_dict())
    lib = _lib.load()
    for precision in ("f32", "f16"):
        assert lib.mmd_unet_weight_bytes(_unet(precision).handle(T, "cuda")) == 4 * blob.size, precision
    assert len(tables) == 30


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("n", BATCHES)
def test_f32_kernels_agree_and_meet_the_fp64_bound(n, t):
    ref64, ref32 = _references(t)
    outs = _forms("f32", _rows()[:n], t)
    assert torch.isfinite(outs[1]).all()
    for k in (2, 4):
        for i in range(n):
            assert same_bits(outs[1][i], outs[k][i]), (n, t, k, i)
    # ... and a row's bits do not depend on the batch it came in
    assert same_bits(outs[4], _forms("f32", _rows(), t)[4][:n]), (n, t)
    err_ref32, err_hip = E.rel_err64(ref32[:n], ref64[:n]), E.rel_err64(outs[1], ref64[:n])
    print(f"n={n} t={t}: err_hip {err_hip:.3g} err_ref32 {err_ref32:.3g} bound {E.bound(err_ref32):.3g}")
    assert err_hip < E.bound(err_ref32), (n, t, err_hip, err_ref32)


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("n", BATCHES)
def test_f16_kernels_agree_and_stay_within_their_limit(n, t):
    """the second build of the same source (csrc/unet_f16.hip): the three kernels agree bit for bit; against float64 the limit of
    tests/f16_edge_cases.py, max(bound(err_ref32), 2 x the one-piece emulation's error), made of references alone"""
    ref64, ref32 = _references(t)
    outs = _forms("f16", _rows()[:n], t)
    assert torch.isfinite(outs[1]).all()
    for k in (2, 4):
        for i in range(n):
            assert same_bits(outs[1][i], outs[k][i]), (n, t, k, i)
    err = E.rel_err64(outs[1], ref64[:n])
    limit = max(E.bound(E.rel_err64(ref32[:n], ref64[:n])), E.EMULATION_MARGIN * _one_piece_errors(t)[n])
    print(f"f16 n={n} t={t}: err {err:.3g} limit {limit:.3g}")
    assert err <= limit, (n, t, err, limit)
    assert not same_bits(outs[1], _forms("f32", _rows()[:n], t)[1])            # (the f16 kernels did run)


# ---- the unguided step in the launch's tail, the persistent run
LOOPS = {"fused": 0, "step_kernel": _lib.SAMPLER_NO_FUSED_STEP, "persist": _lib.SAMPLER_PERSIST}


def _chain(precision, options, n, flags):
    """mmd_p_sample_loop over all T steps (t = T - 1 .. 0) from the first n rows, injected noise: the chain [T + 1, n, H, D]"""
    model = GaussianDiffusionModel(model=_unet(precision, **options), variance_schedule="exponential", n_diffusion_steps=T,
                                   predict_epsilon=True)
    x = _rows()[:n]
    z = torch.from_numpy(synth.synth_noise(412, (T, 9, H, D)))[:, :n].contiguous()
    hc = {0: x[0, 0].clone(), H - 1: x[0, H - 1].clone()}
    model.sampler_flags = flags
    _, chain = model.p_sample_loop((n, H, D), hc, T, return_chain=True, warm_start_path_b=x.cuda(), n_robots=1, seed=5, step_noise=z.cuda())
    return chain.transpose(0, 1).contiguous().cpu()


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("n", BATCHES)
def test_fused_tail_and_persistent_run_follow_the_step_kernel_path(n, precision):
    """every step's forward feeds the next: one wrong epilogue constant in the tail-fused or the persistent kernel moves the chain off the
    one made of separate UNet and step-kernel launches.  unet_kernel<1> / unet_persist_kernel<2> (the launch as it is) and <4>
    (two_per_workgroup_max = -1)."""
    for options in ({}, dict(two_per_workgroup_max=-1)):
        want = _chain(precision, options, n, LOOPS["step_kernel"])
        assert torch.isfinite(want).all() and not same_bits(want[0], want[-1])
        for path in ("fused", "persist"):
            assert same_bits(_chain(precision, options, n, LOOPS[path]), want), (n, precision, options, path)
    # the same rows whatever the kernel form
    assert same_bits(_chain(precision, {}, n, 0), _chain(precision, dict(two_per_workgroup_max=-1), n, 0)), (n, precision)


def test_fused_tail_of_unet_kernel_2():
    """a launch of 257 (the smallest unet_kernel<2> runs at): its first nine rows are the nine-row chain's"""
    x = torch.cat([_rows(), torch.from_numpy(synth.synth_noise(179, (248, H, D)))])
    z = torch.cat([torch.from_numpy(synth.synth_noise(412, (T, 9, H, D))), torch.from_numpy(synth.synth_noise(413, (T, 248, H, D)))], dim=1)
    hc = {0: x[0, 0].clone(), H - 1: x[0, H - 1].clone()}
    for precision in ("f32", "f16"):
        model = GaussianDiffusionModel(model=_unet(precision), variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True)
        _, chain = model.p_sample_loop((257, H, D), hc, T, return_chain=True, warm_start_path_b=x.cuda(), n_robots=1, seed=5,
                                       step_noise=z.contiguous().cuda())
        assert same_bits(chain.transpose(0, 1)[:, :9].cpu(), _chain(precision, {}, 9, 0)), precision
