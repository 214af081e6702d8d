"""One sampler step as the kernels write it, restated in numpy: the DDPM posterior mean with its x0 clamp (ddpm_mean1), the two DDIM updates
(ddim_update, ddim_update_x0), the step noise (add_step_noise), the pinned rows (hard_row) of mmd_amd/csrc/guide_dev.h, the coefficients
make_step / make_ddim_step of mmd_amd/csrc/api.hip hand them, the stitching of cross_condition_kernel and q_sample_kernel (guide.hip).

fp32 form (`step32`): operation for operation.  The kernels spell their fmas out (so that the step kernel and the fused tail of the UNet
launch round identically), every other operation is one IEEE fp32 product, sum or division, and fp32_forms.fma_f32 is the single-rounding fma:
a correct kernel returns these bits -- from IEEE arithmetic, not from the kernel.  sigma = expf(0.5f * logvar) is a host libm call in make_step;
`expf32` is that function through ctypes.  float64 form (`step64`): the same expression on the same fp32 inputs in float64, and `value_bound`
the distance a correct fp32 evaluation may have from it.

The clamp passes a NaN and the stitching's min / max return NaN if either operand is one: x_recon.clamp_(-1., 1.), torch.min and torch.max
do (tests/test_step_edges_host.py pins that on the installed torch).  Host only."""
import ctypes
from collections import namedtuple

import numpy as np

from fp32_forms import fma_f32

H, D = 64, 4
U24 = 2.0 ** -24
F32 = np.float32

_expf = ctypes.CDLL("libm.so.6").expf
_expf.restype, _expf.argtypes = ctypes.c_float, [ctypes.c_float]


def expf32(v):
    """libm's expf on one fp32 value: what make_step calls"""
    return F32(_expf(ctypes.c_float(float(F32(v)))))


# mode: 'ddpm' (eps model, or the x0 model as a = 0, b = -1), 'ddim' (eps model), 'ddim_x0' (b holds 1 / sqrt_recipm1, 0 on the last pair)
Coeffs = namedtuple("Coeffs", "mode a b c1 c2 sigma extra do_noise")


def ddpm_coeffs(tables, i, extra_by_t, predicts_x0=False):
    """make_step: loop index i (negative: t = 0), the model's fp32 tables {name: [T]}, noise_std_extra per t"""
    t = max(int(i), 0)
    a, b = (F32(0), F32(-1)) if predicts_x0 else (F32(tables["sqrt_recip_alphas_cumprod"][t]), F32(tables["sqrt_recipm1_alphas_cumprod"][t]))
    sigma = expf32(F32(0.5) * F32(tables["posterior_log_variance_clipped"][t]))
    return Coeffs("ddpm", a, b, F32(tables["posterior_mean_coef1"][t]), F32(tables["posterior_mean_coef2"][t]), sigma,
                  F32(extra_by_t[t]), t != 0)


def ddim_coeffs(tables, t, tn, predicts_x0=False):
    """make_ddim_step: the pair (t, tn); tn = -1 is the last pair (c1 = 1, c2 = 0, and 0 for the x0 model's 1 / b)"""
    acp = tables["alphas_cumprod"]
    last = tn < 0
    c1 = F32(1) if last else np.sqrt(F32(acp[tn]))
    c2 = F32(0) if last else np.sqrt(F32(1) - F32(acp[tn]))
    a, b = F32(tables["sqrt_recip_alphas_cumprod"][t]), F32(tables["sqrt_recipm1_alphas_cumprod"][t])
    if predicts_x0:
        with np.errstate(divide="ignore"):
            b = F32(0) if last else F32(1) / b
    return Coeffs("ddim_x0" if predicts_x0 else "ddim", a, b, c1, c2, F32(0), F32(0), False)


def clamp_unit(v):
    """x.clamp(-1, 1): np.minimum / np.maximum propagate a NaN as torch's clamp does"""
    one = np.asarray(1, v.dtype)
    return np.minimum(np.maximum(v, -one), one)


def model_update32(co, x, e):
    x, e = np.asarray(x, F32), np.asarray(e, F32)
    with np.errstate(all="ignore"):
        if co.mode == "ddpm":                                  # ddpm_mean1
            x0 = clamp_unit(fma_f32(co.a, x, -(co.b * e)))
            return fma_f32(co.c1, x0, co.c2 * x)
        if co.mode == "ddim":                                  # ddim_update
            return fma_f32(co.c1, fma_f32(co.a, x, -(co.b * e)), co.c2 * e)
        return fma_f32(co.c1, e, co.c2 * (fma_f32(co.a, x, -e) * co.b))      # ddim_update_x0


def model_update64(co, x, e):
    x, e = np.asarray(x, F32).astype(np.float64), np.asarray(e, F32).astype(np.float64)
    a, b, c1, c2 = (float(v) for v in (co.a, co.b, co.c1, co.c2))
    with np.errstate(all="ignore"):
        if co.mode == "ddpm":
            return c1 * clamp_unit(a * x - b * e) + c2 * x
        if co.mode == "ddim":
            return c1 * (a * x - b * e) + c2 * e
        return c1 * e + c2 * ((a * x - e) * b)


def slots_of(rows):
    """{row: slot} of a set of pinned rows: the slot is the number of pinned rows below (hard_row: popcount of the mask below t)"""
    mask = sum(1 << int(r) for r in set(rows))
    return {t: bin(mask & ((1 << t) - 1)).count("1") for t in range(H) if (mask >> t) & 1}


def mask_of(rows):
    return sum(1 << int(r) for r in set(rows))


def pin(v, rows, hard, spr):
    """apply_hard_conditioning: row t of every trajectory of robot j // spr <- hard[robot, slot(t)]; hard [n_robots, n_rows, D], copied as words"""
    v = np.array(v)
    hard = np.asarray(hard, F32)
    for t, slot in slots_of(rows).items():
        for j in range(v.shape[0]):
            v[j, t].view(np.int32)[:] = hard[j // spr, slot].view(np.int32)
    return v


def step32(co, x, e, z, rows=(), hard=None, spr=1):
    """one step in fp32: the model update, fma(sigma z, extra, v) where the step draws noise, then the pinned rows"""
    v = model_update32(co, x, e)
    if co.do_noise:
        with np.errstate(all="ignore"):
            v = fma_f32(co.sigma * np.asarray(z, F32), co.extra, v)
    return pin(v, rows, hard, spr) if len(rows) else v


def step64(co, x, e, z, rows=(), hard=None, spr=1):
    v = model_update64(co, x, e)
    if co.do_noise:
        with np.errstate(all="ignore"):
            v = v + float(co.sigma) * np.asarray(z, F32).astype(np.float64) * float(co.extra)
    if len(rows):
        for t, slot in slots_of(rows).items():
            for j in range(v.shape[0]):
                v[j, t] = np.asarray(hard, F32)[j // spr, slot].astype(np.float64)
    return v


# roundings on the path of one element, per mode (fp32 operations between the inputs and the result):
#   ddpm     b e | fma(a, x, .) | c2 x | fma(c1, x0, .)            = 4   (the clamp rounds nothing and is 1-Lipschitz)
#   ddim     b e | fma(a, x, .) | c2 e | fma(c1, ., .)             = 4
#   ddim_x0  fma(a, x, -o) | . b_inv | c2 . | fma(c1, o, .)        = 4
#   noise    sigma z | fma(., extra, v)                            = 2 more: at most 6 < 7
ROUNDINGS = {"ddpm": 4, "ddim": 4, "ddim_x0": 4}


def value_bound(co, x, e, z, extra_roundings=0):
    """Per element, what |fp32 evaluation - step64| may be: k 2^-24 times the sum S of the magnitudes of the terms that enter the element.
    Every rounding is relative to a partial result whose magnitude is at most S (each later factor is part of S's products), so k roundings
    move the result by at most k u S (1 + O(u)); a result in the subnormal range is rounded absolutely, by at most 2^-150 per operation.
    extra_roundings: those of another fp32 evaluation order held to the same float64 form (the oracle's: see the host test)."""
    x, e = np.abs(np.asarray(x, F32).astype(np.float64)), np.abs(np.asarray(e, F32).astype(np.float64))
    a, b, c1, c2 = (abs(float(v)) for v in (co.a, co.b, co.c1, co.c2))
    with np.errstate(all="ignore"):
        if co.mode == "ddpm":
            s = c1 * (a * x + b * e) + c2 * x
        elif co.mode == "ddim":
            s = c1 * (a * x + b * e) + c2 * e
        else:
            s = c1 * e + c2 * b * (a * x + e)
        k = ROUNDINGS[co.mode] + extra_roundings
        if co.do_noise:
            s = s + abs(float(co.sigma)) * np.abs(np.asarray(z, F32).astype(np.float64)) * abs(float(co.extra))
            k += 2
        return k * U24 * s * (1 + 2.0 ** -20) + k * 2.0 ** -150


def same_words(a, b):
    """equal as fp32 words where neither is NaN, NaN in the same places (a NaN's payload is not part of any definition here)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a.view(np.int32)), np.where(nb, 0, b.view(np.int32))))


def first_word_differences(a, b, n=4):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.int32) != b.view(np.int32)))
    return [(tuple(int(k) for k in i), float(a[tuple(i)]), float(b[tuple(i)])) for i in np.argwhere(bad)[:n]], int(bad.sum())


# ---- cross conditioning and q_sample ------------------------------------------------------------------------------------------------
def cross_condition(x1, x2, ind1, ind2, rel, bnd, by_robot=None, spr=1):
    """apply_cross_conditioning for one pair, in place on copies: x1[:, ind1] = min(x2[:, ind2] + rel, bnd), then x2[:, ind2] = max(x1[:, ind1]
    - rel, -bnd); by_robot [n_robots, 8] = (rel[4], bnd[4]) per robot.  Returns (x1, x2)."""
    x1, x2 = np.array(x1, F32), np.array(x2, F32)
    n = x1.shape[0]
    if by_robot is not None:
        tab = np.asarray(by_robot, F32)[np.arange(n) // spr]
        rel, bnd = tab[:, :4], tab[:, 4:]
    else:
        rel, bnd = np.broadcast_to(np.asarray(rel, F32), (n, D)), np.broadcast_to(np.asarray(bnd, F32), (n, D))
    with np.errstate(all="ignore"):
        v1 = np.minimum(x2[:, ind2] + rel, bnd)
        x1[:, ind1] = v1
        x2[:, ind2] = np.maximum(v1 - rel, -bnd)
    return x1, x2


def q_sample64(x0, z, a, b):
    return float(F32(a)) * np.asarray(x0, F32).astype(np.float64) + float(F32(b)) * np.asarray(z, F32).astype(np.float64)


def q_sample_bound(x0, z, a, b):
    """a s + b z with or without contraction: at most three roundings (two products, one sum), each on at most |a s| + |b z|"""
    s = abs(float(F32(a))) * np.abs(np.asarray(x0, F32).astype(np.float64)) + abs(float(F32(b))) * np.abs(np.asarray(z, F32).astype(np.float64))
    return 3 * U24 * s * (1 + 2.0 ** -20) + 3 * 2.0 ** -150
