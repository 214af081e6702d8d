"""The maximum the fused UNet kernel's dynamic input scales are taken through (csrc/unet_kernel.h, max_nn): for floats whose sign bit is
clear the UNSIGNED integer maximum of the bit patterns is the float maximum, and +inf / NaN keep the biased exponent 255 that dyn_scale reads.
numpy only, no GPU."""
import numpy as np

# +0, the smallest and the largest denormal, the smallest normal, 2^-70, 1, 2^30, the largest finite value, +inf
EDGES = np.array([0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 2.0 ** -70, 1.0, 2.0 ** 30, 3.4028235e38, np.inf], dtype=np.float32)


def umax_bits(a, b):
    """max_nn of csrc/unet_kernel.h"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.maximum(a.view(np.uint32), b.view(np.uint32)).view(np.float32)


def biased_exponent(x):
    return (np.asarray(x, np.float32).view(np.uint32) >> 23) & 0xFF


def test_unsigned_max_is_float_max_for_sign_clear_operands():
    rng = np.random.Generator(np.random.PCG64(5))
    # random sign-clear bit patterns below the NaN range (denormals to +inf) + the edge values, every pair of them
    rnd = rng.integers(0, 0x7F800001, size=2000, dtype=np.uint32).view(np.float32)
    v = np.concatenate([EDGES, rnd, np.abs(rng.standard_normal(500).astype(np.float32))])
    assert not np.isnan(v).any() and not np.signbit(v).any()
    a, b = np.meshgrid(v, v)
    want, got = np.maximum(a, b), umax_bits(a, b)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    # every edge value against every other, named: the cases of the issue
    for x in EDGES:
        for y in EDGES:
            assert umax_bits(x, y).view(np.uint32) == np.maximum(x, y).view(np.uint32), (x, y)


def test_nan_operand_keeps_exponent_255():
    """dyn_scale reads only the biased exponent of the maximum: a NaN among the operands (sign clear: the kernel takes |x| first) must
    leave it at 255 -- fp32's own answer for such a sample is NaN out."""
    nans = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000], dtype=np.uint32).view(np.float32)
    for n in nans:
        for x in EDGES:
            assert biased_exponent(umax_bits(n, x)) == 255 and biased_exponent(umax_bits(x, n)) == 255, (n, x)
    # a reduction over a row with one NaN in it
    row = np.abs(np.random.Generator(np.random.PCG64(6)).standard_normal(64).astype(np.float32))
    row[17] = np.float32(np.nan)
    m = np.float32(0.0)
    for x in np.abs(row):
        m = umax_bits(m, x)
    assert biased_exponent(m) == 255
    # +inf alone: exponent 255 as well, and it is the float maximum
    assert biased_exponent(umax_bits(np.float32(np.inf), np.float32(3.0))) == 255


def test_signed_operands_are_excluded():
    """Why the kernel uses the form only behind fabsf: with a sign bit the integer order is not the float order.  -0.0 = 0x80000000 is the
    largest unsigned pattern below the negative numbers, so it would win against every positive value."""
    neg_zero, one = np.float32(-0.0), np.float32(1.0)
    assert np.maximum(neg_zero, one) == one
    assert umax_bits(neg_zero, one).view(np.uint32) == 0x80000000          # the wrong answer: -0.0
    assert umax_bits(np.float32(-2.0), np.float32(3.0)) == np.float32(-2.0)  # and any negative value beats any positive one
    # behind fabsf both are fine
    assert umax_bits(np.abs(neg_zero), one) == one and umax_bits(np.abs(np.float32(-2.0)), np.float32(3.0)) == np.float32(3.0)
