"""The host reference of the in-kernel noise (tests/philox_ref.py) on its own, no GPU: the Random123 known answers of Philox4x32-10,
the edges of the uniform mapping, and independence of the Gaussian values along every counter and key dimension the project varies
(draw, stream id = consecutive keys, the reserved x_T draw, the high word of the point index, neighbouring points).  Every input is
fixed, so every figure is deterministic; the conditions are 5 sigma of the estimator for N(0,1) samples."""
import numpy as np
import pytest

import philox_ref as P

KNOWN_ANSWERS = [        # Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_known_answers(ctr, key, out):
    got = P.philox4x32_10(np.array(ctr, dtype=np.uint64), key[0], key[1])
    assert [int(v) for v in got] == list(out), [hex(int(v)) for v in got]


def test_known_answers_vectorised_and_through_normal4s_counter_layout():
    """the three vectors as one [3, 4] call with per-row keys; and normal4's own (point, draw, seed) packing reproduces the third: counter
    word 3 is 0 there, so the expected words are computed with the (known-answer-checked) primitive on the documented layout"""
    ctr = np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64)
    got = P.philox4x32_10(ctr, np.array([k[1][0] for k in KNOWN_ANSWERS]), np.array([k[1][1] for k in KNOWN_ANSWERS]))
    assert got.tolist() == [list(k[2]) for k in KNOWN_ANSWERS]
    seed, draw, point = (0x299f31d0 << 32) | 0xa4093822, 0x85a308d3, (0x13198a2e << 32) | 0x243f6a88
    w = P.philox4x32_10(np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, 0], dtype=np.uint64), 0xa4093822, 0x299f31d0)
    u = P.uniform01(w).astype(np.float64)
    z, r = P.normal4(seed, draw, [point])
    assert np.allclose(r[0, [0, 2]], np.sqrt(-2 * np.log(u[[0, 2]])), rtol=1e-15)
    assert np.allclose(z[0, 0], r[0, 0] * np.cos(np.float64(np.float32(6.283185307179586) * np.float32(u[1]))), rtol=1e-12)
    # every argument reaches the counter / key: changing any one changes the output
    for other in ((seed ^ (1 << 40), draw, point), (seed ^ 1, draw, point), (seed, draw ^ 1, point), (seed, draw, point ^ (1 << 35)),
                  (seed, draw, point ^ 1)):
        assert not np.array_equal(P.normal4(*other[:2], [other[2]])[0], z), other


def test_uniform_edges():
    u = P.uniform01(np.array([0, 1, 2 ** 24, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1], dtype=np.uint64))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.5 * 2.0 ** -32)
    assert u[2] == np.float32(2.0 ** -8)                       # 2^24 + 0.5 ties to even: 2^24
    assert u[3] < 1.0 and u[4] == 1.0 and u[5] == 1.0          # u32 -> f32 rounds the top 128 values to 2^32 (the tie goes to even)
    assert (u > 0).all()
    # u = 1: r = 0 and z = 0, no NaN; u = 2^-33: the largest radius, finite.  Box-Muller on hand-made uniforms through the same
    # arithmetic normal4 uses
    r_max = np.sqrt(-2.0 * np.log(np.float64(u[0])))
    assert np.isfinite(r_max) and 6.7 < r_max < 6.8
    assert np.sqrt(np.abs(-2.0 * np.log(np.float64(u[5])))) == 0.0


def test_no_nan_no_inf_and_r_is_the_radius():
    seed = (18 << 24) + 5
    for draw in (0, 7, P.DRAW_Q_SAMPLE, P.DRAW_XT):
        z, r = P.normal4(seed, draw, np.arange(2 ** 16, dtype=np.uint64))
        assert np.isfinite(z).all() and np.isfinite(r).all() and (r >= 0).all()
        assert np.allclose(z[:, 0] ** 2 + z[:, 1] ** 2, r[:, 0] ** 2, rtol=1e-12, atol=1e-300)
        assert np.allclose(z[:, 2] ** 2 + z[:, 3] ** 2, r[:, 2] ** 2, rtol=1e-12, atol=1e-300)
        assert np.array_equal(r[:, 0], r[:, 1]) and np.array_equal(r[:, 2], r[:, 3])


def test_point_helpers():
    assert P.traj_points(7, 2).tolist() == list(range(7 * 64, 9 * 64))
    p = P.traj_points(2 ** 26 - 1, 2)                          # the carry into the high counter word falls inside the batch
    assert int(p[63]) == 2 ** 32 - 1 and int(p[64]) == 2 ** 32 and p.dtype == np.uint64
    rob, pts = P.robot_points(3, 5)
    assert rob.tolist() == [0] * 320 + [1] * 320 + [2] * 320 and pts.tolist() == list(range(320)) * 3
    z, r = P.traj_normal4(11, 3, 4, traj_base=9)
    assert np.array_equal(z.reshape(-1, 4), P.normal4(11, 3, 9 * 64 + np.arange(256))[0])
    zr, _ = P.traj_normal4(None, 3, 4, robot_seeds=[21, 22], samples_per_robot=2)
    assert np.array_equal(zr[2:].reshape(-1, 4), P.normal4(22, 3, np.arange(128))[0])
    # a shard draws what the unsharded call draws
    assert np.array_equal(P.traj_normal4(11, 3, 6)[0][4:], P.traj_normal4(11, 3, 2, traj_base=4)[0])


# ---- independence --------------------------------------------------------------------------------------------------------------------
N = 2 ** 18
SEED = (18 << 24) + 5                                           # what next_stream_seed(18) gives on its sixth call


def _rho(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


@pytest.fixture(scope="module")
def base():
    return P.normal4(SEED, 3, np.arange(N, dtype=np.uint64))[0]


def test_moments_are_standard_normal(base):
    for name, z in (("draw3", base), ("x_T", P.normal4(SEED, P.DRAW_XT, np.arange(N, dtype=np.uint64))[0])):
        for j in range(4):
            v = z[:, j]
            assert abs(v.mean()) < 5 / np.sqrt(N), (name, j, v.mean() * np.sqrt(N))
            assert abs((v ** 2).mean() - 1) < 5 * np.sqrt(2 / N), (name, j)
            assert abs((v ** 4).mean() - 3) < 5 * np.sqrt(96 / N), (name, j)


@pytest.mark.parametrize("name", ["next_draw", "next_seed", "x_T_draw", "point_high_word"])
def test_streams_are_uncorrelated(base, name):
    p = np.arange(N, dtype=np.uint64)
    other = {"next_draw": lambda: P.normal4(SEED, 4, p), "next_seed": lambda: P.normal4(SEED + 1, 3, p),
             "x_T_draw": lambda: P.normal4(SEED, P.DRAW_XT, p), "point_high_word": lambda: P.normal4(SEED, 3, p + np.uint64(2 ** 32))}[name]()[0]
    assert not np.array_equal(other, base)
    for i in range(4):
        for j in range(4):
            assert abs(_rho(base[:, i], other[:, j])) < 5 / np.sqrt(N), (name, i, j)


def test_points_and_components_are_uncorrelated(base):
    for lag in (1, 64):                                         # the next support point, the same support point of the next trajectory
        for j in range(4):
            assert abs(_rho(base[:-lag, j], base[lag:, j])) < 5 / np.sqrt(N - lag), (lag, j)
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(_rho(base[:, i], base[:, j])) < 5 / np.sqrt(N), (i, j)
    # the two values of one Box-Muller pair share a radius: uncorrelated is not enough, their squares must be uncorrelated too
    assert abs(_rho(base[:, 0] ** 2, base[:, 1] ** 2)) < 5 / np.sqrt(N)
    assert abs(_rho(base[:, 2] ** 2, base[:, 3] ** 2)) < 5 / np.sqrt(N)
