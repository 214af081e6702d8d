"""The fp32 forms of a 2-D distance that the collision decisions use, and seeded cases that put pairs / points at the margin.

torch.norm(d, dim=-1) over a last dimension of 2 in fp32 (CPU) is sqrt(fma(dy, dy, dx * dx)) rounded once per operation; the kernels
that decide collisions (multi_agent.hip, the extra-object occupancy of postprocess.hip) pin that form.  NumPy has no fma: `fma_f32` gets
the single rounding exactly by summing in float64 with the error term kept (TwoSum) and rounding to odd before the cast to float32
(53 >= 24 + 2 bits, so the second rounding is correct)."""
import numpy as np

MARGIN = np.float32(2.1 * 0.05)          # RobotPlanarDisk.check_rr_collisions: 2.1 r, r = 0.05, as the fp32 the kernels are passed


def fma_f32(a, b, c):
    """fp32 fma(a, b, c) = round_fp32(a * b + c), a single rounding, elementwise over float32 arrays.  The odd neighbour is taken on the
    side of the error term's SIGN: |e| may lie below half an ulp of s (an addend of 1 next to a product of 1e30), where s + e rounds back to
    s and a tie of the product would be broken to even instead of by the addend.  Where a * b + c is not finite the result is that inf or
    NaN (the error-free sum is not defined there)."""
    with np.errstate(all="ignore"):
        a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
        p = a * b                                              # exact: 48 significant bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                          # TwoSum: p + c = s + e exactly
        even = (s.view(np.int64) & 1) == 0
        odd = np.where((e != 0) & even & np.isfinite(s), np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)       # round to odd
        return odd.astype(np.float32)


def torch_norm2(dx, dy):
    """sqrt(fma(dy, dy, dx * dx)) in fp32: the form of torch.norm(d, dim=-1) over (dx, dy)."""
    dx, dy = np.asarray(dx, np.float32), np.asarray(dy, np.float32)
    return np.sqrt(fma_f32(dy, dy, dx * dx))


def pos_norm(pa, pb):
    """torch-form ||pa - pb|| over the last axis of two float32 [..., 2] arrays."""
    d = np.asarray(pa, np.float32) - np.asarray(pb, np.float32)
    return torch_norm2(d[..., 0], d[..., 1])


def margin_pairs(seed, n, margin=MARGIN, rel=4e-7):
    """Seeded pairs (pa, pb) float32 [m, 2] at distance margin * (1 + delta), |delta| <= rel, random directions, centred anywhere in
    [-1, 1]^2 so that |dx| and |dy| differ in size; plus axis-aligned pairs, pairs exactly fp32(margin) apart along an axis and
    coincident points.  About half of the random pairs lie on each side of the margin."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 2))
    phi = rng.uniform(0, 2 * np.pi, n)
    r = float(margin) * (1 + rng.uniform(-rel, rel, n))
    d = np.stack([np.cos(phi), np.sin(phi)], 1) * r[:, None]
    pa, pb = (c + d / 2).astype(np.float32), (c - d / 2).astype(np.float32)
    k = max(n // 16, 4)
    ca = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
    ra = (float(margin) * (1 + rng.uniform(-rel, rel, k))).astype(np.float32)
    ax = np.zeros((k, 2), np.float32)
    ax[np.arange(k), rng.integers(0, 2, k)] = ra                       # dx = 0 or dy = 0
    ex = np.zeros((k, 2), np.float32)
    ex[np.arange(k), rng.integers(0, 2, k)] = margin
    cz = np.zeros((k, 2), np.float32)                                  # exactly margin apart from the origin
    same = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
    pa = np.concatenate([pa, ca, cz, same])
    pb = np.concatenate([pb, ca + ax, ex, same])
    return pa.astype(np.float32), pb.astype(np.float32)


def near_points(rng, anchors, dist, rel=4e-7):
    """float32 points at distance dist * (1 + delta), |delta| <= rel, from float32 anchors [..., 2] (dist a scalar or per anchor), in
    random directions; a sixteenth of them along an axis and a sixteenth coincident with their anchor."""
    a = np.asarray(anchors, np.float32)
    shp = a.shape[:-1]
    phi = rng.uniform(0, 2 * np.pi, shp)
    kind = rng.integers(0, 16, shp)
    phi = np.where(kind == 0, rng.integers(0, 4, shp) * (np.pi / 2), phi)
    r = np.broadcast_to(np.asarray(dist, np.float64), shp) * (1 + rng.uniform(-rel, rel, shp))
    r = np.where(kind == 1, 0.0, r)
    d = np.stack([np.cos(phi), np.sin(phi)], -1) * r[..., None]
    d[np.abs(d) < 1e-12] = 0.0                                     # exact axes
    return (a.astype(np.float64) + d).astype(np.float32)


def sides(d, margin=MARGIN):
    """(#d < margin, #d >= margin) of torch-form distances."""
    below = int((np.asarray(d) < margin).sum())
    return below, int(np.asarray(d).size) - below
