"""A numpy float32 per-node model of the SDF grid of a map of spheres and rounded boxes: the operation sequence of sdf_grid_kernel
(mmd_amd/csrc/sdf_grid.hip), independent of torch autograd.  Every operation is one fp32 operation, no contraction; the two norms are
sqrt(fma(y, y, x * x)), the fma emulated through float64 (the product of two fp32 numbers is exact there, so the sum rounds once to
float64 and once more to fp32: the same bits as fmaf but for a double rounding that needs a 29-bit run in the exact sum).

The rules (mmd_amd/environments.py::_primitives_sdf, the reference's primitives.py:108-115, :326-333, :569-572):
  - the first of equal minima wins, spheres before boxes, in list order; with no sphere the constant 1 (gradient 0) comes first;
  - a sphere centred on the node has gradient 0;
  - inside a box the amax tie qx == qy splits evenly and minimum(max q, 0) passes half at max q == 0;
  - a zero gradient component is +0.  (The sign of a zero is the one thing not taken from autograd: it leaves -0 = 0 * -1 where a field
    has a single primitive and +0 where the contributions of several are summed.  Values are equal either way.)

The test map (tie_map) holds each tie kind; tie_masks() finds their nodes."""
import numpy as np

F = np.float32

# 5 spheres: two identical, one centred on node (137, 201) of the 400 x 400 grid (its coordinates are filled in from the node rows:
# tie_map()); 3 boxes (cx, cy, size x, size y): a square one centred on node (300, 100), so that its diagonals hit qx == qy, a thin one, and
# a small one in a corner whose distance to the far corner of the tile exceeds 1
TEST_SPHERE_NODE = (137, 201)
TEST_BOX_NODE = (300, 100)
_TEST_SPHERES = [(-0.6, 0.55, 0.12), (0.25, 0.7, 0.1), (0.25, 0.7, 0.1), None, (0.05, -0.75, 0.2)]
_TEST_BOXES = [None, (-0.35, -0.4, 0.7, 0.04), (-0.85, 0.9, 0.2, 0.1)]


def node_rows(n=400, lo=-1.0, hi=1.0):
    import torch
    return torch.linspace(lo, hi, n).numpy(), torch.linspace(lo, hi, n).numpy()


def tie_map(with_spheres=True):
    """(boxes, spheres) of the test map; with_spheres=False: the variant where the constant-1 field acts."""
    xs, ys = node_rows()
    spheres = [s if s is not None else (float(xs[TEST_SPHERE_NODE[0]]), float(ys[TEST_SPHERE_NODE[1]]), 0.15) for s in _TEST_SPHERES]
    boxes = [b if b is not None else (float(xs[TEST_BOX_NODE[0]]), float(ys[TEST_BOX_NODE[1]]), 0.3, 0.3) for b in _TEST_BOXES]
    return boxes, (spheres if with_spheres else [])


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _norm(x, y):
    return np.sqrt(_fma(y, y, x * x))


def _sign(d):
    return np.where(d > 0, F(1), np.where(d < 0, F(-1), F(0))).astype(F)


def primitive_terms(boxes, spheres, xs, ys):
    """Per primitive, in the kernel's order (spheres, then boxes): (d, gx, gy, aux) on the [nx, ny] grid, aux = the norm (spheres) or
    (qx, qy) (boxes)."""
    px, py = np.meshgrid(np.asarray(xs, F), np.asarray(ys, F), indexing="ij")
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for cx, cy, r in np.asarray(spheres, F).reshape(-1, 3):
            dx, dy = px - cx, py - cy
            n = _norm(dx, dy)
            pos = n > 0
            out.append((n - r, np.where(pos, dx / n, F(0)).astype(F), np.where(pos, dy / n, F(0)).astype(F), n))
        for cx, cy, sx, sy in np.asarray(boxes, F).reshape(-1, 4):
            hx, hy = sx / F(2), sy / F(2)
            rad = F(0.3) * min(hx, hy)
            dx, dy = px - cx, py - cy
            qx, qy = np.abs(dx) - hx + rad, np.abs(dy) - hy + rad
            mq, rx, ry = np.maximum(qx, qy), np.maximum(qx, F(0)), np.maximum(qy, F(0))
            n = _norm(rx, ry)
            d = np.minimum(mq, F(0)) + n - rad
            sgx, sgy = _sign(dx), _sign(dy)
            h = np.where(mq < 0, F(1), F(0.5)).astype(F)
            gx_in = np.where(qx > qy, h * sgx, np.where(qx < qy, F(0), F(0.5) * h * sgx))
            gy_in = np.where(qx < qy, h * sgy, np.where(qx > qy, F(0), F(0.5) * h * sgy))
            inside = mq <= 0
            gx = np.where(inside, gx_in, rx / n * sgx).astype(F)
            gy = np.where(inside, gy_in, ry / n * sgy).astype(F)
            out.append((d.astype(F), gx, gy, (qx, qy)))
    return out


def sdf_grid(boxes, spheres, xs, ys):
    """[nx, ny, 4] float32 = (sdf, d/dx, d/dy, 0) at (xs[ix], ys[iy])."""
    nx, ny = len(xs), len(ys)
    best = np.full((nx, ny), F(1) if len(spheres) == 0 else F(np.inf), F)
    gx, gy = np.zeros((nx, ny), F), np.zeros((nx, ny), F)
    for d, dgx, dgy, _ in primitive_terms(boxes, spheres, xs, ys):
        take = d < best
        best, gx, gy = np.where(take, d, best), np.where(take, dgx, gx), np.where(take, dgy, gy)
    tex = np.zeros((nx, ny, 4), F)
    tex[..., 0], tex[..., 1], tex[..., 2] = best, gx + F(0), gy + F(0)          # (-0 + 0 = +0: a zero component is +0, whatever sign autograd leaves)
    return tex


def tie_masks(boxes, spheres, xs, ys):
    """Boolean [nx, ny] masks of the nodes where each tie rule decides the texture."""
    terms = primitive_terms(boxes, spheres, xs, ys)
    tex = sdf_grid(boxes, spheres, xs, ys)
    ds = np.stack([t[0] for t in terms]) if terms else np.zeros((0,) + tex.shape[:2], F)
    n_s = len(spheres)
    at_min = ds == tex[None, ..., 0]
    equal_minimum = at_min.sum(0) >= 2
    zero_norm = np.zeros(tex.shape[:2], bool)
    for k in range(n_s):
        zero_norm |= at_min[k] & (terms[k][3] == 0)
    diag = np.zeros(tex.shape[:2], bool)
    for k in range(n_s, len(terms)):
        qx, qy = terms[k][3]
        diag |= at_min[k] & (qx == qy) & (np.maximum(qx, qy) <= 0) & (at_min[:k].sum(0) == 0)
    capped = (ds.min(0) >= 1) if n_s == 0 and len(terms) else np.zeros(tex.shape[:2], bool)
    return dict(equal_minimum=equal_minimum, zero_norm=zero_norm, box_diagonal=diag, capped=capped)
