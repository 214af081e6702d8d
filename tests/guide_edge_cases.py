"""Seeded inputs that put every DISCRETE decision of the guide gradient (guide_grad, mmd_amd/csrc/guide.hip) at its edge: the SDF cell index,
the object hinge and its arg max over the grids, the workspace walls and their arg max, the constraint radius, the extra objects' ties and
the gradient clip rules.  Host only: numpy, torch and the oracle.  tests/test_guide_edges_host.py checks on the oracle alone that every builder
holds both sides of its decision; tests/test_gpu_guide_edges.py runs the kernels on them.

A guide-only iteration returns y = x + guide(x), so a decision is read back from y - x: every builder isolates ONE cost term (the other
weights zero, the walls out of reach) and encodes the decision in the term's data -- a grid whose gradient at cell (ix, iy) is
(ix, iy) / 1024, gradients that differ per grid, unit wall normals, one constraint slot per planted point.

Positions.  With the tests' normaliser the position limits are -1 / +1: p = ((clip(x) + 1) / 2) * 2 - 1 = fl(x + 1) - 1 whether or not the
multiply-add is contracted (/ 2, * 2 and the final subtraction are exact).  So the positions a trajectory can take are the LATTICE
{x a float32 : x + 1 a float32}, spacing 2^-23 on [0, 1] and 2^-24 on [-1, 0), and on a lattice point p == x bitwise.  Every planted point is
a lattice point (`lattice`), "k ulps from an edge" means k lattice steps, and each label's side and distance are recomputed in float64 from
the fp32 operands actually planted, never from the intent."""
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

import cases
import fp32_forms as F
from oracle import mmd_oracle as O

H, D = 64, 4
U24 = 2.0 ** -24                          # unit roundoff of fp32
FAR = 1e6                                 # workspace walls out of reach
R = np.float32(0.05 * 2.4)                # the vertex-constraint radius (mmd_params.py:52), as the fp32 the tables hold
R2 = np.float32(R * np.abs(R))            # R|R| in fp32: the number cons_term compares with
# The constraint BAND, in ulps of R.  With d = fl(p - q) (the same fp32 operands on both sides) and D = ||d|| exact:
#   kernel  fma(dx, dx, fl(dy dy)) > fl(R|R|): fl(dy dy) = dy^2 (1 + e1), the fma rounds once more, so the left side is D^2 (1 + e),
#           |e| <= 2 u (u = 2^-24), and fl(R|R|) = R^2 (1 + e'), |e'| <= u: the test is D > R sqrt((1 + e') / (1 + e)), a threshold within
#           R (1 +- 1.5 u);
#   oracle  sqrt(fma(dy, dy, fl(dx dx))) > R: the radicand is D^2 (1 + e), |e| <= 2 u, the square root halves that and rounds once: a
#           threshold within R (1 +- 2 u).
# R < 2^24 ulp(R), so R 2 u < 2 ulp(R): both thresholds lie within K = 2 ulps of R, and for |D - R| > 2 ulp(R) both decide as float64 does.
K_BAND = 2.0

# One planted point.  side / ulps: the decision and the distance to the edge in float64 from the fp32 operands.  exact: the kernel must take the
# fp32 oracle's decision (False: the point lies inside the constraint band, either decision passes).  side32 (cell kinds): the decision of the
# fp32 operation sequence, replayed in numpy -- what the device is held to where the sequence rounds across the integer and differs from
# `side`.  carrier (tables_instance): the other robot whose path point is planted next to the sample point.
Label = namedtuple("Label", "kind traj t side ulps exact side32 carrier", defaults=(None, None))
T_ORDER = [t for pair in zip(range(1, H // 2), range(H - 2, H // 2 - 1, -1)) for t in pair]      # 1, 62, 2, 61, ...


def ulps(x, k):
    """float32 x moved by k units in the last place, towards +inf for k > 0."""
    x = np.float32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return np.float32(x)


def lattice_step(e):
    """spacing of the lattice at e: a lattice point is a float32 x whose x + 1 is a float32 too"""
    e32 = np.float32(e)
    return float(max(np.spacing(np.abs(e32)), np.spacing(np.float32(e32 + np.float32(1)))))


def lattice(e, k=0):
    """The lattice point nearest to e (|e| <= 1), moved by k lattice steps (each of the spacing on the side it moves to)."""
    s = lattice_step(e)
    v = np.rint(np.float64(e) / s) * s
    for _ in range(abs(int(k))):
        side = np.float32(np.inf if k > 0 else -np.inf)
        v += np.sign(k) * lattice_step(np.nextafter(np.float32(v), side))
    x = np.float32(v)
    assert float(x) == v and float(np.float32(x + np.float32(1))) == v + 1, (e, k)
    return x


def unnorm32(x):
    """the oracle's / kernel's fp32 un-normalisation of a position coordinate (limits -1 / +1), operation for operation"""
    v = np.clip(np.asarray(x, np.float32), np.float32(-1), np.float32(1))
    return ((v + np.float32(1)) / np.float32(2) * np.float32(2) + np.float32(-1)).astype(np.float32)


@dataclass
class Case:
    name: str
    x: np.ndarray                                  # [B, 64, 4] float32, normalised
    gp: O.GuideParams
    labels: List[Label]
    cons: list = field(default_factory=list)       # oracle ConstraintGroups (one robot)
    desc: Dict[str, object] = field(default_factory=dict)      # mmd_guide_desc fields to patch (the term's isolation)
    tex: Optional[np.ndarray] = None               # synthetic texture [n_grids, nx, ny, 4], or None
    env: str = "EnvEmpty2D"
    clip_rule: Optional[str] = "norm"              # 'norm' | 'value' | None
    max_grad_value: float = 0.1
    extra_objects: Optional[dict] = None
    term_roundings: int = 8                        # T of the value bound (value_bound below)

    def ref32(self):
        return O.guide_grad(torch.from_numpy(self.x), self.gp, self.cons, clip_mode="always", clip_rule=self.clip_rule,
                            max_grad_value=self.max_grad_value)

    def ref64(self):
        """the same guide in float64 on the same fp32 inputs.  The cell index is taken from the fp32 oracle (guide_grad_forced): it is the
        one decision whose float64 form may round differently; every other decision of an exact label is the same in both (host test)."""
        x = torch.from_numpy(self.x)
        if self.name.startswith("cell"):
            return O.guide_grad_forced(x.double(), self.gp, self.cons, O.guide_decisions(x, self.gp, self.cons))
        return O.guide_grad(x.double(), self.gp, self.cons, clip_mode="always", clip_rule=self.clip_rule, max_grad_value=self.max_grad_value)


def value_bound(case, ref64):
    """Per element, what |(y - x) - ref64| may be for a correct fp32 kernel:
      (|x| + 2 |g|) u    y = fl(x + g) is off by at most u |x + g| <= u (|x| + |g|), and y - x rounds once more, by at most u |g|;
      T |g|_term u       the term's own operations, T = case.term_roundings, on the size of the unclipped term: the norm clip is 4 adds of
                         1e-6, 4 products and 3 adds for the squared norm (<= 6 u on it, halved by the root: 3 u), v_rsq_f32 at 1 ulp (2 u),
                         the product with max_norm, the scale and the weight (3 u): T = 8; a constraint's unit vector adds the squared
                         distance (2 u, halved), the rsq (2 u) and the fma (1 u): T = 13; a sum of n unit vectors: see clip_off_case.  An element whose reference is exactly 0 (an inactive point, the
                         zero component of an axis-aligned vector) gets no such allowance: it is a product with 0 and must come back 0."""
    g = ref64.abs().numpy()
    return U24 * (np.abs(case.x.astype(np.float64)) + 2 * g) + case.term_roundings * U24 * np.where(g == 0, 0.0, np.maximum(g, case_scale(case)))


def case_scale(case):
    """size of the unclipped term (the clip's rounding acts on it): 1 for unit vectors, the largest planted gradient for grids"""
    if case.tex is not None:
        return float(np.abs(case.tex[..., 1:3]).max())
    return 1.0


class _Batch:
    """B trajectories of neutral points; plant() takes the next free (trajectory, support point), support points in the order 1, 62, 2,
    61, ... so that every kind has edges at 1 and 62."""

    def __init__(self, B, neutral, one_per_t=False):
        self.x = np.zeros((B, H, D), np.float32)
        self.x[..., :2] = np.asarray(neutral, np.float32)
        self.labels = []
        self.free = [(b, t) for t in T_ORDER for b in range(B)] if not one_per_t else [(k % B, t) for k, t in enumerate(T_ORDER)]
        self.k = 0

    def plant(self, xy, kind, side, dist, exact=True, side32=None):
        b, t = self.free[self.k]
        self.k += 1
        self.x[b, t, :2] = np.asarray(xy, np.float32)
        self.labels.append(Label(kind, b, t, side, float(dist), bool(exact), side32))
        return b, t

    def ends(self, xy):
        """rows 0 and 63 of every trajectory: an ACTIVE point of the term, which must come back exactly 0"""
        self.x[:, 0, :2] = self.x[:, H - 1, :2] = np.asarray(xy, np.float32)


def _gp(**kw):
    return O.GuideParams(norm_mins=cases.MINS, norm_maxs=cases.MAXS, sdf_grids=kw.pop("sdf_grids", []), **kw)


def _grids(tex):
    return [(torch.from_numpy(tex[k, ..., 0].copy()), torch.from_numpy(tex[k, ..., 1:3].copy())) for k in range(tex.shape[0])]


OBJ_ONLY = dict(weight_collision=1.0, weight_smoothness=0.0, ws_min=[-FAR, -FAR], ws_max=[FAR, FAR])
_FAR_WS = dict(ws_min=torch.tensor([-FAR, -FAR]), ws_max=torch.tensor([FAR, FAR]))

# ---- 1. SDF cell -------------------------------------------------------------------------------------------------------------------
CELL_N, CELL_LO, CELL_HI = (24, 40), (-1.0, -0.75), (0.5, 1.0)          # not square, limits not symmetric, all exactly representable


def cell_texture():
    """sdf = 0 everywhere (every cell active), gradient (ix, iy) / 1024: ||grad + 1e-6|| < 1, so the clip factor is exactly 1 and
    round((y - x) 1024) is the cell the kernel read (guide(x) = -w d cost / dp = +grad sdf)."""
    ix, iy = np.meshgrid(np.arange(CELL_N[0]), np.arange(CELL_N[1]), indexing="ij")
    tex = np.zeros((1,) + CELL_N + (4,), np.float32)
    tex[0, ..., 1], tex[0, ..., 2] = ix / 1024.0, iy / 1024.0
    return tex


def cell_index64(p, axis, n=CELL_N, lo=CELL_LO, hi=CELL_HI):
    """float64 floor((p - lo) / dim n) clamped, from the fp32 operands p, lo and dim = |hi - lo| (fp32)"""
    lo32 = np.float32(lo[axis])
    dim = np.abs(np.float32(hi[axis]) - lo32)
    u = (np.asarray(p, np.float64) - float(lo32)) / float(dim) * n[axis]
    return np.clip(np.floor(u), 0, n[axis] - 1).astype(np.int64), u


def cell_index32(p, axis, n=CELL_N, lo=CELL_LO, hi=CELL_HI):
    """the reference's fp32 operation sequence floor((p - lo) / dim * n), clamped, replayed in numpy"""
    lo32 = np.float32(lo[axis])
    dim = np.abs(np.float32(hi[axis]) - lo32)
    u = np.floor(np.float32(np.float32(np.float32(np.float32(p) - lo32) / dim) * np.float32(n[axis])))
    return int(np.clip(u, 0, n[axis] - 1))


def decode_cell(delta):
    """(ix, iy) from y - x on the cell-encoding grid"""
    return np.rint(np.asarray(delta, np.float64)[..., :2] * 1024).astype(np.int64)


def cell_case():
    b = _Batch(16, (0.0, 0.0))
    lo, hi, n = CELL_LO, CELL_HI, CELL_N

    def centre(axis, j):
        return lattice(lo[axis] + (j + 0.5) * (hi[axis] - lo[axis]) / n[axis])

    def put(axis, c, kind, dist, j):
        other = centre(1 - axis, j % n[1 - axis])
        xy = (c, other) if axis == 0 else (other, c)
        p = float(unnorm32(c))
        b.plant(xy, f"{kind}_{'xy'[axis]}", int(cell_index64(p, axis)[0]), dist, side32=cell_index32(p, axis))

    for axis in (0, 1):
        for i in range(1, n[axis]):                                    # every interior edge at 0, +-1 and +-2 lattice steps
            e = lo[axis] + i * (hi[axis] - lo[axis]) / n[axis]
            for k in (-2, -1, 0, 1, 2):
                c = lattice(e, k)
                put(axis, c, "cell_edge", (float(c) - e) / lattice_step(lattice(e)), 7 * i + k)
        put(axis, np.float32(lo[axis]), "cell_lo", 0, 3)               # index 0
        put(axis, np.float32(hi[axis]), "cell_hi", 0, 5)               # index n, clamped to n - 1
        for k, c in enumerate((1.0, -1.0, ulps(1.0, 1), ulps(-1.0, -1), 1.5, -1.5)):      # the un-normalise clip: p = +-1
            put(axis, np.float32(c), "cell_clip", 0, 11 + k)
        put(axis, lattice(hi[axis] + 0.2) if axis == 0 else lattice(lo[axis] - 0.15), "cell_beyond", 0, 2)
        put(axis, lattice(-0.999) if axis == 1 else lattice(0.75), "cell_beyond", 0, 9)
    b.ends((centre(0, 5), centre(1, 7)))
    tex = cell_texture()
    gp = _gp(sdf_grids=_grids(tex), limits_lo=torch.tensor(lo), limits_hi=torch.tensor(hi), weight_collision=1.0, weight_smoothness=0.0,
             **_FAR_WS)
    return Case("cell", b.x, gp, b.labels, desc=dict(OBJ_ONLY, limits_lo=list(lo), limits_hi=list(hi)), tex=tex, term_roundings=0)


def cell_real_case():
    """The real 400 x 400 EnvHighways2D grid at cell edges whose two cells decide the hinge differently (0, +-1 and +-2 lattice steps: one step moves (p + 1) / 2 * 400 by less than its fp32 ulp): the
    output is 0 on one side and the clipped gradient on the other."""
    import post_edge_cases as P
    gp0 = cases.guide_params("EnvHighways2D")
    gp = _gp(sdf_grids=gp0.sdf_grids, weight_collision=1.0, weight_smoothness=0.0, **_FAR_WS)
    axis, i, j, _ = P.flip_pairs(gp, gp.margin)
    pick = np.random.default_rng(41).permutation(len(axis))[:24]
    b = _Batch(4, (0.5, 0.5))
    sdf = gp.sdf_grids[0][0].numpy()
    assert sdf[300, 300] > 2 * gp.margin                               # the neutral point is inactive
    for a, ii, jj in zip(axis[pick], i[pick], j[pick]):
        e = -1.0 + (ii + 1) * 0.005
        for k in (-2, -1, 0, 1, 2):
            c, other = lattice(e, k), lattice(float(P.centre(jj)))
            xy = (c, other) if a == 0 else (other, c)
            real = dict(n=(400, 400), lo=(-1.0, -1.0), hi=(1.0, 1.0))
            idx, idx32 = int(cell_index64(float(c), 0, **real)[0]), cell_index32(c, 0, **real)
            cell, cell32 = ((idx, jj), (idx32, jj)) if a == 0 else ((jj, idx), (jj, idx32))
            b.plant(xy, "cell_real", int(sdf[cell] < gp.margin), (float(c) - e) / lattice_step(c), side32=int(sdf[cell32] < gp.margin))
    deep = np.unravel_index(np.argmin(sdf), sdf.shape)
    b.ends((lattice(float(P.centre(deep[0]))), lattice(float(P.centre(deep[1])))))
    return Case("cell_real", b.x, gp, b.labels, desc=dict(OBJ_ONLY), env="EnvHighways2D")


# ---- 2. object hinge and arg max over grids ------------------------------------------------------------------------------------------
HINGE_N = (16, 16)


def decode_hinge(delta):
    """(active, cell, grid) from y - x on the hinge grids: grid k holds the gradient ((cell + 1), (k + 1)) / 1024 at its cells"""
    d = np.asarray(delta, np.float64)[..., :2] * 1024
    active = np.abs(d).max(-1) > 0.25
    return np.stack([active, np.where(active, np.rint(d[..., 0]) - 1, -1), np.where(active, np.rint(d[..., 1]) - 1, -1)], -1).astype(np.int64)


def hinge_case(margin):
    """Cells whose sdf is the margin, one and two ulps either side of it, and pairs of grids that tie or differ by one ulp.  All values lie
    within 8 ulps of the margin, so margin - sdf is exact in fp32 and the fp32 and float64 decisions are the same."""
    m = np.float32(margin)
    off = 1.0                                                          # inactive
    specs = [(ulps(m, k), off, "hinge", int(k < 0), k) for k in (-2, -1, 0, 1, 2)]
    specs += [(off, ulps(m, k), "hinge_grid1", int(k < 0), k) for k in (-2, -1, 0, 1, 2)]
    specs += [(ulps(m, -4), ulps(m, -4), "argmax_tie", 0, 0), (ulps(m, -4), ulps(m, -5), "argmax_deeper1", 1, 1),
              (ulps(m, -5), ulps(m, -4), "argmax_deeper0", 0, -1), (m, ulps(m, -1), "argmax_deeper1", 1, 1), (ulps(m, -1), m, "argmax_deeper0", 0, -1),
              (0.0, 0.0, "argmax_tie", 0, 0), (ulps(m, -1), ulps(m, -1), "argmax_tie", 0, 0)]
    nx, ny = HINGE_N
    tex = np.zeros((2, nx, ny, 4), np.float32)
    tex[..., 0] = 1.0
    cell = np.arange(nx * ny).reshape(nx, ny)
    for k in range(2):
        tex[k, ..., 1], tex[k, ..., 2] = (cell + 1) / 1024.0, (k + 1) / 1024.0
    b = _Batch(4, (lattice(-1 + 0.5 * 2 / nx), lattice(-1 + 0.5 * 2 / ny)))          # neutral: the centre of cell (0, 0), inactive
    act = None
    for rep in range(2):                                               # twice, so that the edges also land on support points 1 and 62
        for s, (s0, s1, kind, side, k) in enumerate(specs):
            ix, iy = 1 + (5 * s + 3 * rep) % (nx - 2), 1 + (s + 7 * rep) % (ny - 2)
            while tex[0, ix, iy, 0] != 1.0 or tex[1, ix, iy, 0] != 1.0:
                iy = 1 + iy % (ny - 2)
            tex[0, ix, iy, 0], tex[1, ix, iy, 0] = s0, s1
            xy = (lattice(-1 + (ix + 0.5) * 2 / nx), lattice(-1 + (iy + 0.5) * 2 / ny))
            b.plant(xy, kind, side, k)
            if kind == "argmax_tie" and act is None:
                act = xy
    b.ends(act)
    gp = _gp(sdf_grids=_grids(tex), weight_collision=1.0, weight_smoothness=0.0, **_FAR_WS)
    return Case("hinge", b.x, gp, b.labels, desc=dict(OBJ_ONLY), tex=tex, term_roundings=0)


def decode_extra_win(delta):
    """(active, the extra objects win) from y - x on hinge_extra_case: the sphere's gradient is the unit vector (1, 0), a grid's is below 1 / 2"""
    d = np.asarray(delta, np.float64)[..., :2]
    return np.stack([np.abs(d).max(-1) > 1e-4, np.abs(d[..., 0]) > 0.5], -1).astype(np.int64)


def hinge_extra_case(margin):
    """The analytic field of the extra objects against a grid cell, both below the margin: the point sits at a cell centre, a quarter to the
    right of a sphere's centre (dx = 1/4, dy = 0), so ||d|| = 1/4 and sdf = 1/4 - r are exact on both sides (and in float64), and the cell
    holds 1/4 - r0 exactly: with r = r0 moved by k ulps the sphere is k x 2^-26 deeper (k > 0) or shallower than the cell.  The first
    maximum wins, the grid comes first: the sphere wins iff it is strictly deeper.  Every operation of the comparison is exact for these
    operands, so the band of this decision is empty here and the labels are exact."""
    m = np.float32(margin)
    nx, ny = HINGE_N
    tex = np.zeros((1, nx, ny, 4), np.float32)
    tex[..., 0] = 1.0
    r0 = np.float32(0.2)
    s = np.float32(np.float32(0.25) - r0)
    assert float(s) == 0.25 - float(r0) and float(np.float32(m - s)) == float(m) - float(s) and s < m
    b = _Batch(4, (lattice(-1 + 14.5 * 2 / nx), lattice(-1 + 0.5 * 2 / ny)))       # neutral: cell (14, 0), inactive, away from the spheres
    spheres, first = [], None
    for n, k in enumerate((-2, -1, 0, 1, 2)):
        ix, iy = 4, 1 + 3 * n
        px, py = lattice(-1 + (ix + 0.5) * 2 / nx), lattice(-1 + (iy + 0.5) * 2 / ny)
        tex[0, ix, iy] = (s, (ix * ny + iy + 1) / 1024.0, 1 / 1024.0, 0)
        r = ulps(r0, k)
        spheres.append((np.float32(px - np.float32(0.25)), py, r))
        assert np.float32(px - spheres[-1][0]) == 0.25
        for rep in range(2):
            b.plant((px, py), "hinge_extra", int((0.25 - float(r)) < float(s)), k)
        first = first or (px, py)
    b.ends(first)
    sph = np.asarray(spheres, np.float32)
    gp = _gp(sdf_grids=_grids(tex), weight_collision=1.0, weight_smoothness=0.0, extra_spheres=torch.from_numpy(sph), **_FAR_WS)
    return Case("hinge_extra", b.x, gp, b.labels, desc=dict(OBJ_ONLY), tex=tex, extra_objects=dict(spheres=sph.tolist()))


# ---- 3. workspace walls --------------------------------------------------------------------------------------------------------------
WS = np.float32(1.08)                              # tasks.py:81-83: the limits x 1.08


def decode_wall(delta):
    """(active, wall) from y - x with only the wall term on, w = 1: wall 0: x-min, 1: y-min, 2: x-max, 3: y-max"""
    d = np.asarray(delta, np.float64)[..., :2]
    active = np.abs(d).max(-1) > 0.5
    axis = np.argmax(np.abs(d), -1)
    neg = np.take_along_axis(d, axis[..., None], -1)[..., 0] < 0        # y - x = -w normal: the max walls push towards -
    return np.stack([active, np.where(active, axis + 2 * neg, -1)], -1).astype(np.int64)


def wall_case(margin):
    m = np.float32(margin)
    b = _Batch(4, (0.0, 0.0))
    for wall in range(4):
        axis, sign = wall % 2, (-1.0 if wall < 2 else 1.0)
        e = sign * (float(WS) - float(m))                              # p with margin - distance = 0
        for k in (-1, 0, 1):
            c = lattice(e, k)
            dist = np.float64(c) + float(WS) if wall < 2 else float(WS) - np.float64(c)
            xy = (c, lattice(0.3)) if axis == 0 else (lattice(-0.3), c)
            b.plant(xy, f"wall{wall}", int(float(m) - dist > 0), (float(c) - e) / lattice_step(c))
    a, a1 = lattice(0.99), lattice(0.99, 1)                            # both on the lattice with either sign
    # equal penetration at the corners: the first maximum in the order x-min, y-min, x-max, y-max wins; one step deeper on the later wall: that wall
    for (sx, sy), first, later in (((-1, -1), 0, 1), ((1, -1), 1, 2), ((-1, 1), 0, 3), ((1, 1), 2, 3)):
        b.plant((sx * a, sy * a), "wall_corner_tie", first, 0)
        deeper = (sx * a1, sy * a) if later % 2 == 0 else (sx * a, sy * a1)
        b.plant(deeper, "wall_corner_later", later, 1)
    b.ends((lattice(-0.995), lattice(0.2)))
    gp = _gp(weight_collision=1.0, weight_smoothness=0.0)
    return Case("walls", b.x, gp, b.labels, desc=dict(weight_collision=1.0, weight_smoothness=0.0, n_grids=0))


# ---- 4. constraint radius ------------------------------------------------------------------------------------------------------------
NO_BASE = dict(weight_collision=0.0, weight_smoothness=0.0, n_grids=0)
NEUTRAL = (lattice(0.875), lattice(0.875))
RANGE_T = (30, 31, 32)                             # the support points of the time-range case


def _f32(*v):
    return np.asarray(v, np.float32)


def dist_ulps(p, q, radius=R):
    """(||fl(p - q)|| - R) / ulp(R) in float64 from the fp32 operands"""
    d = (np.asarray(p, np.float32) - np.asarray(q, np.float32)).astype(np.float64)
    return float((np.hypot(d[0], d[1]) - float(radius)) / float(np.spacing(np.float32(radius))))


def _search_offset(phi, want, span=40, radius=float(R)):
    """fp32 (dx, dy) near radius (cos phi, sin phi), each coordinate within `span` ulps, minimising want(dx [n, n], dy [n, n]) -> score"""
    dx0, dy0 = np.float32(radius * np.cos(phi)), np.float32(radius * np.sin(phi))
    k = np.arange(-span, span + 1)
    dx = (dx0 + k * np.spacing(dx0)).astype(np.float32)[:, None] * np.ones((1, len(k)), np.float32)
    dy = (dy0 + k * np.spacing(dy0)).astype(np.float32)[None, :] * np.ones((len(k), 1), np.float32)
    score = want(dx, dy)
    i, j = np.unravel_index(np.argmin(score), score.shape)
    return dx[i, j], dy[i, j], float(score[i, j])


def constraint_case():
    """One group of weight 1, one slot per planted point: the point of support point t belongs to trajectory t % 4 and lies within 2^-20 of
    the origin, where q = p - d and d = fl(p - q) are exact at the 2^-27 spacing of R; the other trajectories rest at NEUTRAL, out of reach."""
    b = _Batch(4, NEUTRAL, one_per_t=True)
    b.free = [f for f in b.free if f[1] not in RANGE_T]
    q, tr, rad = [], [], []
    anchors = [_f32(0, 0), _f32(3 * 2.0 ** -23, -(2.0 ** -22))]

    def add(p, qq, kind, side, dist, exact=True, radius=R):
        bb, t = b.plant(p, kind, side, dist, exact)
        assert np.all(np.abs(np.asarray(p, np.float64) - np.asarray(qq, np.float64)) < 0.2)
        q.append(np.asarray(qq, np.float32)); tr.append((t, t + 1)); rad.append(radius)
        return bb, t

    n = 0
    for axis in (0, 1):                                                # exact: along an axis ||d|| = |dx| on both sides of the comparison
        for sign in (1, -1):
            for k in (-2, -1, 0, 1, 2):
                p = anchors[n % 2]; n += 1
                d = np.zeros(2, np.float32)
                d[axis] = sign * ulps(R, k)
                qq = (p - d).astype(np.float32)
                assert np.array_equal(p - qq, d)
                add(p, qq, "cons_axis", int(k <= 0), k)
    for phi in (np.pi / 4, 0.6 + np.pi):                               # a diagonal and a general direction, at k ulps of R
        for k in (1, -1, 2, -2, 4, -4, 8, -8, 64, -64):
            target = float(R) + k * float(np.spacing(R))
            dx, dy, _ = _search_offset(phi, lambda a, c: np.abs(np.hypot(a.astype(np.float64), c.astype(np.float64)) - target), radius=target)
            p = anchors[n % 2]; n += 1
            qq = (p - _f32(dx, dy)).astype(np.float32)
            assert np.array_equal(p - qq, _f32(dx, dy))
            du = dist_ulps(p, qq)
            add(p, qq, "cons_general", int(du <= 0), du, exact=abs(du) > K_BAND)
    for k in (-1, 0, 1):                                               # fma(dx, dx, dy dy) == R|R| and its two fp32 neighbours exactly
        t2 = ulps(R2, k)
        dx, dy, miss = _search_offset(1.1, lambda a, c: np.abs(F.fma_f32(a, a, c * c).astype(np.float64) - float(t2)))
        assert miss == 0.0
        qq = (-_f32(dx, dy)).astype(np.float32)
        du = dist_ulps(_f32(0, 0), qq)
        add(_f32(0, 0), qq, "cons_d2", int(k <= 0), du, exact=abs(du) > K_BAND)
    add(_f32(0.25, -0.5), _f32(0.25, -0.5), "cons_d0", 1, -float(R) / float(np.spacing(R)))           # d = 0: active, gradient 0
    add(_f32(0, 0), _f32(0, 0), "cons_r0_d0", 1, 0, radius=np.float32(0))                              # R = 0, d = 0: active, gradient 0
    add(_f32(0, 0), _f32(-1.4e-45, 0), "cons_r0_denormal", 0, 1, exact=False, radius=np.float32(0))    # R = 0 < |d|, but d^2 underflows in fp32 on both sides: no gradient either way
    # a slot whose time range ends at t: active at t - 2 and t - 1, not at t (exclusive end, cost_functions.py:305), through the host pack
    p, qq = _f32(0, 0), _f32(0.0625, 0)
    t0 = RANGE_T[0]
    q.append(qq); tr.append((t0, t0 + 2)); rad.append(R)
    for t, (kind, side) in zip(RANGE_T, (("cons_range_in", 1), ("cons_range_in", 1), ("cons_range_end", 0))):
        b.x[t % 4, t, :2] = p
        b.labels.append(Label(kind, t % 4, t, side, dist_ulps(p, qq), True))
    # rows 0 and 63: an active point each, which must come back 0
    b.ends((0.0, 0.0))
    for t in (0, H - 1):
        q.append(_f32(0, 0.0625)); tr.append((t, t + 1)); rad.append(R)
    grp = O.ConstraintGroup(q=torch.from_numpy(np.stack(q)), t_range=torch.tensor(tr, dtype=torch.float32),
                            radius=torch.from_numpy(np.asarray(rad, np.float32)), weight=1.0)
    gp = _gp(weight_collision=0.0, weight_smoothness=0.0)
    return Case("constraint", b.x, gp, b.labels, cons=[grp], desc=dict(NO_BASE), term_roundings=13)


def decode_active(delta):
    return (np.abs(np.asarray(delta, np.float64)[..., :2]).max(-1) > 0.25).astype(np.int64)[..., None]


# ---- 4b. one instance in three tables ------------------------------------------------------------------------------------------------
TABLES_N_ALL, TABLES_B = 90, 8                     # 89 slots per robot: more than the 80 compact / 40 general slots the 4-wave kernel stages
TABLES_CARRIERS = (5, 47, 70, 85)                  # the other robots that carry planted points: slots 3 .. 84, in LDS and in L2


def tables_instance(seed=77):
    """-> (paths [90, 64, 2], x [2 * 8, 64, 4], labels): two local robots (ids 0 and 1), eight samples each, and 88 other robots whose path
    points are planted at the radius of a sample point: along an axis at R and R +- 1 ulp, at fma(dx, dx, dy dy) == R|R| and its two fp32
    neighbours, and across an edge of the 15 x 15 cell table (the sample point at 0 and +-1 lattice steps of the edge, the neighbour in the
    next cell at R -+ 1 ulp).  Every other path point is random: a sample point has a few ordinary neighbours as well."""
    rng = np.random.default_rng(seed)
    n, B = TABLES_N_ALL, TABLES_B
    paths = rng.uniform(-0.9, 0.9, (n, H, 2)).astype(np.float32)
    x = np.zeros((2 * B, H, D), np.float32)
    x[..., :2] = (np.floor(rng.uniform(-0.7, 0.7, (2 * B, H, 2)) * 2 ** 22) / 2 ** 22).astype(np.float32)      # lattice points
    # row 63 of every trajectory next to another robot's last point: active, and it must come back 0 (the table has no time step 0)
    x[:, H - 1, :2] = (np.floor((paths[10, H - 1] + np.float32(0.03)) * 2 ** 22) / 2 ** 22).astype(np.float32)
    labels, k = [], 0
    d2 = {}
    for s in (-1, 0, 1):
        dx, dy, miss = _search_offset(2.3, lambda a, c: np.abs(F.fma_f32(a, a, c * c).astype(np.float64) - float(ulps(R2, s))))
        assert miss == 0.0
        d2[s] = _f32(dx, dy)
    edge = -1.0 + 8 * 2.0 / 15                                          # between cells 7 and 8 of the cell table
    plants = [("tables_axis", _f32(0, 0), _f32(ulps(R, s), 0) * sign, s) for s in (-1, 0, 1) for sign in (1, -1)]
    plants += [("tables_axis", _f32(0, 0), _f32(0, ulps(R, s)), s) for s in (-1, 0, 1)]
    plants += [("tables_d2", _f32(0, 0), d2[s], s) for s in (-1, 0, 1)]
    plants += [("tables_bin_edge", _f32(lattice(edge, s), lattice(0.01)), _f32(ulps(R, -r), 0), s) for s in (-1, 0, 1) for r in (-1, 1)]
    for kind, p, d, s in plants:
        for rep in range(2):                                            # each plant twice: two carriers, both local robots
            j = TABLES_CARRIERS[k % len(TABLES_CARRIERS)]
            traj, t = (k % 2) * B + (k // 2) % B, T_ORDER[(k // 2) % len(T_ORDER)]
            while any(lb.t == t for lb in labels):                     # one plant per time step: no other planted point near this one
                t = T_ORDER[(T_ORDER.index(t) + 1) % len(T_ORDER)]
            qq = (p - d).astype(np.float32)
            assert np.array_equal(p - qq, d)
            x[traj, t, :2] = p
            paths[j, t] = qq
            du = dist_ulps(p, qq)
            labels.append(Label(kind, traj, t, int(du <= 0), du, kind != "tables_d2", None, j))      # (along an axis the decision is exact)
            k += 1
    return paths, x, labels


# ---- 5. extra objects in the guide ---------------------------------------------------------------------------------------------------
def extras_case():
    """extra_sdf<false> against O.extra_objects_sdf (primitives.py:108-115, :326-333, :554-572) at its ties.  torch's sub-gradients there: the
    norm at 0 has gradient 0; min over objects takes the first minimum; amax over (qx, qy) at qx == qy splits 1/2 : 1/2; minimum(max_q, 0)
    at max_q == 0 splits 1/2 : 1/2 with the constant; |dx| at dx == 0 has gradient 0.
    A position is a multiple of 2^-24, rad = 0.15 min(size) is not: the first box's centre is (rad, rad), size (1/8, 1/8), so that at
    p = 1/16 the fp32 q = (|p - c| - half) + rad is exactly 0 (every step exact), and qx == qy on the diagonal by symmetry; the second box
    has a lattice centre, for dx == 0."""
    spheres = np.array([[-0.5, 0.5, 0.125], [-0.5625, -0.25, 0.0625], [-0.4375, -0.25, 0.0625]], np.float32)
    rad = np.float32(0.125) * np.float32(0.15)
    boxes = np.array([[rad, rad, 0.125, 0.125], [0.5, -0.5, 0.125, 0.25]], np.float32)            # (cx, cy, size x, size y)
    dx = np.float32(np.float32(0.0625) - rad)
    assert np.float32(np.float32(dx - np.float32(0.0625)) + rad) == 0 and float(dx) == 0.0625 - float(rad)
    b = _Batch(4, (lattice(0.5), lattice(0.9)))                        # neutral: away from every object by more than the margin
    for rep in range(2):
        b.plant((-0.5, 0.5), "extra_sphere_centre", 1, 0)
        b.plant((-0.5, lattice(-0.25 + 0.03 * (rep + 1))), "extra_two_spheres_tie", 1, 0)         # |dx| = 1/16 to both: the first sphere wins
        for k in (-1, 0, 1):                                           # max q = qx = 0 at k lattice steps, qy < 0: the inside / outside switch
            b.plant((lattice(0.0625, k), lattice(0.01 * (rep + 1))), "extra_box_switch", int(k <= 0), k)
        b.plant((lattice(0.03125), lattice(0.03125)), "extra_box_qx_eq_qy", 1, 0)
        b.plant((lattice(-0.01), lattice(-0.01)), "extra_box_qx_eq_qy", 1, 0)
        b.plant((0.5, lattice(-0.5 + 0.125 + 0.05)), "extra_box_dx0", 1, 0)                        # dx = 0 outside, above the second box
        b.plant((0.5, lattice(-0.5 + 0.03)), "extra_box_dx0", 1, 0)                                # dx = 0 inside, qx > qy: gradient 0
        b.plant((lattice(0.0625 + 0.04), lattice(0.0625 + 0.05)), "extra_box_corner", 1, 0)      # both q > 0: the rounded corner
    b.ends((-0.5, lattice(0.55)))
    gp = _gp(weight_collision=1.0, weight_smoothness=0.0, extra_spheres=torch.from_numpy(spheres), extra_boxes=torch.from_numpy(boxes), **_FAR_WS)
    return Case("extras", b.x, gp, b.labels, desc=dict(OBJ_ONLY), extra_objects=dict(spheres=spheres.tolist(), boxes=boxes.tolist()),
                term_roundings=16)          # T: the box's |d| - half + rad, the squares, root and quotient (8) in front of the clip's 8


# ---- 6. clip rules -------------------------------------------------------------------------------------------------------------------
def _planted_gradient_case(name, values, gp_kw=None, desc_kw=None, **kw):
    """a 16 x 16 grid (sdf = 0: active) whose cell s holds the gradient values[s], one planted point per cell centre"""
    nx, ny = HINGE_N
    tex = np.zeros((1, nx, ny, 4), np.float32)
    b = _Batch(4, (lattice(-1 + 0.5 * 2 / nx), lattice(-1 + 0.5 * 2 / ny)))           # cell (0, 0): gradient 0
    for rep in range(2):
        for s, (gx, gy, kind, side, k) in enumerate(values):
            ix, iy = 1 + s % (nx - 1), 1 + (s // (nx - 1)) % (ny - 1)
            tex[0, ix, iy, 1], tex[0, ix, iy, 2] = gx, gy
            b.plant((lattice(-1 + (ix + 0.5) * 2 / nx), lattice(-1 + (iy + 0.5) * 2 / ny)), kind, side, k)
    ix, iy = 1, 1
    b.ends((lattice(-1 + (ix + 0.5) * 2 / nx), lattice(-1 + (iy + 0.5) * 2 / ny)))
    gp = _gp(sdf_grids=_grids(tex), weight_collision=1.0, weight_smoothness=0.0, **_FAR_WS, **(gp_kw or {}))
    return Case(name, b.x, gp, b.labels, desc=dict(OBJ_ONLY, **(desc_kw or {})), tex=tex, **kw)


def clip_value_case(max_value=0.1):
    """rule 1: a component at max_grad_value and one ulp either side, both signs, the other component inside / outside"""
    m = np.float32(max_value)
    vals = [(s * ulps(m, k), o, "clip_value", int(k > 0), k) for k in (-1, 0, 1) for s in (1, -1) for o in (np.float32(0.03125), np.float32(-0.75))]
    vals += [(o, s * ulps(m, k), "clip_value", int(k > 0), k) for k in (-1, 0, 1) for s in (1, -1) for o in (np.float32(0.0),)]
    return _planted_gradient_case("clip_value", vals, clip_rule="value", max_grad_value=float(m), term_roundings=0)


def clip_norm_case(max_norm=0.25):
    """rule 0: ||g + 1e-6|| at max_norm and a few ulps either side (a value check: the rule is continuous)"""
    gx0 = np.float32(max_norm - 1e-6)
    vals = [(s * ulps(gx0, k), np.float32(0), "clip_norm", int(k > 0), k) for k in (-2, -1, 0, 1, 2) for s in (1, -1)]
    g45 = np.float32((max_norm - 1.5e-6) / np.sqrt(2.0))
    vals += [(ulps(g45, k), ulps(g45, -k), "clip_norm", int(k > 0), k) for k in (-2, -1, 0, 1, 2)]
    return _planted_gradient_case("clip_norm", vals, gp_kw=dict(max_grad_norm=float(max_norm)), desc_kw=dict(max_grad_norm=float(max_norm)))


def clip_off_case(n_coincident=40):
    """clip_grad = False on a group sum of 40 coincident unit vectors: the value is 40, not 1.  T per unit of the sum's size: 5 u for each
    unit vector (value_bound), the four fma chains of ten round at most u (1 + 2 + .. + 10) each, 5.5 u of 40, and the two-level total 3 u:
    T = 14."""
    b = _Batch(4, NEUTRAL, one_per_t=True)
    q, tr = [], []
    for k, phi in enumerate((0.0, 0.5 * np.pi, 0.3, 2.5, 4.0, 5.5)):
        d = _f32(0.0625 * np.cos(phi), 0.0625 * np.sin(phi))
        _, t = b.plant(_f32(0, 0), "clip_off_sum", 1, n_coincident)
        q += [(-d).astype(np.float32)] * n_coincident
        tr += [(t, t + 1)] * n_coincident
    b.ends((0.0, 0.0))
    for t in (0, H - 1):
        q.append(_f32(0, 0.0625)); tr.append((t, t + 1))
    grp = O.ConstraintGroup(q=torch.from_numpy(np.stack(q)), t_range=torch.tensor(tr, dtype=torch.float32),
                            radius=torch.full((len(q),), float(R)), weight=1.0)
    gp = _gp(weight_collision=0.0, weight_smoothness=0.0)
    return Case("clip_off", b.x, gp, b.labels, cons=[grp], desc=dict(NO_BASE), clip_rule=None, term_roundings=14)


# ---- twenty iterations ---------------------------------------------------------------------------------------------------------------
def walking_case():
    """The cell-encoding grid with a start that walks across cell edges: in cell (ix, iy) a step moves the point by -(ix, iy) / 1024, so a
    point a few steps above an edge crosses it mid-chain and the decision changes."""
    c = cell_case()
    b = _Batch(4, (0.0, 0.0))
    lo, hi, n = CELL_LO, CELL_HI, CELL_N
    for ix, iy, fx, fy in ((8, 20, 0.5, 0.1), (16, 10, 0.1, 0.5), (2, 3, 0.7, 0.4), (12, 30, 0.01, 0.01), (1, 1, 0.8, 0.9)):     # cell, start inside it
        b.plant((lattice(lo[0] + (ix + fx) * (hi[0] - lo[0]) / n[0]), lattice(lo[1] + (iy + fy) * (hi[1] - lo[1]) / n[1])), "walk", 0, 0)
    c.name, c.x, c.labels = "cell_walk", b.x, b.labels
    return with_far_group(c)


FAR_SLOTS = 41                                     # one more than the 40 general slots a 4-wave workgroup stages


def far_group():
    """A constraint group that can never act: 41 coincident points far outside the workspace, every time step, weight 1.  With it a robot
    HAS a constraint table, so a launch takes the kernels the product takes -- the cooperative kernel up to 512 trajectories, the 8-wave
    kernel (more than 40 slots, samples a multiple of 8) or the 4-wave kernel with 40 slots in LDS and the rest from L2 -- and the term
    under test is read back from each of them.  The group's contribution is w * clip(0) = 0 exactly."""
    n = FAR_SLOTS
    return O.ConstraintGroup(q=torch.full((n, 2), 50.0), t_range=torch.tensor([[0.0, float(H)]] * n), radius=torch.full((n,), float(R)), weight=1.0)


def with_far_group(case):
    case.cons = list(case.cons) + [far_group()]
    return case


def single_term_cases():
    margin = _gp().margin
    return [with_far_group(c) for c in (cell_case(), cell_real_case(), hinge_case(margin), hinge_extra_case(margin), wall_case(margin),
                                        constraint_case(), extras_case(), clip_value_case(), clip_norm_case(), clip_off_case())]
