"""Occupancy maps (environments.register_occupancy_map): the models the tests hold the definition and the kernels to.

  brute_nearest    the definition's nearest site by brute force over all sites in lexicographic order (small grids);
  brute_texture    the texture on top of it, in float64-free fp32 steps written independently of environments.occupancy_sdf_texture;
  kernel_texture   the two kernels' operation sequence (csrc/sdf_grid.hip: occupancy_rows_kernel, occupancy_sdf_kernel) in numpy:
                   the outward walk per row, the ascending jx loop with a strict <, then the fp32 sequence;
  test_occupancy   the 400 x 400 test map (golden g26 holds scipy's distance transform of it);
  tie_mask         the cells whose nearest site is not unique."""
import numpy as np

NONE = 1 << 14


def brute_nearest(site):
    """(D2, jx, jy) [nx, ny] of every cell's nearest True cell of `site`: minimal D2, the lexicographically smallest (jx, jy) among equal
    D2 (np.argwhere lists the sites in that order and argmin takes the first minimum)."""
    nx, ny = site.shape
    js = np.argwhere(site)
    c = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 1, 2)
    d2 = ((c - js[None]) ** 2).sum(-1)
    k = d2.argmin(1)
    return d2[np.arange(len(k)), k].reshape(nx, ny), js[k, 0].reshape(nx, ny), js[k, 1].reshape(nx, ny)


def brute_texture(occ, cell):
    """The definition, cell by cell, on top of brute_nearest."""
    occ = np.asarray(occ) != 0
    f = np.float32
    cell = f(cell)
    nx, ny = occ.shape
    tex = np.zeros((nx, ny, 4), f)
    if not occ.any() or occ.all():
        tex[..., 0] = f(-1) if occ.all() else f(1)
        return tex
    to_occ, to_free = brute_nearest(occ), brute_nearest(~occ)
    for ix in range(nx):
        for iy in range(ny):
            d2, jx, jy = (t[ix, iy] for t in (to_free if occ[ix, iy] else to_occ))
            s = np.sqrt(f(d2))
            v = f(f(cell * s) - f(f(0.5) * cell))
            if occ[ix, iy]:
                tex[ix, iy, :3] = (-v, f(jx - ix) / s, f(jy - iy) / s)
            elif v < 1:
                tex[ix, iy, :3] = (v, f(ix - jx) / s, f(iy - jy) / s)
            else:
                tex[ix, iy, 0] = 1
    return tex


def row_offsets_of(want):
    """The outward walk of occupancy_rows_kernel for one class: per cell the signed iy offset to the row's nearest True cell of `want`,
    the smaller jy first at each distance; NONE where the row holds none."""
    nx, ny = want.shape
    off = np.full((nx, ny), NONE, np.int32)
    for d in range(ny):
        # cell iy looks at iy - d (cells [d, ny) look at [0, ny - d)), then at iy + d (cells [0, ny - d) look at [d, ny))
        for cells, seen, value in ((slice(d, ny), slice(0, ny - d), -d), (slice(0, ny - d), slice(d, ny), d)):
            view = off[:, cells]
            view[want[:, seen] & (view == NONE)] = value
        if not (off == NONE).any():
            break
    return off


def row_offsets(occ):
    """occupancy_rows_kernel's two tables: to the nearest occupied and to the nearest free cell of the row."""
    occ = np.asarray(occ) != 0
    return row_offsets_of(occ), row_offsets_of(~occ)


def kernel_texture(occ, cell):
    """occupancy_sdf_kernel on the tables of row_offsets, the same operations in the same order."""
    occ = np.asarray(occ) != 0
    f = np.float32
    cell = f(cell)
    nx, ny = occ.shape
    to_occ, to_free = row_offsets(occ)
    ix = np.arange(nx, dtype=np.int32)[:, None]
    best = np.full((nx, ny), np.iinfo(np.int32).max, np.int32)
    bdx, bdy = np.zeros((nx, ny), np.int32), np.zeros((nx, ny), np.int32)
    for jx in range(nx):
        dy = np.where(occ, to_free[jx][None, :], to_occ[jx][None, :])
        dx = np.int32(jx) - ix
        d2 = dx * dx + dy * dy
        m = d2 < best
        best, bdx, bdy = np.where(m, d2, best), np.where(m, dx, bdx), np.where(m, dy, bdy)
    none = best >= NONE * NONE
    s = np.sqrt(np.where(none, 1, best).astype(f))
    v = cell * s - f(0.5) * cell
    tex = np.zeros((nx, ny, 4), f)
    capped = ~occ & ~(v < f(1))
    tex[..., 0] = np.where(none, np.where(occ, f(-1), f(1)), np.where(occ, -v, np.where(capped, f(1), v)))
    zero = none | capped
    tex[..., 1] = np.where(zero, f(0), np.where(occ, bdx, -bdx).astype(f) / s)
    tex[..., 2] = np.where(zero, f(0), np.where(occ, bdy, -bdy).astype(f) / s)
    return tex


def tie_mask(occ):
    """[nx, ny] bool: the cell's nearest cell of the other class is not unique (the tie rule decides its gradient)."""
    occ = np.asarray(occ) != 0
    nx, ny = occ.shape
    ix = np.arange(nx, dtype=np.int64)[:, None]
    out = np.zeros((nx, ny), bool)
    for own in (~occ, occ):
        site = ~own
        lo = row_offsets_of(site)
        hi = -row_offsets_of(site[:, ::-1])[:, ::-1]                 # a tie to the LARGER jy
        hi[np.abs(hi) >= NONE] = NONE
        best = np.full((nx, ny), np.iinfo(np.int64).max)
        count = np.zeros((nx, ny), np.int64)
        for jx in range(nx):
            d2 = (ix - jx) ** 2 + lo[jx].astype(np.int64)[None, :] ** 2
            n = 1 + (lo[jx] != hi[jx])[None, :]
            count = np.where(d2 < best, n, np.where(d2 == best, count + n, count))
            best = np.minimum(best, d2)
        out |= own & (count > 1) & (best < NONE * NONE)
    return out


def test_occupancy():
    """The 400 x 400 test map, [ix, iy] uint8: rasterised boxes and a disc, a one-cell-thick wall with a one-cell gap, isolated single
    cells, a symmetric pair (and a symmetric quartet) whose mid lines are ties, a box ring that encloses a free pocket, occupied cells
    along an edge and in the corners."""
    n = 400
    occ = np.zeros((n, n), np.uint8)
    occ[40:120, 60:100] = 1                                    # boxes
    occ[250:330, 40:130] = 1
    occ[180:200, 150:330] = 1
    i = np.arange(n)
    occ[(i[:, None] - 300) ** 2 + (i[None, :] - 280) ** 2 <= 45 ** 2] = 1          # a disc
    occ[20:170, 200] = 1                                       # a wall one cell thick ...
    occ[97, 200] = 0                                           # ... with a gap of one cell
    for c in ((15, 15), (130, 30), (222, 111), (377, 201), (60, 301), (140, 260), (141, 261)):      # single cells (one diagonal pair)
        occ[c] = 1
    occ[230, 350] = occ[230, 370] = 1                          # a symmetric pair: the cells of iy = 360 are tied
    occ[100, 330] = occ[100, 350] = occ[120, 330] = occ[120, 350] = 1              # a quartet: its centre has four nearest sites
    occ[50:110, 230:290] = 1                                   # a ring ...
    occ[60:100, 240:280] = 0                                   # ... around a free pocket
    occ[75, 255] = 1                                           # (with a speck in it)
    occ[0, 100:180] = 1                                        # along an edge
    occ[340:400, 399] = 1
    occ[0, 0] = occ[399, 0] = occ[399, 399] = occ[398, 399] = 1                     # corners
    occ[380:400, 380:400] = 1
    return occ


def small_grids():
    """{name: (occ [nx, ny] uint8, cell)}: the small shapes every layer is held to the brute force on."""
    rng = np.random.Generator(np.random.PCG64(26))
    g = {}
    g["24x40"] = ((rng.random((24, 40)) < 0.05).astype(np.uint8), 0.005)          # nx != ny, 960 cells = 3 workgroups + 192 threads
    g["1x37"] = ((rng.random((1, 37)) < 0.1).astype(np.uint8), 0.005)
    g["37x1"] = ((rng.random((37, 1)) < 0.1).astype(np.uint8), 0.005)
    g["1x1 free"] = (np.zeros((1, 1), np.uint8), 0.005)
    g["1x1 occupied"] = (np.ones((1, 1), np.uint8), 0.005)
    g["checkerboard 16x16"] = ((np.indices((16, 16)).sum(0) % 2 == 0).astype(np.uint8), 0.005)
    corner = np.zeros((7, 5), np.uint8)
    corner[0, 0] = 1
    g["corner 7x5"] = (corner, 0.005)
    for dens in (0.005, 0.5, 0.995):
        g[f"64x64 at {dens}"] = ((rng.random((64, 64)) < dens).astype(np.uint8), 0.005)
    coarse = np.zeros((31, 33), np.uint8)                      # cell 0.13: a free cell 9 or more cells from every obstacle is capped
    coarse[3, 4] = coarse[3, 5] = coarse[4, 4] = coarse[28, 30] = 1
    g["31x33 coarse"] = (coarse, 0.13)
    for name in ("1x37", "37x1", "24x40", "64x64 at 0.005"):
        assert g[name][0].any(), name
    assert not g["64x64 at 0.995"][0].all()
    return g
