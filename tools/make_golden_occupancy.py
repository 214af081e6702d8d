#!/usr/bin/env python
"""tests/golden/g26_occupancy_map.npz: the squared Euclidean distance transform of the occupancy test map (tests/occupancy_model.py::
test_occupancy) by scipy.ndimage.distance_transform_edt, an implementation independent of the project's two-pass form.

    python tools/make_golden_occupancy.py [OUT.npz]

Stored: the map's packed bits; about 8 000 listed nodes -- random ones, nodes whose nearest site is not unique (occupancy_model.tie_mask)
and nodes next to a surface (a neighbour of the other class within two cells); scipy's D2 = rint(edt^2) from each listed node to the
nearest cell of the OTHER class; the int64 sums of D2 over the free and over the occupied cells.  Numeric arrays only."""
import os
import sys

import numpy as np
from scipy.ndimage import binary_dilation, distance_transform_edt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import occupancy_model                                                                         # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "g26_occupancy_map.npz")
    occ = occupancy_model.test_occupancy().astype(bool)
    # distance_transform_edt: for every non-zero cell the distance to the nearest zero cell
    d2_free = np.rint(distance_transform_edt(~occ) ** 2).astype(np.int64)       # free cells: to the nearest occupied one
    d2_occ = np.rint(distance_transform_edt(occ) ** 2).astype(np.int64)         # occupied cells: to the nearest free one
    d2 = np.where(occ, d2_occ, d2_free)
    rng = np.random.Generator(np.random.PCG64(26))
    pick = np.zeros(occ.shape, bool)
    pick.reshape(-1)[rng.choice(occ.size, 3000, replace=False)] = True
    ties = np.argwhere(occupancy_model.tie_mask(occ))
    pick[tuple(ties[rng.choice(len(ties), min(len(ties), 2000), replace=False)].T)] = True
    ring = np.argwhere(binary_dilation(occ, iterations=2) & binary_dilation(~occ, iterations=2))
    pick[tuple(ring[rng.choice(len(ring), min(len(ring), 3000), replace=False)].T)] = True
    idx = np.argwhere(pick).astype(np.uint16)
    np.savez_compressed(out, shape=np.asarray(occ.shape, np.int32), bits=np.packbits(occ), idx=idx,
                        d2=d2[idx[:, 0], idx[:, 1]].astype(np.int32), sum_d2_free=np.int64(d2_free[~occ].sum()),
                        sum_d2_occupied=np.int64(d2_occ[occ].sum()))
    print(f"{out}: {len(idx)} nodes ({len(ties)} tie nodes, {len(ring)} surface nodes on the map), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
