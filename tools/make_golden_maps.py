#!/usr/bin/env python
"""Generate tests/golden/g25_custom_map.npz by running the GENUINE reference (tools/ref_bootstrap.py): an EnvBase whose fixed objects
are ONE ObjectField([MultiSphereField, MultiBoxField]) of the custom-map test map (tests/sdf_grid_model.py::tie_map), with and without
its spheres, and GridMapSDF.precompute_sdf's grid of it (grid_map_sdf.py:34-63).  Stored per variant: the primitives, the grid's shape,
two float64 checksums, and value and gradient at the listed nodes -- 4096 seeded random ones, every tie node of the map
(sdf_grid_model.tie_masks) and a ring of nodes around each primitive's surface.  Numeric arrays only; no reference code is stored.

    python tools/make_golden_maps.py            # rewrites tests/golden/g25_custom_map.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

from ref_harness import TENSOR_ARGS, quiet                                                     # noqa: E402
from torch_robotics.environments.env_base import EnvBase                                       # noqa: E402
from torch_robotics.environments.primitives import MultiBoxField, MultiSphereField, ObjectField  # noqa: E402

import sdf_grid_model                                                                          # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
RING = 0.006            # |distance to a primitive's surface| below this: about one cell (0.005) either side
MAX_TIE_NODES = 1500    # per tie kind (the two identical spheres tie on every node where they are the minimum)


def reference_grid(boxes, spheres):
    sph = np.asarray(spheres, np.float32).reshape(-1, 3)
    box = np.asarray(boxes, np.float32).reshape(-1, 4)
    fields = [MultiSphereField(sph[:, :2] if len(sph) else np.array([]), sph[:, 2] if len(sph) else np.array([]), tensor_args=TENSOR_ARGS),
              MultiBoxField(box[:, :2], box[:, 2:], tensor_args=TENSOR_ARGS)]
    with quiet():
        env = EnvBase(name="CustomMap", limits=torch.tensor([[-1, -1], [1, 1]], **TENSOR_ARGS),
                      obj_fixed_list=[ObjectField(fields, "custom_map")], precompute_sdf_obj_fixed=True, sdf_cell_size=0.005,
                      tensor_args=TENSOR_ARGS)
    g = env.grid_map_sdf_obj_fixed
    return g.sdf_tensor.numpy(), g.grad_sdf_tensor.numpy()


def listed_nodes(boxes, spheres, rng):
    xs, ys = sdf_grid_model.node_rows()
    nodes = [rng.integers(0, 400, size=(4096, 2))]
    for mask in sdf_grid_model.tie_masks(boxes, spheres, xs, ys).values():
        idx = np.argwhere(mask)
        nodes.append(idx if len(idx) <= MAX_TIE_NODES else idx[rng.choice(len(idx), MAX_TIE_NODES, replace=False)])
    for d, _, _, _ in sdf_grid_model.primitive_terms(boxes, spheres, xs, ys):
        nodes.append(np.argwhere(np.abs(d) < RING))
    return np.unique(np.concatenate(nodes), axis=0)


def main():
    out = {}
    rng = np.random.Generator(np.random.PCG64(25))
    for variant, with_spheres in (("with_spheres", True), ("no_spheres", False)):
        boxes, spheres = sdf_grid_model.tie_map(with_spheres)
        sdf, grad = reference_grid(boxes, spheres)
        idx = listed_nodes(boxes, spheres, rng)
        out[f"{variant}.boxes"] = np.asarray(boxes, np.float32).reshape(-1, 4)
        out[f"{variant}.spheres"] = np.asarray(spheres, np.float32).reshape(-1, 3)
        out[f"{variant}.shape"] = np.array(sdf.shape)
        out[f"{variant}.sum_sdf"] = np.float64(sdf.astype(np.float64).sum())
        out[f"{variant}.sum_abs_grad"] = np.float64(np.abs(grad.astype(np.float64)).sum())
        out[f"{variant}.idx"] = idx.astype(np.int32)
        out[f"{variant}.sdf"] = sdf[idx[:, 0], idx[:, 1]]
        out[f"{variant}.grad"] = grad[idx[:, 0], idx[:, 1]]
        print(variant, "grid", sdf.shape, "listed nodes", len(idx))
    path = os.path.join(OUT, "g25_custom_map.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
