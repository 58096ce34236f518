"""Generate tests/golden/facade_ref.npz: the input, the random numbers numpy handed out, and the outputs of the REFERENCE's own
with-normal augmentation functions (utils/data_util.py:64-105: rotate_point_cloud_with_normal,
rotate_perturbation_point_cloud_with_normal) on a [4, 16, 6] float32 batch (xyz, unit normal), so that
``sph3d_gcn_amd/harness/facadefeed.py``'s float64 transform of xyz and normal can be pinned against them
(tests/test_facadefeed.py).

The reference tree is read at generation time only (nothing of it is copied here): data_util.py is pure numpy and is imported as
it is.  While a function runs, np.random.uniform and np.random.randn are wrapped so that what they return is recorded; the fixture
holds arrays only.

    python tests/golden/make_facade_golden.py REFERENCE_ROOT          # writes tests/golden/facade_ref.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_objfeed_golden import Recorder  # noqa: E402

FUNCTIONS = (("rotate_point_cloud_with_normal", 51), ("rotate_perturbation_point_cloud_with_normal", 52))


def main(reference_root):
    sys.path.insert(0, os.path.join(reference_root, "utils"))
    import data_util                                           # the reference's module, unmodified
    rng = np.random.RandomState(2026)
    xyz = rng.rand(4, 16, 3) * 2.0 - 1.0
    normal = rng.randn(4, 16, 3)
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    batch = np.concatenate((xyz, normal), axis=2).astype(np.float32)
    out = {"xyz_normal": batch}
    for name, seed in FUNCTIONS:
        np.random.seed(seed)
        with Recorder() as rec:
            res = getattr(data_util, name)(batch.copy())       # (the first one writes into its argument)
        out[name] = np.asarray(res)
        out[name + "_random"] = np.concatenate(rec.handed)
        out[name + "_seed"] = np.int64(seed)
    path = os.path.join(HERE, "facade_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items() if hasattr(v, "shape")})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
