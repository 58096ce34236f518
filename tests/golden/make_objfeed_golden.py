"""Generate tests/golden/objfeed_ref.npz: inputs, the random numbers numpy handed out, and the outputs of the REFERENCE's own
augmentation functions (utils/data_util.py: rotate_point_cloud, rotate_perturbation_point_cloud, random_scale_point_cloud,
shift_point_cloud, jitter_point_cloud) on a [4, 16, 3] float32 batch, so that ``sph3d_gcn_amd/harness/objfeed.py``'s float64
transform can be pinned against them (tests/test_objfeed.py).

Runs in the build container only (it reads /root/reference at run time; nothing of it is copied here): data_util.py is pure numpy
and is imported as it is.  While a function runs, np.random.uniform and np.random.randn are wrapped so that what they return is
recorded; the fixture holds data only.

    python tests/golden/make_objfeed_golden.py          # writes tests/golden/objfeed_ref.npz
"""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
FUNCTIONS = (("rotate_point_cloud", 41), ("rotate_perturbation_point_cloud", 42), ("random_scale_point_cloud", 43),
             ("shift_point_cloud", 44), ("jitter_point_cloud", 45))


class Recorder:
    """np.random.uniform / randn, recording every value they hand out"""

    def __init__(self):
        self.handed = []
        self._uniform, self._randn = np.random.uniform, np.random.randn

    def __enter__(self):
        def uniform(*a, **k):
            v = self._uniform(*a, **k)
            self.handed.append(np.asarray(v, dtype=np.float64).reshape(-1))
            return v

        def randn(*a):
            v = self._randn(*a)
            self.handed.append(np.asarray(v, dtype=np.float64).reshape(-1))
            return v
        np.random.uniform, np.random.randn = uniform, randn
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.randn = self._uniform, self._randn
        return False


def main():
    sys.path.insert(0, os.path.join(REF, "utils"))
    import data_util                                           # the reference's module, unmodified
    xyz = (np.random.RandomState(2025).rand(4, 16, 3) * 2.0 - 1.0).astype(np.float32)
    out = {"xyz": xyz}
    for name, seed in FUNCTIONS:
        np.random.seed(seed)
        with Recorder() as rec:
            res = getattr(data_util, name)(xyz.copy())
        out[name] = np.asarray(res)
        out[name + "_random"] = np.concatenate(rec.handed)
        out[name + "_seed"] = np.int64(seed)
    path = os.path.join(HERE, "objfeed_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items() if hasattr(v, "shape")})


if __name__ == "__main__":
    main()
