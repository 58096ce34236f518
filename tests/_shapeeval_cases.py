"""The inputs tests/test_gpu_shapeeval.py evaluates on the device, shared with tests/test_shapeeval.py, which asserts without a
GPU that their loops complete within the caps the GPU test uses (so the GPU test cannot hide an unfinished loop behind a cap)."""
import numpy as np

from sph3d_gcn_amd.harness import objfeed

SIZES = [1, 2, 37, 255, 256, 257, 400, 700]        # N = 256: both sides of N, of a workgroup's 256 rows, and tiny shapes
NUM_POINT, BATCH, SEED = 256, 3, 5                 # batch 3: the last batch (2 shapes) is smaller
MIN_COUNT, MAX_PASSES = 3, 128
DEFAULT_SIZES = [300, 1, 150]                      # one batch of shapes with n <= 300 at the default min_count = 11
DEFAULT_MAX_PASSES = 256
# a one-hot model over 16 categories with 50 parts in all (ShapeNet's layout: 2 to 6 consecutive parts per category)
PART_N = np.array([4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3], dtype=np.int32)
PART_LO = np.concatenate(([0], np.cumsum(PART_N)[:-1])).astype(np.int32)


def shapes(sizes, seed, C, category=None):
    """-> (shape_blocks rows per shape, category [P]).  With `category` None: a per-category model, labels in [0, C), category 0;
    else labels inside the category's range of the one-hot table — except that every 11th row's label lies outside it"""
    rng = np.random.RandomState(seed)
    out = []
    category = np.zeros((len(sizes),), np.int32) if category is None else np.asarray(category, dtype=np.int32)
    for k, n in enumerate(sizes):
        xyz = (rng.rand(n, 3) * 2.0 - 1.0).astype(np.float32)
        if C == int(PART_N.sum()):
            lo, pn = int(PART_LO[category[k]]), int(PART_N[category[k]])
            lab = lo + rng.randint(0, pn, n)
            lab[::11] = (lab[::11] + pn) % C
        else:
            lab = rng.randint(0, C, n)
        out.append(objfeed.shape_blocks(xyz, lab))
    return out, category
