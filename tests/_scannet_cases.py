"""The inputs tests/test_gpu_scaneval.py evaluates on the device, shared with tests/test_scannet.py, which asserts without a GPU
that their loops complete within the caps the GPU tests use (so a GPU test cannot pass by running out of passes), and the toy
"network" both sides compute: small-integer logits that are a function of (pool row, view, class), so every fp32 vote sum is exact."""
import numpy as np

from sph3d_gcn_amd.harness import evalvote, scannet, scenemerge, scenesynth

C = scannet.NUM_CLASSES
NUM_POINT, BATCH, SEED, MAX_PASSES = 64, 4, 11, 256
SIZES = [20, 64, 300, 65, 150, 37]                 # N = 64: both sides of N and n == N; batches of 4: the last one has 2 blocks
EMPTY_IDS = [2, -1, 0]                             # a batch with an id outside the pool, run as batch 7
EMPTY_BATCH_INDEX = 7
VIEW_IDS, VIEW_BATCH_INDEX = [2, 4, 1], 3          # the batch of the test that looks at the views the model is handed
SCENE_SEED, SCENE_BATCH = 5, 3


def number_rows(blocks):
    """column 3 (the first rgb channel) := the row's position in the pool, columns 4:6 := 0: the feed copies rgb into every view
    bit for bit, so a model_fn can read which pool row it is looking at, whatever the view did to xyz"""
    lo = 0
    for blk in blocks:
        blk[:, 3] = np.arange(lo, lo + len(blk), dtype=np.float32)
        blk[:, 4:6] = 0.0
        lo += len(blk)
    return blocks


def blocks(sizes=SIZES, seed=3):
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        blk = np.zeros((n, 8), dtype=np.float32)
        blk[:, 0:3] = rng.rand(n, 3) * 1.5
        blk[:, 6], blk[:, 7] = rng.randint(0, C, n), rng.rand(n) < 0.7
        blk[0, 7] = 1
        out.append(blk)
    return number_rows(out)


def toy_logits(row, view):
    """row [...] int64 pool rows, view: int -> logits [..., C] float32, integers in [-5, 5]"""
    c = np.arange(C, dtype=np.int64)
    return (((np.asarray(row, dtype=np.int64)[..., None] * 7 + int(view) * 13 + c * 5) % 11) - 5).astype(np.float32)


def logits_fn(offsets, batch_ids, views=3):
    """-> logits_fn(batch_index, q, index) of the statement: the toy on pool row = offsets[block] + index, view = q % views;
    batch_ids(batch_index) -> the batch's block ids"""
    def fn(i, q, index):
        ids = np.asarray(batch_ids(i), dtype=np.int64)
        base = np.array([offsets[k] if 0 <= k < len(offsets) - 1 else 0 for k in ids], dtype=np.int64)
        row = np.where(index >= 0, base[:, None] + index, 0)
        return toy_logits(row, q % views)
    return fn


def scenes():
    """two tiny synthetic scenes cut into overlapping blocks -> (blocks, index, scene_of_block, [scenemerge.Scene])"""
    out_blocks, index, sob, sc = [], [], [], []
    for s, (n, ext) in enumerate(((420, (1.7, 1.6, 1.0)), (260, (1.6, 1.2, 0.8)))):
        full_xyz, full_label, vx, vl = scenesynth.synthetic_scene(40 + s, n, extent=ext, voxel=0.1, num_cls=C)
        blk, idx = scenesynth.split_scene(vx, vl)
        out_blocks += blk
        index += idx
        sob += [s] * len(blk)
        sc.append(scenemerge.Scene(vx, vl, full_xyz, full_label))
    return number_rows(out_blocks), index, sob, sc


def scene_batch_ids(sob, batch_size=SCENE_BATCH):
    """batch_index -> block ids under scenemerge.scene_plan"""
    first_block, first_batch = scenemerge.scene_plan(sob, int(max(sob)) + 1, batch_size)
    table = {}
    for s in range(len(first_block) - 1):
        for j, ids in enumerate(scenemerge.scene_batches(first_block, s, batch_size)):
            table[int(first_batch[s]) + j] = ids
    return table


def pool_batch_ids(i, sizes=SIZES, batch=BATCH):
    return EMPTY_IDS if i == EMPTY_BATCH_INDEX else evalvote.batch_blocks(len(sizes), batch, i)
