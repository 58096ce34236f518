"""Batches of the object datasets (ShapeNet parts, ModelNet40) assembled on the device: what shapenet_seg/train_shapenet.py:
121-152 and modelnet40_cls/train_modelnet.py:95-115 do per step on the host, and the two-pass draw of
shapenet_seg/evaluate_shapenet.py:86-94,228-247, as one kernel over a pool of shapes that lives in HBM (csrc/objfeed.hip,
include/sph3d.h: sph3d_objfeed_assemble).

  * ``shape_blocks`` / ``ShapePool``: a shape is a "block" of a ``feed.BlockPool`` — rows [n, 8] with xyz, three zero columns,
    the label and inner == 1 — so the vote kernels read the same pool unchanged; the pool adds the shapes' category and,
    for a one-hot model, the part table;
  * ``assemble_reference``: the SPECIFICATION of the draws, in numpy, no GPU.  The sample draws are ``feed``'s (cloud key,
    PERM, REPL), so ``index`` is a pure function of (seed, step, b, n, N) and does not depend on the recipe: the evaluation
    draws the same sample twice, once plain and once augmented.  The kernel's integer outputs equal this statement bit for
    bit; what it computes in fp32 is held to the project's 1e-5 bound against the float64 evaluation of ``apply_reference``;
  * ``train_recipe`` / ``EVAL_AUGMENT``: the reference's recipes as per-cloud bit masks;
  * ``assemble``: the C entry;  ``ObjectFeed``: one epoch of batches on the feed's own stream (``feed.TwoSetFeed``).

A recipe is a bit mask per cloud, applied in the reference's order (utils/data_util.py:47-61,140-204):
TURN (Rz of a uniform angle, purpose 3), TILT (Rz Ry Rx of three clipped normal angles, purpose 4), SCALE
(s = 0.8 + 0.45 u, purpose 6, counter 0), SHIFT (-0.1 + 0.2 u per axis, purpose 7, counters 0..2), JITTER (clipped normal noise
per point, purpose 5, counters as in feed.py).  A mask of 0 copies xyz.

What differs from the reference's loop, on purpose — as in feed.py: its two shuffles (the shapes of a batch, the point order)
are not separate steps — the shape ids arrive in random order from the epoch plan and the sample is in random order already —
and the random numbers are this project's counter-based ones, not numpy's Mersenne twister.  The arithmetic is the
reference's, checked against its recorded results (tests/test_objfeed.py, tests/golden/objfeed_ref.npz).
"""
import collections

import numpy as np

from . import feed
from .feed import (ANGLE_CLIP, ANGLE_SIGMA, JITTER_CLIP, JITTER_SIGMA, _hi, cloud_key, draw, jitter_noise, tilt_angles,  # noqa: F401
                   tilt_matrix, turn_angle, turn_matrix, uniform)

TURN, TILT, SCALE, SHIFT, JITTER = 1, 2, 4, 8, 16        # the bits of a recipe
ALL = TURN | TILT | SCALE | SHIFT | JITTER
P_SCALE, P_SHIFT = 6, 7                                  # the `purpose` of the two draws feed.py does not have
SCALE_LOW, SCALE_HIGH = 0.8, 1.25                        # utils/data_util.py:193
SHIFT_RANGE = 0.1                                        # utils/data_util.py:179
EVAL_AUGMENT = TILT | SCALE | SHIFT | JITTER             # evaluate_shapenet.py:86-92


# ---------------------------------------------------------------------------------------------------------------
# the draws the feed does not have, and the recipes
# ---------------------------------------------------------------------------------------------------------------
def scale_factor(ck):
    return SCALE_LOW + (SCALE_HIGH - SCALE_LOW) * float(uniform(_hi(draw(ck, P_SCALE, 0))))


def shift_vector(ck):
    return -SHIFT_RANGE + 2.0 * SHIFT_RANGE * uniform(_hi(draw(ck, P_SHIFT, np.arange(3))))


def train_recipe(B, dataset):
    """-> recipe [B] int32 of a training batch.  "shapenet" (train_shapenet.py:136-150): the first B // 3 clouds get all five
    transforms, the next B // 3 scale, shift and jitter, the rest none.  "modelnet" (train_modelnet.py:104-113, augment_ratio
    0.5): the first int(0.5 * B) clouds get turn, tilt, scale and shift, the rest none."""
    B = int(B)
    if B <= 0:
        raise ValueError("train_recipe: B>0 required")
    r = np.zeros((B,), dtype=np.int32)
    if dataset == "shapenet":
        third = B // 3
        r[:third] = ALL
        r[third:2 * third] = SCALE | SHIFT | JITTER
    elif dataset == "modelnet":
        r[:int(0.5 * B)] = TURN | TILT | SCALE | SHIFT
    else:
        raise ValueError("train_recipe: dataset is 'shapenet' or 'modelnet'")
    return r


def check_recipe(recipe, B):
    """-> recipe as int32 [B]; one mask for all clouds is broadcast; masks outside [0, 31] are refused"""
    r = np.asarray(recipe)
    if r.ndim == 0:
        r = np.full((B,), int(r))
    if r.shape != (B,) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("recipe: one integer mask per cloud expected")
    if r.min() < 0 or r.max() > ALL:
        raise ValueError("recipe: masks are in [0, %d]" % ALL)
    return np.ascontiguousarray(r, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "index recipe theta tilt scale shift noise")


def assemble_reference(sizes, shape_ids, num_point, seed, step, recipe):
    """The draws of one batch.  sizes: rows per shape of the pool; shape_ids [B]; recipe: [B] masks, or one for all.
    -> Reference(index [B, N] int32 — feed.assemble_reference's, whatever the recipe; recipe [B] int32;
                 theta [B], tilt [B, 3], scale [B], shift [B, 3], noise [B, N, 3] — float64, the identity values
                 (0, 0, 1, 0, 0) where the cloud's mask does not ask for the transform)
    A pure function of its arguments."""
    shape_ids = np.asarray(shape_ids, dtype=np.int64).reshape(-1)
    B, N = shape_ids.shape[0], int(num_point)
    index = feed.assemble_reference(sizes, shape_ids, N, seed, step, False).index
    recipe = check_recipe(recipe, B)
    theta, tilts = np.zeros((B,)), np.zeros((B, 3))
    scale, shift, noise = np.ones((B,)), np.zeros((B, 3)), np.zeros((B, N, 3))
    for b in range(B):
        ck, m = cloud_key(seed, step, b), int(recipe[b])
        if m & TURN:
            theta[b] = turn_angle(ck)
        if m & TILT:
            tilts[b] = tilt_angles(ck)
        if m & SCALE:
            scale[b] = scale_factor(ck)
        if m & SHIFT:
            shift[b] = shift_vector(ck)
        if m & JITTER:
            noise[b] = jitter_noise(ck, N)
    return Reference(index, recipe, theta, tilts, scale, shift, noise)


def transform(xyz, mask, theta=0.0, tilt=(0.0, 0.0, 0.0), scale=1.0, shift=(0.0, 0.0, 0.0), noise=0.0):
    """one cloud's transform in float64, in the reference's order: xyz [N, 3] -> [N, 3]"""
    xyz = np.asarray(xyz, dtype=np.float64)
    if mask & TURN:
        xyz = np.dot(xyz, turn_matrix(theta))
    if mask & TILT:
        xyz = np.dot(xyz, tilt_matrix(*tilt))
    if mask & SCALE:
        xyz = xyz * scale
    if mask & SHIFT:
        xyz = xyz + np.asarray(shift, dtype=np.float64)
    if mask & JITTER:
        xyz = xyz + noise
    return xyz


def apply_reference(blocks, shape_ids, ref):
    """the batch `ref` describes, from host shapes [n, 8]: -> points [B, N, 3] float64, label [B, N] int32"""
    B, N = ref.index.shape
    points = np.zeros((B, N, 3), dtype=np.float64)
    label = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        rows = np.asarray(blocks[int(shape_ids[b])])[ref.index[b]]
        points[b] = transform(rows[:, 0:3], int(ref.recipe[b]), ref.theta[b], ref.tilt[b], ref.scale[b], ref.shift[b], ref.noise[b])
        label[b] = rows[:, 6].astype(np.int32)
    return points, label


# ---------------------------------------------------------------------------------------------------------------
# the pool
# ---------------------------------------------------------------------------------------------------------------
def shape_blocks(xyz, label):
    """a shape as a block of a feed.BlockPool: xyz [n, 3], label [n] (a scalar: the same for every row, ModelNet's class)
    -> [n, 8] fp32 with columns 3:6 zero, column 6 the label and column 7 equal to 1 (every row is an inner row)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
        raise ValueError("shape_blocks: xyz [n, 3] with n > 0 expected")
    label = np.broadcast_to(np.asarray(label), (xyz.shape[0],)) if np.ndim(label) == 0 else np.asarray(label).reshape(-1)
    if label.shape[0] != xyz.shape[0]:
        raise ValueError("shape_blocks: one label per row expected")
    out = np.zeros((xyz.shape[0], 8), dtype=np.float32)
    out[:, 0:3], out[:, 6], out[:, 7] = xyz, label, 1.0
    return out


def read_class_info(path):
    """The ShapeNet category table (class_info_all.txt of shapenet_seg/evaluate_shapenet_onehot.py:58-62; one line per category,
    four tab-separated columns: name, folder, number of parts, first part among the one-hot model's outputs)
    -> (names [list of str], part_lo int32 [T], part_n int32 [T]): the part table a ShapePool takes."""
    names, lo, n = [], [], []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            if not line.strip():
                continue
            cols = line.rstrip("\r\n").split("\t")
            if len(cols) != 4:
                raise ValueError("%s:%d: four tab-separated columns expected" % (path, number))
            names.append(cols[0])
            n.append(int(cols[2]))
            lo.append(int(cols[3]))
    part_lo, part_n = np.asarray(lo, dtype=np.int32), np.asarray(n, dtype=np.int32)
    if not names or (part_n <= 0).any() or part_lo[0] != 0 or (part_lo[1:] != np.cumsum(part_n)[:-1]).any():
        raise ValueError("%s: the parts of the categories should be consecutive ranges that start at 0" % path)
    return names, part_lo, part_n


class ShapePool:
    """The shapes of a dataset resident on the device: `pool`, a feed.BlockPool of shape_blocks rows; `category` [P] int32 on
    the host and `category_dev` on the device (the ModelNet class or the ShapeNet category); and, for a one-hot model, the
    part table `part_lo` / `part_n` [num_categories] int32 (the consecutive parts of each category among the model's outputs:
    seg_info of evaluate_shapenet_onehot.py:58-60).  Without a table both are None: a per-category model, whose parts start
    at 0."""

    def __init__(self, shapes, category, part_lo=None, part_n=None, device=None):
        import torch
        shapes = [np.asarray(s) for s in shapes]
        for s in shapes:
            if s.ndim != 2 or s.shape[1] != 8 or s[:, 3:6].any() or not (s[:, 7] == 1).all():
                raise ValueError("ShapePool: a shape is shape_blocks' [n, 8]: columns 3:6 zero, column 7 equal to 1")
        self.pool = feed.BlockPool(shapes, device)
        self.category = np.ascontiguousarray(np.asarray(category).reshape(-1), dtype=np.int32)
        if self.category.shape[0] != len(self.pool) or (self.category < 0).any():
            raise ValueError("ShapePool: one non-negative category per shape expected")
        if (part_lo is None) != (part_n is None):
            raise ValueError("ShapePool: part_lo and part_n come together")
        self.part_lo = self.part_n = None
        if part_lo is not None:
            self.part_lo = np.ascontiguousarray(np.asarray(part_lo).reshape(-1), dtype=np.int32)
            self.part_n = np.ascontiguousarray(np.asarray(part_n).reshape(-1), dtype=np.int32)
            if self.part_lo.shape != self.part_n.shape or (self.part_lo < 0).any() or (self.part_n <= 0).any():
                raise ValueError("ShapePool: a part table has part_lo >= 0 and part_n > 0 per category")
            if self.category.max() >= self.part_lo.shape[0]:
                raise ValueError("ShapePool: a shape's category is outside the part table")
        self.category_dev = torch.from_numpy(self.category).to(self.pool.device)

    @classmethod
    def from_arrays(cls, xyz, label, category, part_lo=None, part_n=None, device=None):
        """xyz: per shape [n, 3]; label: per shape [n] part labels, or a scalar (ModelNet: the class on every row)"""
        return cls([shape_blocks(x, l) for x, l in zip(xyz, label)], category, part_lo, part_n, device)

    # the BlockPool's face, so that a ShapePool can stand where the scene pipeline takes a pool
    rows = property(lambda self: self.pool.rows)
    offsets = property(lambda self: self.pool.offsets)
    sizes = property(lambda self: self.pool.sizes)
    host_offsets = property(lambda self: self.pool.host_offsets)
    device = property(lambda self: self.pool.device)

    def __len__(self):
        return len(self.pool)

    def part_range(self, shape_ids, num_cls):
        """-> (part_lo, part_n) int32 [b] of the shapes (ids outside the pool get the empty range 0, 0)"""
        ids = np.asarray(shape_ids, dtype=np.int64).reshape(-1)
        ok = (ids >= 0) & (ids < len(self))
        lo, n = np.zeros(ids.shape, np.int32), np.zeros(ids.shape, np.int32)
        if self.part_lo is None:
            n[ok] = int(num_cls)
        else:
            cat = self.category[ids[ok]]
            lo[ok], n[ok] = self.part_lo[cat], self.part_n[cat]
        if (lo[ok] + n[ok] > int(num_cls)).any():
            raise ValueError("part table reaches past the model's %d outputs" % int(num_cls))
        return lo, n


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
def assemble(rows, offsets, shape_ids, num_point, seed, step, recipe, out=None, want_index=False):
    """sph3d_objfeed_assemble on torch's current stream.  rows [T, 8] fp32, offsets [P+1] int64, shape_ids [B] int32, all on the
    device.  recipe: a host array of B masks or one mask for all (checked here: masks outside [0, 31] are refused, then
    uploaded), or an int32 device tensor [B] that check_recipe has seen before its upload.
    out: (points [B, N, 3] fp32, label [B, N] i32) to write into, else new tensors.
    -> points, label (and index [B, N] i32 with want_index)"""
    import torch
    from .. import _lib
    B, N, (points, label), index = feed.assemble_args(_lib, rows, offsets, shape_ids, "shape_ids", num_point, out, _OBJ_OUT,
                                                      want_index)
    if torch.is_tensor(recipe):
        _lib.require_device(recipe)
        if recipe.dtype != torch.int32 or tuple(recipe.shape) != (B,) or not recipe.is_contiguous():
            raise ValueError("assemble: a device recipe is a contiguous int32 [B]")
    else:
        recipe = torch.from_numpy(check_recipe(recipe, B)).to(rows.device)
    _lib.check(_lib.lib().sph3d_objfeed_assemble(B, N, int(offsets.shape[0]) - 1, int(rows.shape[0]), _lib.ptr(rows),
                                                 _lib.ptr(offsets), _lib.ptr(shape_ids), seed & 0xffffffffffffffff,
                                                 step & 0xffffffffffffffff, _lib.ptr(recipe), _lib.ptr(points), _lib.ptr(label),
                                                 _lib.ptr(index), _lib.stream_ptr()))
    return (points, label, index) if want_index else (points, label)


_OBJ_OUT = ((3,), ())               # the shapes after [B, N] of points (fp32) and label (int32)


class ObjectFeed(feed.TwoSetFeed):
    """One epoch of training batches of an object dataset per iteration, assembled on the device (feed.TwoSetFeed states the
    protocol and who owns an item's tensors).

        feed = ObjectFeed(pool, 32, 2048, seed=1, dataset="shapenet")
        for points, label, category, ready in feed:              # epoch 0; the next `for` is epoch 1
            pred, _ = model(points, is_training=True, points_ready=ready)
            loss = model.loss(pred, label)
            feed.done(ready)
            ...

    The last, smaller batch gets train_recipe of its own size.  label is [b, N] int32 (ModelNet: the class repeated on every
    point); category [b] int32 is gathered from the pool on the same stream.  `recipe`: a mask for every cloud instead of the
    dataset's training recipe (0: no augmentation)."""

    def __init__(self, pool, batch_size, num_point, seed, dataset="shapenet", recipe=None, rank=0, world=1, stream=None, post=None):
        super().__init__(pool, batch_size, num_point, seed, rank, world, stream, post)
        self._recipe = (lambda b: train_recipe(b, dataset)) if recipe is None else (lambda b: check_recipe(int(recipe), b))
        self._recipe(self.batch_size)                       # (a bad dataset name or mask fails here, not in the first epoch)
        self._recipes = {}

    def _new_set(self, dev):
        import torch
        return (torch.empty((self.batch_size, self.num_point, 3), dtype=torch.float32, device=dev),
                torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev),
                torch.empty((self.batch_size,), dtype=torch.int32, device=dev))

    def _begin_epoch(self, plan):
        import torch
        for b in set(len(ids) for _step, ids in plan) - set(self._recipes):
            self._recipes[b] = torch.from_numpy(self._recipe(b)).to(self.pool.device)

    def _launch(self, step, ids_dev, out):
        import torch
        points, label, category = out
        assemble(self.pool.rows, self.pool.offsets, ids_dev, self.num_point, self.seed, step, self._recipes[len(category)],
                 out=(points, label))
        torch.index_select(self.pool.category_dev, 0, ids_dev, out=category)
