"""The ScanNet line on the device: the training recipe of scannet_seg/train_scannet.py:112-127, the three-view overlap vote of
scannet_seg/evaluate_scannet_withoverlap.py:263-351 with its sub-20 figures, and the scene stage of post-merging/scannet_merge.m
on those votes (csrc/scanfeed.hip, include/sph3d.h: sph3d_blockfeed_assemble; the votes are csrc/vote.hip's, the scene stage
csrc/scene.hip's).

  * ``train_recipe`` / ``EVAL_VIEWS``: the reference's recipes as objfeed's per-cloud bit masks.  Training: the first B // 3
    clouds get turn, tilt, scale, shift and jitter, the next B // 3 tilt, scale, shift and jitter, the rest none.  Evaluation:
    every draw is evaluated three times — plain, then `augment_fn1` (tilt, scale, shift, jitter) applied to the plain view, then
    `augment_fn2` (all five) applied ON TOP of the augmented one: the script augments `batch_input` in place;
  * ``view_key`` / ``assemble_reference`` / ``apply_reference``: the SPECIFICATION of a batch of views in numpy, no GPU.  The
    sample draws are ``feed``'s, so index, label and inner do not depend on the recipes; view v takes its transform draws from
    ``view_key(ck, v)`` — view 0's key is the cloud's own, so one view draws what ``objfeed`` draws — and is computed from view
    v - 1.  The kernel's integer outputs equal the statement bit for bit; what it computes in fp32 is held to the project's
    1e-5 bound per view against the float64 transform of its OWN previous view (``apply_reference(base=...)``);
  * ``assemble``: the C entry;  ``ScanNetFeed``: one epoch of training batches under ``feed.TwoSetFeed``'s protocol, in
    ``feed.DeviceFeed``'s item format, so ``train.LINES["scannet"]`` and ``train.Trainer`` take it unchanged;
  * ``scan_vote_reference`` / ``evaluate_reference``: the three-view vote loop in numpy;  ``ScanNetVoter`` / ``evaluate``: the
    loop on the device;  ``scannet_metrics``: the script's figures over a subset of the classes;
  * ``SPH3DScanNet``: the model (models/SPH3D_scannet.py is the S3DIS model with 21 classes);
  * ``evaluate_scenes`` / ``write_predictions``: scannet_merge.m on the three-view votes, and its `dlmwrite`.

THE VOTE.  Per draw p the reference takes ONE sample, counts it once (`batch_sample_count[b][sample_index] += 1`) and adds the
three views' logits to the drawn rows' sums in view order; a row is covered when `count > 1`, that is after two draws.  On the
device the three views of draw p are voted as passes 3 p, 3 p + 1, 3 p + 2 of csrc/vote.hip (shapeeval.ShapeVoter does the same
with two): one fp32 add per logits tensor in order, numpy's last-duplicate-wins rule per view, and a device count — the logits
vectors a row received — that is a multiple of 3 after every draw, so min_votes = 6 is exactly `count > 1`.  The pass number is
below 2^20, hence 3 * max_passes < 2^20.

What differs from the reference, on purpose — as in feed.py and evalvote.py: the draws are this project's counter-based ones
(step = (batch_index << 20) | draw), not numpy's generator, so a batch's votes are a pure function of (seed, batch_index) on any
number of ranks; the two shuffles of the training loop are not separate steps; the last, smaller batch runs at its own size;
`max_passes` ends a batch that does not get covered (`complete == False`); the coordinates are fp32 throughout (the evaluation
script's `batch_input` is a float64 array filled with float32 rows); the .mat dumps and the "eval mean loss" line are not
reproduced.  ``scannet_metrics`` reports the real per-class accuracy where the script prints the IoU under that name (:343).
"""
import collections
import os

import numpy as np

from . import evalvote, feed, objfeed, s3dis_net, scenemerge
from .objfeed import ALL, JITTER, SCALE, SHIFT, TILT, TURN  # noqa: F401

CLASS_NAMES = ("other20", "wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture",
               "counter", "desk", "curtain", "refridgerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")
NUM_CLASSES = len(CLASS_NAMES)
SUB20 = tuple(range(1, 20))          # evaluate_scannet_withoverlap.py:52: np.arange(1, 20) — see scannet_metrics
BENCHMARK20 = tuple(range(1, 21))    # the 20 classes of the ScanNet benchmark
LABELID_SET = (40, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)      # scannet_merge.m:8, NYU-40 ids
TRAIN_FULL = ALL                                     # train_scannet.py:114-120
TRAIN_LIGHT = TILT | SCALE | SHIFT | JITTER          # train_scannet.py:122-127; augment_fn1 of the evaluation
EVAL_VIEWS = (0, TRAIN_LIGHT, ALL)                   # 'none', 'aug1', 'aug2' of evaluate_scannet_withoverlap.py:282-286
MAX_VIEWS = 4                                        # csrc/scanfeed.hip: kScanMaxViews
MIN_DRAWS = 2                                        # `count > 1` of evaluate_scannet_withoverlap.py:280
MAX_PASSES = evalvote.MAX_PASSES                     # draws


# ---------------------------------------------------------------------------------------------------------------
# the recipes
# ---------------------------------------------------------------------------------------------------------------
def train_recipe(B):
    """-> recipe [B] int32 of a training batch (train_scannet.py:112-127, augSize = np.int32(1 / 3.0 * bsize)): the first B // 3
    clouds TRAIN_FULL, the next B // 3 TRAIN_LIGHT, the rest 0"""
    B = int(B)
    if B <= 0:
        raise ValueError("train_recipe: B>0 required")
    r = np.zeros((B,), dtype=np.int32)
    third = B // 3
    r[:third] = TRAIN_FULL
    r[third:2 * third] = TRAIN_LIGHT
    return r


def check_recipes(recipes, B):
    """-> recipes as int32 [V, B], 1 <= V <= MAX_VIEWS, from [V, B] masks or [B] masks (one view); masks outside [0, 31] are
    refused.  (One mask per view for all clouds, as EVAL_VIEWS: eval_recipes.)"""
    r = np.asarray(recipes)
    if r.ndim == 1:
        r = r.reshape(1, -1)
    if r.ndim != 2 or r.shape[1] != B or not 1 <= r.shape[0] <= MAX_VIEWS or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("recipes: integer masks [views, B] with 1 <= views <= %d expected" % MAX_VIEWS)
    if r.min() < 0 or r.max() > ALL:
        raise ValueError("recipes: masks are in [0, %d]" % ALL)
    return np.ascontiguousarray(r, dtype=np.int32)


def eval_recipes(views, B):
    """one mask per view for all B clouds -> int32 [V, B]"""
    v = np.asarray(views)
    if v.ndim != 1 or not 1 <= v.shape[0] <= MAX_VIEWS:
        raise ValueError("views: 1..%d masks expected" % MAX_VIEWS)
    return check_recipes(np.repeat(v.reshape(-1, 1), int(B), axis=1), int(B))


# ---------------------------------------------------------------------------------------------------------------
# the statement of a batch of views (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def view_key(ck, v):
    """the key view v of the cloud with key ck takes its transform draws from (csrc/feed_draws.hpp: feed_view_key): ck itself for
    v = 0, one more splitmix round over (ck, v) for v >= 1"""
    v = int(v)
    if v < 0:
        raise ValueError("view_key: v>=0 required")
    if v == 0:
        return np.uint64(ck)
    with np.errstate(over="ignore"):
        return feed._mix(np.uint64(ck) + np.uint64(v) + feed._GOLD)


ScanReference = collections.namedtuple("ScanReference", "index recipes views")


def assemble_reference(sizes, block_ids, num_point, seed, step, recipes):
    """The draws of one batch of views.  sizes: rows per block of the pool; block_ids [B]; recipes [V, B] (check_recipes).
    -> ScanReference(index [B, N] int32 — feed.assemble_reference's, whatever the recipes; recipes [V, B] int32;
                     views: per view an objfeed.Reference (index, recipe [B], theta, tilt, scale, shift, noise) whose draws
                     come from view_key(cloud key, v))
    A pure function of its arguments."""
    block_ids = np.asarray(block_ids, dtype=np.int64).reshape(-1)
    B, N = block_ids.shape[0], int(num_point)
    index = feed.assemble_reference(sizes, block_ids, N, seed, step, False).index
    recipes = check_recipes(recipes, B)
    views = []
    for v in range(recipes.shape[0]):
        theta, tilts = np.zeros((B,)), np.zeros((B, 3))
        scale, shift, noise = np.ones((B,)), np.zeros((B, 3)), np.zeros((B, N, 3))
        for b in range(B):
            vk, m = view_key(feed.cloud_key(seed, step, b), v), int(recipes[v, b])
            if m & TURN:
                theta[b] = objfeed.turn_angle(vk)
            if m & TILT:
                tilts[b] = objfeed.tilt_angles(vk)
            if m & SCALE:
                scale[b] = objfeed.scale_factor(vk)
            if m & SHIFT:
                shift[b] = objfeed.shift_vector(vk)
            if m & JITTER:
                noise[b] = objfeed.jitter_noise(vk, N)
        views.append(objfeed.Reference(index, recipes[v], theta, tilts, scale, shift, noise))
    return ScanReference(index, recipes, views)


def apply_reference(blocks, block_ids, ref, base=None):
    """the views `ref` describes, from host blocks [n, 8]: -> points [V, B, N, 6] float64, label, inner [B, N] int32.
    View v's xyz is objfeed.transform of view v - 1 (view -1: the pool rows), in float64 all the way.  With `base` — an array
    [V, B, N, >= 3], the kernel's own points — view v >= 1 is computed from base[v - 1] instead, so that every view can be held
    against one fp32 transform of the kernel's previous view; view 0 is computed from the pool rows either way."""
    B, N = ref.index.shape
    V = len(ref.views)
    points = np.zeros((V, B, N, 6), dtype=np.float64)
    label = np.zeros((B, N), dtype=np.int32)
    inner = np.zeros((B, N), dtype=np.int32)
    if base is not None:
        base = np.asarray(base)
        if base.ndim != 4 or base.shape[:3] != (V, B, N) or base.shape[3] < 3:
            raise ValueError("apply_reference: base [V, B, N, >= 3] expected")
    for b in range(B):
        rows = np.asarray(blocks[int(block_ids[b])])[ref.index[b]]
        xyz = rows[:, 0:3].astype(np.float64)
        for v, r in enumerate(ref.views):
            if base is not None and v > 0:
                xyz = base[v - 1, b, :, 0:3].astype(np.float64)
            xyz = objfeed.transform(xyz, int(r.recipe[b]), r.theta[b], r.tilt[b], r.scale[b], r.shift[b], r.noise[b])
            points[v, b, :, 0:3], points[v, b, :, 3:6] = xyz, rows[:, 3:6]
        label[b], inner[b] = rows[:, 6].astype(np.int32), rows[:, 7].astype(np.int32)
    return points, label, inner


# ---------------------------------------------------------------------------------------------------------------
# the device side of the feed
# ---------------------------------------------------------------------------------------------------------------
def assemble(rows, offsets, block_ids, num_point, seed, step, recipes, out=None, want_index=False):
    """sph3d_blockfeed_assemble on torch's current stream.  rows [T, 8] fp32, offsets [P+1] int64, block_ids [B] int32, all on
    the device.  recipes: a host array (check_recipes: [V, B] or [B]; checked here, then uploaded), or a
    contiguous int32 device tensor [V, B] or [B] that check_recipes has seen before its upload.  A 1-D recipe [B] means one view.
    out: (points [V, B, N, 6] fp32 — [B, N, 6] for a 1-D recipe —, label [B, N] i32, inner [B, N] i32) to write into, else new
    tensors.  -> points, label, inner (and index [B, N] i32 with want_index)"""
    import torch
    from .. import _lib
    _lib.require_device(rows, offsets, block_ids)
    B, N, dev = int(block_ids.shape[0]), int(num_point), rows.device
    if torch.is_tensor(recipes):
        _lib.require_device(recipes)
        if recipes.dtype != torch.int32 or not recipes.is_contiguous() or recipes.dim() not in (1, 2) or recipes.shape[-1] != B \
                or not 1 <= (recipes.shape[0] if recipes.dim() == 2 else 1) <= MAX_VIEWS:
            raise ValueError("assemble: a device recipe is a contiguous int32 [views, B] or [B], views <= %d" % MAX_VIEWS)
        one = recipes.dim() == 1
    else:
        one = np.ndim(recipes) == 1
        recipes = torch.from_numpy(check_recipes(recipes, B)).to(dev)
    V = 1 if one else int(recipes.shape[0])
    shape = (B, N, 6) if one else (V, B, N, 6)
    if out is None:
        out = (torch.empty(shape, dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
               torch.empty((B, N), dtype=torch.int32, device=dev))
    points, label, inner = out
    if tuple(points.shape) != shape or not points.is_contiguous():
        raise ValueError("assemble: points of shape %s expected" % (shape,))
    # (the checks of the pool's tensors, the ids and the outputs: view 0 stands for the whole points tensor)
    B, N, _out, index = feed.assemble_args(_lib, rows, offsets, block_ids, "block_ids", N, (points if one else points[0], label, inner),
                                           feed._FEED_OUT, want_index)
    _lib.check(_lib.lib().sph3d_blockfeed_assemble(B, N, int(offsets.shape[0]) - 1, int(rows.shape[0]), _lib.ptr(rows),
                                                   _lib.ptr(offsets), _lib.ptr(block_ids), seed & 0xffffffffffffffff,
                                                   step & 0xffffffffffffffff, V, _lib.ptr(recipes), _lib.ptr(points),
                                                   _lib.ptr(label), _lib.ptr(inner), _lib.ptr(index), _lib.stream_ptr()))
    return (points, label, inner, index) if want_index else (points, label, inner)


class ScanNetFeed(feed.TwoSetFeed):
    """One epoch of ScanNet training batches per iteration, assembled on the device under train_recipe (feed.TwoSetFeed states
    the protocol and who owns an item's tensors).  An item is feed.DeviceFeed's: (points [b, N, 6], label, inner, ready).

        feed = ScanNetFeed(pool, 16, 8192, seed=1)
        trainer = train.Trainer(model, model.loss, ..., 21, line=train.LINES["scannet"], prime=..., seed=1)
        trainer.train_one_epoch(feed)

    The last, smaller batch gets train_recipe of its own size.  augment=False: every mask is 0."""

    def __init__(self, pool, batch_size, num_point, seed, augment=True, rank=0, world=1, stream=None, post=None):
        self.augment = bool(augment)
        self._recipes = {}
        super().__init__(pool, batch_size, num_point, seed, rank, world, stream, post)

    def recipe(self, b):
        return train_recipe(b) if self.augment else np.zeros((int(b),), dtype=np.int32)

    def _new_set(self, dev):
        import torch
        return (torch.empty((self.batch_size, self.num_point, 6), dtype=torch.float32, device=dev),
                torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev),
                torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev))

    def _begin_epoch(self, plan):
        import torch
        for b in set(len(ids) for _step, ids in plan) - set(self._recipes):
            self._recipes[b] = torch.from_numpy(self.recipe(b)).to(self.pool.device)

    def _launch(self, step, ids_dev, out):
        assemble(self.pool.rows, self.pool.offsets, ids_dev, self.num_point, self.seed, step, self._recipes[int(ids_dev.shape[0])],
                 out=out)


# ---------------------------------------------------------------------------------------------------------------
# the vote loop (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def _check_loop_args(num_point, num_cls, views, min_draws, max_passes):
    if not 1 <= int(views) <= MAX_VIEWS:
        raise ValueError("1<=views<=%d required" % MAX_VIEWS)
    if min_draws < 1:
        raise ValueError("min_draws>=1 required")
    evalvote._check_loop_args(num_point, num_cls, int(views) * int(min_draws), 1)
    if not 0 < max_passes or not int(views) * int(max_passes) < (1 << evalvote.PASS_BITS):
        raise ValueError("0<max_passes and views*max_passes<2^%d required" % evalvote.PASS_BITS)


def scan_vote_reference(sizes, rows_label, rows_inner, block_ids, num_point, seed, batch_index, logits_of_pass, num_cls=NUM_CLASSES,
                        views=len(EVAL_VIEWS), min_draws=MIN_DRAWS, max_passes=MAX_PASSES):
    """The loop of one batch.  sizes [P]: rows per block of the pool; rows_label, rows_inner [T]: columns 6 and 7 of the pool's
    rows; block_ids [b] (distinct); logits_of_pass(q, index [b, N] int32) -> [b, N, C] float32, q = views * p + v for view v of
    draw p; views: how many views a draw has.  Per draw: one sample at pass_step(batch_index, p), then one evalvote.vote_update
    per view, in view order.  Coverage: count >= views * min_draws over the inner rows.
    -> evalvote.BatchVotes (count: the logits vectors a row received, `views` per draw that took it; passes: draws)"""
    V = int(views)
    _check_loop_args(num_point, num_cls, V, min_draws, max_passes)
    sizes = np.asarray(sizes, dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(sizes)))
    block_ids = np.asarray(block_ids, dtype=np.int64).reshape(-1)
    b, C = block_ids.shape[0], int(num_cls)
    valid = [i for i in block_ids if 0 <= i < sizes.shape[0]]
    if len(set(valid)) != len(valid):
        raise ValueError("the blocks of a batch are distinct")
    label, inner = [], []
    for i in block_ids:
        lo, hi = (int(offsets[i]), int(offsets[i + 1])) if 0 <= i < sizes.shape[0] else (0, 0)
        label.append(np.asarray(rows_label[lo:hi]))
        inner.append(np.asarray(rows_inner[lo:hi]) == 1)
    votes = [np.zeros((l.shape[0], C), dtype=np.float32) for l in label]
    count = [np.zeros((l.shape[0],), dtype=np.int32) for l in label]
    inner_size = np.array([m.sum() for m in inner], dtype=np.int32)
    covered = np.zeros((b,), dtype=np.int32)
    passes = 0
    while (covered < inner_size).any() and passes < max_passes:
        index = evalvote.draw_index(sizes, block_ids, num_point, seed, evalvote.pass_step(batch_index, passes))
        for v in range(V):
            logits = np.asarray(logits_of_pass(V * passes + v, index), dtype=np.float32)
            if logits.shape != (b, num_point, C):
                raise ValueError("logits_of_pass: [b, N, C] expected, got %s" % (logits.shape,))
            for k in range(b):
                evalvote.vote_update(votes[k], count[k], index[k], logits[k])
        for k in range(b):
            covered[k] = np.sum(count[k][inner[k]] >= V * min_draws)
        passes += 1
    confusion = np.zeros((C, C), dtype=np.int64)
    pred, nonfinite = [], 0
    for k in range(b):
        pr = np.argmax(votes[k], axis=1).astype(np.int32) if votes[k].shape[0] else np.zeros((0,), dtype=np.int32)
        pred.append(pr)
        nonfinite += int((~np.isfinite(votes[k]).all(axis=1)).sum())
        use = inner[k] & (label[k] >= 0) & (label[k] < C)
        np.add.at(confusion, (label[k][use].astype(np.int64), pr[use].astype(np.int64)), 1)
    return evalvote.BatchVotes(votes, count, pred, passes, covered, inner_size, confusion, not (covered < inner_size).any(), nonfinite)


def evaluate_reference(logits_fn, sizes, rows_label, rows_inner, batch_size, num_point, seed, num_cls=NUM_CLASSES,
                       views=len(EVAL_VIEWS), min_draws=MIN_DRAWS, max_passes=MAX_PASSES, rank=0, world=1, keep_votes=False):
    """`evaluate` stated in numpy: scan_vote_reference over the batches of rank `rank`;
    logits_fn(batch_index, q, index [b, N]) -> [b, N, C] float32, q = views * draw + view"""
    evalvote.check_share(batch_size, rank, world, "evaluate_reference")
    P, C = len(sizes), int(num_cls)
    mine = list(range(rank, feed.batches_per_epoch(P, batch_size), world))
    done = [scan_vote_reference(sizes, rows_label, rows_inner, evalvote.batch_blocks(P, batch_size, i), num_point, seed, i,
                                lambda q, index, _i=i: logits_fn(_i, q, index), C, views, min_draws, max_passes) for i in mine]
    return evalvote.EvalResult(sum((d.confusion for d in done), np.zeros((C, C), np.int64)), mine, [d.passes for d in done],
                               [d.covered for d in done], [d.inner_size for d in done], sum(d.nonfinite_rows for d in done),
                               dict(zip(mine, done)) if keep_votes else None)


# ---------------------------------------------------------------------------------------------------------------
# the vote loop on the device
# ---------------------------------------------------------------------------------------------------------------
class ScanNetVoter(evalvote.Voter):
    """evalvote.Voter's buffers and loop with a pass that is ONE draw evaluated in all views: one sph3d_blockfeed_assemble, then
    model_fn and a vote per view, voted as passes V p + v with min_votes = V * min_draws (see THE VOTE above).  `views`: one mask
    per view, applied to every cloud."""

    def __init__(self, pool, batch_size, num_point, num_cls, capacity_rows, views=EVAL_VIEWS, min_draws=MIN_DRAWS):
        self.views = tuple(int(m) for m in views)
        self.V = len(self.views)
        _check_loop_args(num_point, num_cls, self.V, min_draws, 1)
        eval_recipes(self.views, 1)                                      # (a mask outside [0, 31] fails here)
        super().__init__(pool, batch_size, num_point, num_cls, capacity_rows, self.V * int(min_draws))

    def _alloc(self, dev):
        import torch
        self.confusion = torch.zeros((self.C * self.C,), dtype=torch.int64, device=dev)
        # points: the loop cuts every output to the batch's b leading rows; [B, V * N * 6] cut to b rows is the contiguous
        # storage of a [V, b, N, 6] tensor, which is how _pass looks at it
        self.out = (torch.empty((self.B, self.V * self.N * 6), dtype=torch.float32, device=dev),
                    torch.empty((self.B, self.N), dtype=torch.int32, device=dev),
                    torch.empty((self.B, self.N), dtype=torch.int32, device=dev))
        self.recipes = {}

    def _open(self, block_ids):
        import torch
        b = len(block_ids)
        if b not in self.recipes:
            self.recipes[b] = torch.from_numpy(eval_recipes(self.views, b)).to(self.pool.device)
        self._recipes = self.recipes[b]

    def _pass(self, model_fn, ids_dev, out, seed, batch_index, p, vote):
        """draw p of a batch: one sample in all views, voted as passes V p .. V p + V - 1"""
        b = int(ids_dev.shape[0])
        points = out[0].view(self.V, b, self.N, 6)
        points, label, inner, index = assemble(self.pool.rows, self.pool.offsets, ids_dev, self.N, seed,
                                               evalvote.pass_step(batch_index, p), self._recipes, out=(points, out[1], out[2]),
                                               want_index=True)
        for v in range(self.V):
            vote(self.V * p + v, index, lambda _v=v: model_fn(points[_v], label, inner))

    def run_batch(self, model_fn, block_ids, seed, batch_index, max_passes=MAX_PASSES, keep_votes=False, on_pass=None):
        """all draws of one batch (at most max_passes of them) -> evalvote.BatchVotes; passes counts draws"""
        _check_loop_args(self.N, self.C, self.V, 1, max_passes)
        return super().run_batch(model_fn, block_ids, seed, batch_index, max_passes, keep_votes, on_pass)


def evaluate(model_fn, pool, batch_size, num_point, seed, num_cls=NUM_CLASSES, views=EVAL_VIEWS, min_draws=MIN_DRAWS,
             max_passes=MAX_PASSES, rank=0, world=1, keep_votes=False, on_pass=None):
    """Evaluate a network on every block of `pool` (feed.BlockPool) the ScanNet way -> evalvote.EvalResult.

        pool = feed.BlockPool.from_records(val_paths)
        res = scannet.evaluate(lambda p, l, i: model(p, is_training=False)[0], pool, 16, 8192, seed=0)
        m = scannet.scannet_metrics(res.confusion)
        print(m.miou, m.overall_acc, m.mean_class_acc, res.complete)

    model_fn(points [b, N, 6] fp32, label [b, N] i32, inner [b, N] i32) -> logits [b, N, num_cls] on the device; it is called
    once per view of every draw — plain, augment_fn1, augment_fn2 on top of it — under torch.no_grad() on the current stream;
    the tensors it gets are overwritten by the next draw.  Batches, ranks, `merge`, keep_votes: as evalvote.evaluate.
    min_draws: the draws every inner row must have had (the reference's `count > 1`).  on_pass(batch_index, q, index, logits):
    a hook that sees the device tensors of evaluation q = len(views) * draw + view before they are voted.  The result's own
    miou / overall_acc are evalvote.metrics over all num_cls classes; the script's figures are scannet_metrics(res.confusion)."""
    V = len(tuple(views))
    _check_loop_args(num_point, num_cls, V, min_draws, max_passes)
    evalvote.check_share(batch_size, rank, world, "evaluate")
    mine = list(range(rank, feed.batches_per_epoch(len(pool), batch_size), world))
    C = int(num_cls)
    if not mine:
        return evalvote.EvalResult(np.zeros((C, C), np.int64), [], [], [], [], 0, {} if keep_votes else None)
    spans = [evalvote.batch_blocks(len(pool), batch_size, i) for i in mine]
    cap = max(int(pool.host_offsets[ids[-1] + 1] - pool.host_offsets[ids[0]]) for ids in spans)
    voter = ScanNetVoter(pool, batch_size, num_point, C, cap, views, min_draws)
    done = [voter.run_batch(model_fn, ids, seed, i, max_passes, keep_votes, on_pass) for i, ids in zip(mine, spans)]
    confusion, nonfinite = voter.totals()
    return evalvote.EvalResult(confusion, mine, [d.passes for d in done], [d.covered for d in done], [d.inner_size for d in done],
                               nonfinite, dict(zip(mine, done)) if keep_votes else None)


# ---------------------------------------------------------------------------------------------------------------
# the figures
# ---------------------------------------------------------------------------------------------------------------
ScanMetrics = collections.namedtuple("ScanMetrics", "overall_acc class_acc class_iou miou mean_class_acc classes")


def scannet_metrics(confusion, classes=SUB20):
    """confusion [C, C] (label, prediction) over ALL classes -> ScanMetrics, in float64:
      class_acc, class_iou [C]   evalvote.metrics' formulas and eps on the full matrix (evaluate_scannet_withoverlap.py:331-334):
                                 a prediction of class 0 ("other20") for a wall point is in the wall's union, and a point
                                 labelled 0 that is predicted as wall is in it too
      miou, mean_class_acc       their means over `classes`
      overall_acc                sum of the diagonal over `classes` / sum of the points LABELLED with one of `classes`
                                 (:336-339, :346); nan without such a point
    classes=SUB20 is the script's set: `sub20_classids = np.arange(1, 20)` leaves out class 0 AND class 20 ("otherfurniture"),
    which the benchmark does count: classes=BENCHMARK20 gives the 20-class figures.  (The script's means divide by 20 all the
    same, because its dictionaries hold 'otherfurniture' at 0.0: its printed means are 19 / 20 of the ones given here.)  The
    script prints the IoU under the name of class accuracy (:343, `sub20_class_acc[cat] = class_iou[cat]`); mean_class_acc here
    is the real accuracy."""
    m = evalvote.metrics(confusion)
    cm = np.asarray(confusion, dtype=np.float64)
    cls = np.asarray(classes, dtype=np.int64).reshape(-1)
    if cls.size == 0 or cls.min() < 0 or cls.max() >= cm.shape[0] or np.unique(cls).shape[0] != cls.shape[0]:
        raise ValueError("scannet_metrics: distinct classes inside the matrix expected")
    seen = cm.sum(axis=1)[cls].sum()
    overall = float(np.diag(cm)[cls].sum() / seen) if seen > 0 else float("nan")
    return ScanMetrics(overall, m.class_acc, m.class_iou, float(m.class_iou[cls].mean()), float(m.class_acc[cls].mean()),
                       tuple(int(c) for c in cls))


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
class SPH3DScanNet(s3dis_net.SPH3DS3DIS):
    """models/SPH3D_scannet.py differs from models/SPH3D_s3dis.py in nothing but the class count: s3dis_net.SPH3DS3DIS on
    s3dis_net.scannet_config(num_input) (scannet_seg/scannet_config.py: 8192 points, 21 classes).  config: another plan with
    21 classes instead (a reduced one for tests)."""

    def __init__(self, num_input=8192, config=None, device=None, seed=7):
        config = config if config is not None else s3dis_net.scannet_config(num_input)
        if config.num_cls != NUM_CLASSES:
            raise ValueError("SPH3DScanNet: a plan with %d classes expected" % NUM_CLASSES)
        super().__init__(config, device=device, seed=seed)


# ---------------------------------------------------------------------------------------------------------------
# the scene stage (post-merging/scannet_merge.m)
# ---------------------------------------------------------------------------------------------------------------
def evaluate_scenes_reference(logits_fn, sizes, rows_label, rows_inner, index, scene_of_block, scenes, batch_size, num_point, seed,
                              num_cls=NUM_CLASSES, views=len(EVAL_VIEWS), min_draws=MIN_DRAWS, max_passes=MAX_PASSES, rank=0,
                              world=1, label_map=LABELID_SET, keep_pred=False):
    """`evaluate_scenes` stated in numpy: scenemerge.evaluate_scenes_reference fed with scan_vote_reference's three-view votes"""
    V = int(views)
    _check_loop_args(num_point, num_cls, V, min_draws, max_passes)

    def vote_fn(sizes, rows_label, rows_inner, ids, num_point, seed, i, fn, C, _min_votes, max_passes):
        return scan_vote_reference(sizes, rows_label, rows_inner, ids, num_point, seed, i, fn, C, V, min_draws, max_passes)
    return scenemerge.evaluate_scenes_reference(logits_fn, sizes, rows_label, rows_inner, index, scene_of_block, scenes, batch_size,
                                                num_point, seed, num_cls, V * int(min_draws), max_passes, rank, world, label_map,
                                                keep_pred, vote_fn=vote_fn)


def evaluate_scenes(model_fn, pool, scenes, batch_size, num_point, seed, num_cls=NUM_CLASSES, views=EVAL_VIEWS, min_draws=MIN_DRAWS,
                    max_passes=MAX_PASSES, rank=0, world=1, label_map=LABELID_SET, keep_pred=False, on_pass=None):
    """scenemerge.evaluate_scenes on the three-view votes -> scenemerge.SceneResult: every batch of a scene's blocks runs
    ScanNetVoter.run_batch, and the scene's `pred_full` goes through label_map (scannet_merge.m:8,55: the NYU-40 ids).

        pool = feed.BlockPool.from_records(scene_files, with_index=True)         # one record file per scene
        res = scannet.evaluate_scenes(lambda p, l, i: model(p, is_training=False)[0], pool, scenes, 16, 8192, seed=0, keep_pred=True)
        scannet.write_predictions("test_pred", scene_names, res)"""
    views = tuple(views)
    _check_loop_args(num_point, num_cls, len(views), min_draws, max_passes)
    return scenemerge.evaluate_scenes(
        model_fn, pool, scenes, batch_size, num_point, seed, num_cls, len(views) * int(min_draws), max_passes, rank, world, label_map,
        keep_pred, on_pass,
        voter_factory=lambda p, B, N, C, cap, _min_votes: ScanNetVoter(p, B, N, C, cap, views, min_draws))


def prediction_path(directory, name):
    return os.path.join(directory, "%s.txt" % name)


def write_predictions(directory, names, result):
    """the `dlmwrite` of scannet_merge.m:64: one file <name>.txt per evaluated scene with a full cloud, one id per line — the
    scene's pred_full (NYU-40 ids under label_map=LABELID_SET; -1 for a point without a prediction).  names: the names of ALL
    scenes, indexed by scene number; result: a SceneResult of keep_pred=True.  -> the paths written"""
    if result.pred is None:
        raise ValueError("write_predictions: a result of evaluate_scenes(..., keep_pred=True) expected")
    os.makedirs(directory, exist_ok=True)
    paths = []
    for s in result.scenes:
        pf = result.pred[s]["pred_full"]
        if pf is None:
            continue
        path = prediction_path(directory, names[s])
        with open(path, "w") as f:
            f.write("".join("%d\n" % v for v in np.asarray(pf).reshape(-1)))
        paths.append(path)
    return paths


def read_predictions(path):
    """-> int32 [F]: a file write_predictions wrote"""
    with open(path) as f:
        return np.array([int(line) for line in f if line.strip()], dtype=np.int32)
