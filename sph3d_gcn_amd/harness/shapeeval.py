"""The ShapeNet part-segmentation evaluation with the votes kept on the device: the per-shape part IoU the paper reports
(shapenet_seg/evaluate_shapenet.py:228-301, evaluate_shapenet_onehot.py:247-334, post-merging/shapenet_mIoU.m / evaluateIoU.m),
on a pool of shapes (harness/objfeed.py:ShapePool).

THE LOOP, per batch of shapes in evalvote.batch_blocks order:
  1. draw num_point rows per shape with recipe 0 (objfeed.assemble, want_index);
  2. logits0 = model_fn(points, label, category);
  3. draw again with the same (seed, step) and objfeed.EVAL_AUGMENT: the sample is the same, the coordinates are augmented;
  4. logits1 = model_fn(...);
  5. add both to the drawn rows' sums, in that order;
  6. repeat until every row of every shape has been drawn more than 10 times (min_count = 11 draws).
The votes are csrc/vote.hip's, used directly: sph3d_vote_begin, then per draw p two sph3d_vote_accumulate with pass numbers 2p and
2p + 1 and min_votes = 2 * min_count.  That is arithmetically the reference: one fp32 add per logits tensor in order; numpy's
last-duplicate-wins rule for `sum[index] += logits` (evalvote.py: THE DUPLICATE RULE) — which also holds for its
`count[index] += 1`, one count per drawn row and draw; and `count > 10` <=> 2 * draws >= 22, where the device count — the logits
vectors a row received — is even after every draw and so reaches min_votes exactly at the end of draw min_count.  Every row of a
shape is an inner row (column 7 == 1), so the voter's "covered == inner_size" is the reference's "covered == size".  The pass
number is below 2^20, hence max_passes <= 2^19 draws.

Then sph3d_shape_iou (csrc/shapeeval.hip) takes the place of the voter's finalize: arg-max inside the shape's own part range and
the integer counts inter / pred_cnt / gt_cnt per part and correct per shape; the host forms
part_iou = 1.0 if union == 0 else inter / float(union), union = pred_cnt + gt_cnt - inter, and shape_iou = np.mean(part_ious) in
float64 from integers — the reference's figures bit for bit.

  * ``shape_vote_reference`` / ``evaluate_reference``: the SPECIFICATION in numpy, no GPU;
  * ``ShapeResult``: the figures, and ``merge`` of the ranks' shares;
  * ``evaluate``: the public call.

What differs from the reference, on purpose: the draws are this project's counter-based ones (step = (batch_index << 20) | draw),
so a batch's votes are a pure function of (seed, batch_index) on any number of ranks; the last, smaller batch runs at its own size;
`max_passes` ends a batch that does not get covered (`complete == False`); the per-shape text dumps and the "eval mean loss" line
are not reproduced.  The loop reads one word per draw from the device: a host synchronisation per draw.
"""
import collections

import numpy as np

from . import evalvote, feed, objfeed

MIN_COUNT = 11                       # `count > 10` of evaluate_shapenet.py:241
MAX_PASSES = 1 << 12                 # draws; at most 2^19 (two vote passes per draw, pass < 2^20)
MAX_CLASSES = evalvote.MAX_CLASSES


def _check_loop_args(num_point, num_cls, min_count, max_passes):
    if num_point <= 0 or not 0 < num_cls <= MAX_CLASSES:
        raise ValueError("num_point>0 and 0<num_cls<=%d required" % MAX_CLASSES)
    if min_count < 1:
        raise ValueError("min_count>=1 required")
    if not 0 < max_passes <= 1 << (evalvote.PASS_BITS - 1):
        raise ValueError("0<max_passes<=2^%d required" % (evalvote.PASS_BITS - 1))


# ---------------------------------------------------------------------------------------------------------------
# the statement (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def part_counts(votes, gt, part_lo, part_n):
    """one shape: votes [n, C] fp32 sums, gt [n] labels, its part range -> (pred [n] int32, inter, pred_cnt, gt_cnt [C] int32
    — zero outside the range —, correct)"""
    C = votes.shape[1]
    inter, pred_cnt, gt_cnt = (np.zeros((C,), dtype=np.int32) for _ in range(3))
    if part_n <= 0 or votes.shape[0] == 0:
        return np.zeros((votes.shape[0],), dtype=np.int32), inter, pred_cnt, gt_cnt, 0
    pred = (np.argmax(votes[:, part_lo:part_lo + part_n], axis=1) + part_lo).astype(np.int32)
    for l in range(part_lo, part_lo + part_n):
        inter[l] = np.sum((pred == l) & (gt == l))
        pred_cnt[l] = np.sum(pred == l)
        gt_cnt[l] = np.sum(gt == l)
    return pred, inter, pred_cnt, gt_cnt, int(np.sum(pred == gt))


def shape_iou(inter, pred_cnt, gt_cnt, part_lo, part_n):
    """the reference's figure of one shape from its integer counts (evaluate_shapenet.py:276-289): float64; nan without parts"""
    if part_n <= 0:
        return float("nan")
    part_ious = []
    for l in range(part_lo, part_lo + part_n):
        union = int(pred_cnt[l]) + int(gt_cnt[l]) - int(inter[l])
        part_ious.append(1.0 if union == 0 else int(inter[l]) / float(union))
    return float(np.mean(part_ious))


ShapeVotes = collections.namedtuple(
    "ShapeVotes", "votes count pred passes covered size inter pred_cnt gt_cnt correct shape_iou complete nonfinite_rows")


def shape_vote_reference(sizes, rows_label, shape_ids, part_lo, part_n, num_point, seed, batch_index, logits_of_pass, num_cls,
                         min_count=MIN_COUNT, max_passes=MAX_PASSES):
    """The loop of one batch.  sizes [P]: rows per shape of the pool; rows_label [T]: column 6 of the pool's rows; shape_ids [b]
    (distinct); part_lo, part_n [b]: the shapes' part ranges; logits_of_pass(q, index [b, N] int32) -> [b, N, C] float32, q = 2 p
    for the plain and 2 p + 1 for the augmented evaluation of draw p.
    -> ShapeVotes(votes: per shape [n, C] fp32 sums, added in order with fp32 adds; count: per shape [n] int32, the logits
                  vectors a row received (two per draw that took it); pred: per shape [n] int32; passes: draws; covered, size [b];
                  inter, pred_cnt, gt_cnt [b, C] int32; correct [b] int32; shape_iou [b] float64; complete; nonfinite_rows)
    A shape id outside the pool has no rows: empty arrays, zero counts."""
    _check_loop_args(num_point, num_cls, min_count, max_passes)
    sizes = np.asarray(sizes, dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(sizes)))
    shape_ids = np.asarray(shape_ids, dtype=np.int64).reshape(-1)
    b, C = shape_ids.shape[0], int(num_cls)
    part_lo, part_n = np.asarray(part_lo).reshape(-1), np.asarray(part_n).reshape(-1)
    valid = [i for i in shape_ids if 0 <= i < sizes.shape[0]]
    if len(set(valid)) != len(valid):
        raise ValueError("the shapes of a batch are distinct")
    gt = []
    for i in shape_ids:
        lo, hi = (int(offsets[i]), int(offsets[i + 1])) if 0 <= i < sizes.shape[0] else (0, 0)
        gt.append(np.asarray(rows_label[lo:hi]))
    for k in range(b):
        if gt[k].shape[0] and not (part_n[k] > 0 and part_lo[k] >= 0 and part_lo[k] + part_n[k] <= C):
            raise ValueError("shape %d: part range [%d, %d + %d) is not inside the %d outputs" % (k, part_lo[k], part_lo[k], part_n[k], C))
    votes = [np.zeros((g.shape[0], C), dtype=np.float32) for g in gt]
    count = [np.zeros((g.shape[0],), dtype=np.int32) for g in gt]
    size = np.array([g.shape[0] for g in gt], dtype=np.int32)
    covered = np.zeros((b,), dtype=np.int32)
    passes = 0
    while (covered < size).any() and passes < max_passes:
        index = evalvote.draw_index(sizes, shape_ids, num_point, seed, evalvote.pass_step(batch_index, passes))
        for a in range(2):
            logits = np.asarray(logits_of_pass(2 * passes + a, index), dtype=np.float32)
            if logits.shape != (b, num_point, C):
                raise ValueError("logits_of_pass: [b, N, C] expected, got %s" % (logits.shape,))
            for k in range(b):
                evalvote.vote_update(votes[k], count[k], index[k], logits[k])
        for k in range(b):
            covered[k] = np.sum(count[k] >= 2 * min_count)
        passes += 1
    pred, nonfinite = [], 0
    inter, pred_cnt, gt_cnt = (np.zeros((b, C), dtype=np.int32) for _ in range(3))
    correct, iou = np.zeros((b,), dtype=np.int32), np.full((b,), np.nan)
    for k in range(b):
        pr, inter[k], pred_cnt[k], gt_cnt[k], correct[k] = part_counts(votes[k], gt[k], int(part_lo[k]), int(part_n[k]))
        pred.append(pr)
        nonfinite += int((~np.isfinite(votes[k]).all(axis=1)).sum())
        if size[k]:
            iou[k] = shape_iou(inter[k], pred_cnt[k], gt_cnt[k], int(part_lo[k]), int(part_n[k]))
    return ShapeVotes(votes, count, pred, passes, covered, size, inter, pred_cnt, gt_cnt, correct, iou,
                      not (covered < size).any(), nonfinite)


# ---------------------------------------------------------------------------------------------------------------
# the result
# ---------------------------------------------------------------------------------------------------------------
class ShapeResult:
    """The figures of an evaluation, from integer counts, in float64 with the reference's formulas:
      shapes, category, shape_iou, correct, seen   per evaluated shape, in pool order (seen = its rows)
      category_miou [num_categories]   the mean shape_iou of each category (nan for a category without shapes)
      mean_category_miou               the mean of category_miou over the categories that occur (shapenet_mIoU.m "mean",
                                       evaluate_shapenet_onehot.py:326, where all of them do)
      instance_miou                    the mean of shape_iou ("total" / "all shapes")
      accuracy                         total_correct / float(total_seen)
      class_correct, class_seen [C]    int64 sums of inter and gt_cnt; class_acc = their quotient (nan for an absent part)
      batches, passes, covered, size   per evaluated batch; complete: every batch got covered within max_passes
      nonfinite_rows; votes: {batch number: ShapeVotes} with keep_votes, else None"""

    def __init__(self, shapes, category, shape_iou, correct, seen, class_correct, class_seen, batches, passes, covered, size,
                 nonfinite_rows, num_categories, votes=None):
        self.shapes = np.asarray(shapes, dtype=np.int64)
        self.category = np.asarray(category, dtype=np.int32)
        self.shape_iou = np.asarray(shape_iou, dtype=np.float64)
        self.correct, self.seen = np.asarray(correct, dtype=np.int64), np.asarray(seen, dtype=np.int64)
        self.class_correct, self.class_seen = np.asarray(class_correct, dtype=np.int64), np.asarray(class_seen, dtype=np.int64)
        self.batches, self.passes = list(batches), list(passes)
        self.covered, self.size = list(covered), list(size)
        self.nonfinite_rows, self.num_categories, self.votes = int(nonfinite_rows), int(num_categories), votes
        self.complete = all((np.asarray(c) >= np.asarray(s)).all() for c, s in zip(self.covered, self.size))
        self.category_miou = np.full((self.num_categories,), np.nan)
        for c in range(self.num_categories):
            mine = self.shape_iou[self.category == c]
            if mine.size:
                self.category_miou[c] = np.mean(mine)
        present = self.category_miou[~np.isnan(self.category_miou)]
        self.mean_category_miou = float(np.mean(present)) if present.size else float("nan")
        self.instance_miou = float(np.mean(self.shape_iou)) if self.shape_iou.size else float("nan")
        total_seen = int(self.seen.sum())
        self.accuracy = int(self.correct.sum()) / float(total_seen) if total_seen else float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            self.class_acc = self.class_correct / self.class_seen.astype(np.float64)

    @classmethod
    def from_batches(cls, mine, ids, cats, done, num_cls, num_categories, keep_votes):
        """mine: batch numbers; ids / cats: per batch the shape ids and categories; done: per batch ShapeVotes"""
        C = int(num_cls)
        cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt) for x in xs]) if xs else np.zeros((0,), dtype=dt)
        return cls(cat(ids, np.int64), cat(cats, np.int32), cat([d.shape_iou for d in done], np.float64),
                   cat([d.correct for d in done], np.int64), cat([d.size for d in done], np.int64),
                   sum((d.inter.astype(np.int64).sum(axis=0) for d in done), np.zeros((C,), np.int64)),
                   sum((d.gt_cnt.astype(np.int64).sum(axis=0) for d in done), np.zeros((C,), np.int64)),
                   mine, [d.passes for d in done], [d.covered for d in done], [d.size for d in done],
                   sum(d.nonfinite_rows for d in done), num_categories, dict(zip(mine, done)) if keep_votes else None)

    @classmethod
    def merge(cls, results):
        """the result of the ranks' shares together: equal to the world = 1 result"""
        results, order, votes = evalvote.merge_order(results)
        shapes = np.concatenate([res.shapes for res in results])
        if np.unique(shapes).shape[0] != shapes.shape[0]:
            raise ValueError("merge: a shape occurs in two results")
        by_shape = np.argsort(shapes, kind="stable")
        pick = lambda name: np.concatenate([getattr(res, name) for res in results])[by_shape]
        return cls(pick("shapes"), pick("category"), pick("shape_iou"), pick("correct"), pick("seen"),
                   sum(res.class_correct for res in results), sum(res.class_seen for res in results), order("batches"),
                   order("passes"), order("covered"), order("size"), sum(res.nonfinite_rows for res in results),
                   max(res.num_categories for res in results), votes)


def _table(category, part_lo, part_n, num_cls):
    """-> (part_lo, part_n per category or None, num_categories), checked"""
    category = np.asarray(category, dtype=np.int32).reshape(-1)
    if part_lo is None:
        return None, None, int(category.max()) + 1 if category.size else 0
    part_lo, part_n = np.asarray(part_lo, dtype=np.int32).reshape(-1), np.asarray(part_n, dtype=np.int32).reshape(-1)
    if part_lo.shape != part_n.shape or (part_lo < 0).any() or (part_n <= 0).any() or (part_lo + part_n > num_cls).any():
        raise ValueError("part table: 0 < part_n and 0 <= part_lo, part_lo + part_n <= num_cls required per category")
    if category.size and category.max() >= part_lo.shape[0]:
        raise ValueError("a shape's category is outside the part table")
    return part_lo, part_n, int(part_lo.shape[0])


def evaluate_reference(logits_fn, sizes, rows_label, category, batch_size, num_point, seed, num_cls, part_lo=None, part_n=None,
                       min_count=MIN_COUNT, max_passes=MAX_PASSES, rank=0, world=1, keep_votes=False):
    """`evaluate` stated in numpy: shape_vote_reference over the batches of rank `rank`; category [P]; part_lo / part_n: the
    one-hot model's table per category, None for a per-category model; logits_fn(batch_index, q, index [b, N]) -> [b, N, C]"""
    evalvote.check_share(batch_size, rank, world, "evaluate_reference")
    P, C = len(sizes), int(num_cls)
    category = np.asarray(category, dtype=np.int32).reshape(-1)
    tlo, tn, ncat = _table(category, part_lo, part_n, C)
    mine = list(range(rank, feed.batches_per_epoch(P, batch_size), world))
    ids = [evalvote.batch_blocks(P, batch_size, i) for i in mine]
    done = []
    for i, s in zip(mine, ids):
        lo = tlo[category[s]] if tlo is not None else np.zeros(s.shape, np.int32)
        n = tn[category[s]] if tn is not None else np.full(s.shape, C, np.int32)
        done.append(shape_vote_reference(sizes, rows_label, s, lo, n, num_point, seed, i,
                                         lambda q, index, _i=i: logits_fn(_i, q, index), C, min_count, max_passes))
    return ShapeResult.from_batches(mine, ids, [category[s] for s in ids], done, C, ncat, keep_votes)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
class ShapeVoter(evalvote.Voter):
    """evalvote.Voter's buffers and loop on an objfeed.ShapePool: a pass is one draw evaluated twice, on the plain and on the
    augmented coordinates, and a finished batch is closed by sph3d_shape_iou into `parts` instead of a confusion matrix.  A
    batch's shapes must lie inside `capacity_rows` consecutive rows of the pool."""
    what = "shapes"

    def __init__(self, pool, batch_size, num_point, num_cls, capacity_rows, min_count=MIN_COUNT):
        _check_loop_args(num_point, num_cls, min_count, 1)
        super().__init__(pool, batch_size, num_point, num_cls, capacity_rows, 2 * int(min_count))

    def _alloc(self, dev):
        import torch
        B, C = self.B, self.C
        self.parts = torch.zeros((3 * B * C + B,), dtype=torch.int32, device=dev)         # inter | pred_cnt | gt_cnt | correct
        self.out = (torch.empty((B, self.N, 3), dtype=torch.float32, device=dev), torch.empty((B, self.N), dtype=torch.int32, device=dev))
        self.recipes = (torch.zeros((B,), dtype=torch.int32, device=dev),
                        torch.full((B,), objfeed.EVAL_AUGMENT, dtype=torch.int32, device=dev))

    def _open(self, shape_ids):
        """the shapes' part ranges and categories, on the host and on the device; the two recipes cut to the batch"""
        import torch
        p, P = self.pool, len(self.pool)
        self._plo, self._pn = p.part_range(shape_ids, self.C)
        self._range_dev = torch.from_numpy(np.concatenate([self._plo, self._pn])).to(p.device)
        self._recipes = tuple(r[:len(shape_ids)] for r in self.recipes)
        self._category = torch.from_numpy(np.where((shape_ids >= 0) & (shape_ids < P), p.category[np.clip(shape_ids, 0, P - 1)], 0)
                                          .astype(np.int32)).to(p.device)

    def _pass(self, model_fn, ids_dev, out, seed, batch_index, p, vote):
        """draw p of a batch: the same sample plain, then with EVAL_AUGMENT, voted as passes 2 p and 2 p + 1"""
        step = evalvote.pass_step(batch_index, p)
        for a in range(2):
            points, label, index = objfeed.assemble(self.pool.rows, self.pool.offsets, ids_dev, self.N, seed, step,
                                                    self._recipes[a], out=out, want_index=True)
            vote(2 * p + a, index, lambda: model_fn(points, label, self._category))

    def run_batch(self, model_fn, shape_ids, seed, batch_index, max_passes=MAX_PASSES, keep_votes=False, on_pass=None):
        """all draws of one batch (at most max_passes of them), then its predictions and part counts -> ShapeVotes (votes /
        count / pred are per-shape host arrays with keep_votes, else None)"""
        _check_loop_args(self.N, self.C, 1, max_passes)
        return super().run_batch(model_fn, shape_ids, seed, batch_index, max_passes, keep_votes, on_pass)

    def _empty(self, b):
        zb, zc = np.zeros((b,), np.int32), np.zeros((b, self.C), np.int32)
        return ShapeVotes(None, None, None, 0, zb, zb.copy(), zc, zc.copy(), zc.copy(), zb.copy(), np.full((b,), np.nan), True, 0)

    def _close(self, shape_ids, common, passes, keep_votes):
        """the batch's predictions and part counts -> ShapeVotes"""
        from .. import _lib
        b, B, C, plo, pn = len(shape_ids), self.B, self.C, self._plo, self._pn
        before = int(self.nonfinite.item())
        inter, pred_cnt, gt_cnt = (self.parts[k * B * C:k * B * C + b * C] for k in range(3))
        correct = self.parts[3 * B * C:3 * B * C + b]
        _lib.check(_lib.lib().sph3d_shape_iou(b, C, *common, _lib.ptr(self.votes), _lib.ptr(self._range_dev),
                                              _lib.ptr(self._range_dev[b:]), _lib.ptr(self.pred), _lib.ptr(inter), _lib.ptr(pred_cnt),
                                              _lib.ptr(gt_cnt), _lib.ptr(correct), _lib.ptr(self.nonfinite), _lib.stream_ptr()))
        covered, size = self._coverage(b)
        parts = self.parts.cpu().numpy()
        nonfinite = int(self.nonfinite.item()) - before
        inter, pred_cnt, gt_cnt = (parts[k * B * C:k * B * C + b * C].reshape(b, C).copy() for k in range(3))
        correct = parts[3 * B * C:3 * B * C + b].copy()
        iou = np.array([shape_iou(inter[k], pred_cnt[k], gt_cnt[k], int(plo[k]), int(pn[k])) if size[k] else np.nan
                        for k in range(b)], dtype=np.float64)
        votes, count, pred = self._kept(shape_ids, common, keep_votes)
        return ShapeVotes(votes, count, pred, passes, covered, size, inter, pred_cnt, gt_cnt, correct, iou,
                          bool((covered >= size).all()), nonfinite)


def evaluate(model_fn, pool, batch_size, num_point, seed, num_cls, min_count=MIN_COUNT, max_passes=MAX_PASSES, rank=0, world=1,
             keep_votes=False, on_pass=None):
    """Evaluate a part-segmentation network on every shape of `pool` (objfeed.ShapePool) -> ShapeResult.

        pool = objfeed.ShapePool.from_arrays(xyz, part_label, category)
        res = evaluate(lambda p, l, c: model(p, is_training=False)[0], pool, 32, 2048, seed=0, num_cls=4)
        print(res.instance_miou, res.mean_category_miou, res.accuracy, res.complete)

    model_fn(points [b, N, 3] fp32, label [b, N] i32, category [b] i32) -> logits [b, N, num_cls] on the device; it is called
    twice per draw — on the plain and on the augmented coordinates of the same sample — under torch.no_grad() on the current
    stream, and the tensors it gets are overwritten by the next call.  With a part table in the pool (a one-hot model over all
    categories) a shape's prediction is taken among its category's parts only; without one among all num_cls outputs.
    Batch i is shapes [i * batch_size, (i + 1) * batch_size) of the pool; rank r of `world` takes batches r, r + world, ... and
    ShapeResult.merge of the ranks' results equals the world = 1 result.  min_count: the draws every row must have had (the
    reference's `count > 10`).  on_pass(batch_index, q, index, logits): a hook that sees the device tensors of evaluation
    q = 2 draw + (1 if augmented) before they are voted.  keep_votes: the sums, counts and predictions come to the host."""
    _check_loop_args(num_point, num_cls, min_count, max_passes)
    evalvote.check_share(batch_size, rank, world, "evaluate")
    C = int(num_cls)
    _lo, _n, ncat = _table(pool.category, pool.part_lo, pool.part_n, C)
    mine = list(range(rank, feed.batches_per_epoch(len(pool), batch_size), world))
    ids = [evalvote.batch_blocks(len(pool), batch_size, i) for i in mine]
    done = []
    if mine:
        cap = max(int(pool.host_offsets[s[-1] + 1] - pool.host_offsets[s[0]]) for s in ids)
        voter = ShapeVoter(pool, batch_size, num_point, C, cap, min_count)
        done = [voter.run_batch(model_fn, s, seed, i, max_passes, keep_votes, on_pass) for i, s in zip(mine, ids)]
    return ShapeResult.from_batches(mine, ids, [pool.category[s] for s in ids], done, C, ncat, keep_votes)
