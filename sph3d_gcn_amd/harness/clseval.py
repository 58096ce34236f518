"""The ModelNet40 classification evaluation with the votes kept on the device: the figures modelnet40_cls/evaluate_modelnet.py:
149-223 prints — instance accuracy, mean class accuracy, the per-class table, the `pred_votes` array — on a pool of shapes
(harness/objfeed.py:ShapePool; csrc/clseval.hip, include/sph3d.h: sph3d_clsfeed_assemble, sph3d_cls_vote_accumulate / _finalize).

THE LOOP, per batch of shapes in evalvote.batch_blocks order (evaluate_modelnet.py:168-207):
  1. every shape of the batch whole, in stored order (order = 1), its axes swapped from x-z-y to x-y-z if the records are the
     reference's (swap_yz; `batch_xyz[:, :, [0, 2, 1]]`, :173);
  2. vote 0 on the plain coordinates, votes >= 1 on EVAL_AUGMENT = turn, tilt, scale, shift (augment_fn, :71-78,181-184), each
     with its own draw step evalvote.pass_step(batch_index, vote);
  3. the [b, C] fp32 logits of every vote added to a FLOAT64 sum — `np.zeros((BATCH_SIZE, NUM_CLASSES))` is float64 (:180,196),
     so a sum of fp32 logits in fp32 is not the reference's —, one add per vote, in vote order;
  4. the first maximum of the sums is the shape's class; seen / correct in total and per class (:198-207).
The vote count is fixed, so nothing waits for the device: ClassVoter.run_batch issues `assemble -> model_fn -> accumulate` per vote
and one finalize without a device-to-host read, and ClassVoter.result reads the counters once, after the last batch.

  * ``assemble_reference`` / ``vote_reference`` / ``evaluate_reference``: the SPECIFICATION in numpy, no GPU.  The kernels equal
    it bit for bit wherever the values are integers, copies or ordered float64 adds; what the feed computes in fp32 is held to
    the project's 1e-5 bound against the float64 evaluation (tests/test_gpu_clseval.py);
  * ``ClsResult``: the figures, and ``merge`` of the ranks' shares;
  * ``assemble``: the C entry of the batch;  ``ClassVoter``: the device buffers and the loop;  ``evaluate``: the public call.

What differs from the reference, on purpose: the random numbers of the augmented votes are this project's counter-based ones
(harness/feed.py), not numpy's; the last, smaller batch is evaluated at its own size (the reference keeps a fixed placeholder
and feeds the short batch as it is, which its graph would not accept — there is no padding to restate); a label outside [0, C)
is counted in `bad_label` where the reference would raise; the "eval mean loss" line — the LAST vote's loss of each batch,
regulariser included (:191,202,211) — is not reproduced.
"""
import collections

import numpy as np

from . import evalvote, feed, objfeed
from .objfeed import SCALE, SHIFT, TILT, TURN

EVAL_AUGMENT = TURN | TILT | SCALE | SHIFT            # evaluate_modelnet.py:71-78
MASKS = TURN | TILT | SCALE | SHIFT                   # what a recipe of this feed may ask for: no jitter
MAX_CLASSES = evalvote.MAX_CLASSES
SEEN, CORRECT, NONFINITE, BAD_LABEL = 0, 1, 2, 3      # the finalize kernel's counters


def vote_recipe(vote):
    """the mask of vote `vote`: the first is plain (evaluate_modelnet.py:183)"""
    return 0 if vote == 0 else EVAL_AUGMENT


def check_recipe(recipe, B):
    """objfeed.check_recipe with this feed's range -> int32 [B]; a mask outside [0, 15] raises ValueError"""
    r = objfeed.check_recipe(recipe, B)
    if r.max() > MASKS:
        raise ValueError("recipe: masks are in [0, %d] (turn, tilt, scale, shift; this feed has no jitter)" % MASKS)
    return r


def _check_loop_args(num_point, num_cls, num_votes):
    if num_point <= 0 or not 0 < num_cls <= MAX_CLASSES:
        raise ValueError("num_point>0 and 0<num_cls<=%d required" % MAX_CLASSES)
    if not 0 < num_votes < (1 << evalvote.PASS_BITS):
        raise ValueError("0<num_votes<2^%d required" % evalvote.PASS_BITS)


# ---------------------------------------------------------------------------------------------------------------
# the statement (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
ClsBatch = collections.namedtuple("ClsBatch", "points index source recipe")


def assemble_reference(sizes, rows_xyz, shape_ids, num_point, seed, step, recipe, order, swap_yz):
    """One batch.  sizes [P]: rows per shape of the pool; rows_xyz [T, 3]: columns 0:3 of the pool's rows; shape_ids [B];
    recipe: [B] masks in [0, 15], or one for all; order 1: slot i takes row i (index -1 and zeros past the shape's last row),
    order 0: objfeed.assemble_reference's sample; swap_yz: columns 1 and 2 exchanged before any transform.
    -> ClsBatch(points [B, N, 3] float64: objfeed.transform of `source` with objfeed.assemble_reference's draws — for a mask
                of 0 exactly the fp32 values of `source`; index [B, N] int32; source [B, N, 3] fp32: the rows taken, swapped;
                recipe [B] int32)
    A shape id outside the pool takes nothing: index -1, zeros.  A pure function of its arguments."""
    sizes = np.asarray(sizes, dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(sizes)))
    rows_xyz = np.asarray(rows_xyz, dtype=np.float32)
    shape_ids = np.asarray(shape_ids, dtype=np.int64).reshape(-1)
    B, N = shape_ids.shape[0], int(num_point)
    if order not in (0, 1) or swap_yz not in (0, 1, False, True):
        raise ValueError("assemble_reference: order and swap_yz are 0 or 1")
    recipe = check_recipe(recipe, B)
    inside = (shape_ids >= 0) & (shape_ids < sizes.shape[0])
    # the draws are a function of the cloud's position in the batch; a shape outside the pool borrows shape 0's size and is blanked
    ref = objfeed.assemble_reference(sizes, np.where(inside, shape_ids, 0), N, seed, step, recipe)
    index = np.full((B, N), -1, dtype=np.int32)
    source = np.zeros((B, N, 3), dtype=np.float32)
    points = np.zeros((B, N, 3), dtype=np.float64)
    for b in range(B):
        if not inside[b]:
            continue
        n = int(sizes[shape_ids[b]])
        if order:
            index[b, :min(n, N)] = np.arange(min(n, N), dtype=np.int32)
        else:
            index[b] = ref.index[b]
        took = index[b] >= 0
        xyz = rows_xyz[int(offsets[shape_ids[b]]) + index[b, took]]
        source[b, took] = xyz[:, [0, 2, 1]] if swap_yz else xyz
        points[b, took] = objfeed.transform(source[b, took], int(recipe[b]), ref.theta[b], ref.tilt[b], ref.scale[b], ref.shift[b])
    return ClsBatch(points, index, source, recipe)


ClsVotes = collections.namedtuple("ClsVotes", "sums pred seen correct nonfinite bad_label class_seen class_correct")


def vote_reference(logits_of_vote, labels, num_cls):
    """The votes of one batch, literally (evaluate_modelnet.py:180-207).  logits_of_vote: per vote [b, C] fp32; labels [b].
    -> ClsVotes(sums [b, C] float64 = np.zeros + every vote's logits in order; pred [b] int32 = np.argmax(sums, 1);
                seen, correct; nonfinite: clouds whose sums hold a NaN or an infinity; bad_label: clouds with a label outside
                [0, C), which count nowhere else; class_seen, class_correct [C] int64)"""
    C = int(num_cls)
    labels = np.asarray(labels).reshape(-1)
    b = labels.shape[0]
    sums = np.zeros((b, C))
    with np.errstate(invalid="ignore", over="ignore"):
        for logits in logits_of_vote:
            logits = np.asarray(logits, dtype=np.float32)
            if logits.shape != (b, C):
                raise ValueError("vote_reference: logits [%d, %d] expected, got %s" % (b, C, logits.shape))
            sums += logits
    pred = np.argmax(sums, 1).astype(np.int32) if b else np.zeros((0,), np.int32)
    seen = correct = nonfinite = bad_label = 0
    class_seen, class_correct = np.zeros((C,), np.int64), np.zeros((C,), np.int64)
    for i in range(b):
        l = int(labels[i])
        if not 0 <= l < C:
            bad_label += 1
            continue
        seen += 1
        class_seen[l] += 1
        nonfinite += int(not np.isfinite(sums[i]).all())
        correct += int(pred[i] == l)
        class_correct[l] += int(pred[i] == l)
    return ClsVotes(sums, pred, seen, correct, nonfinite, bad_label, class_seen, class_correct)


# ---------------------------------------------------------------------------------------------------------------
# the result
# ---------------------------------------------------------------------------------------------------------------
class ClsResult:
    """The figures of an evaluation, in float64 from integer counts with the reference's formulas (evaluate_modelnet.py:212-218):
      accuracy            correct / float(seen)
      class_acc [C]       class_correct / class_seen; NaN where a class was never seen
      mean_class_acc      the mean of class_acc over the classes that were seen.  Whenever every class occurs — the ModelNet40
                          test set — this is the reference's np.mean(total_correct_class / total_seen_class) exactly; where
                          one does not, the reference's figure is NaN
      pred [P] int32      the predicted class per shape of the pool, -1 for a shape this result did not visit
      label [P] int32     the pool's classes
      votes [P, V, C]     fp32 logits of every vote (`pred_votes`; zero rows for shapes not visited) with keep_votes, else None
      seen, correct       the shapes counted and those predicted right; nonfinite: shapes whose sums hold a NaN or an infinity
                          (a broken checkpoint shows here, not as class 0); bad_label: shapes whose class is outside [0, C) —
                          they are predicted but counted nowhere else
      class_seen, class_correct [C] int64;  shapes: the visited shape ids, ascending;  batches: the batch numbers evaluated"""

    def __init__(self, pred, label, seen, correct, nonfinite, bad_label, class_seen, class_correct, shapes, batches, votes=None):
        self.pred, self.label = np.asarray(pred, dtype=np.int32), np.asarray(label, dtype=np.int32)
        self.seen, self.correct, self.nonfinite, self.bad_label = int(seen), int(correct), int(nonfinite), int(bad_label)
        self.class_seen, self.class_correct = np.asarray(class_seen, dtype=np.int64), np.asarray(class_correct, dtype=np.int64)
        self.shapes, self.batches, self.votes = np.asarray(shapes, dtype=np.int64), list(batches), votes
        self.accuracy = self.correct / float(self.seen) if self.seen else float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            self.class_acc = self.class_correct / self.class_seen.astype(np.float64)
        present = self.class_acc[self.class_seen > 0]
        self.mean_class_acc = float(np.mean(present)) if present.size else float("nan")

    @classmethod
    def merge(cls, results):
        """the result of the ranks' shares together: equal to the world = 1 result"""
        results = list(results)
        if not results:
            raise ValueError("merge: no results")
        shapes = np.concatenate([res.shapes for res in results])
        if np.unique(shapes).shape[0] != shapes.shape[0]:
            raise ValueError("merge: a shape occurs in two results")
        first = results[0]
        pred = np.full(first.pred.shape, -1, dtype=np.int32)
        votes = np.zeros(first.votes.shape, np.float32) if all(res.votes is not None for res in results) else None
        for res in results:
            if res.pred.shape != pred.shape or not np.array_equal(res.label, first.label):
                raise ValueError("merge: the results are of different pools")
            pred[res.shapes] = res.pred[res.shapes]
            if votes is not None:
                votes[res.shapes] = res.votes[res.shapes]
        total = lambda name: sum(getattr(res, name) for res in results)
        return cls(pred, first.label, total("seen"), total("correct"), total("nonfinite"), total("bad_label"), total("class_seen"),
                   total("class_correct"), np.sort(shapes), sorted(k for res in results for k in res.batches), votes)


def _share(num_shapes, batch_size, rank, world):
    """-> the batch numbers of rank `rank` and their shape ids"""
    mine = list(range(rank, feed.batches_per_epoch(num_shapes, batch_size), world))
    return mine, [evalvote.batch_blocks(num_shapes, batch_size, i) for i in mine]


def evaluate_reference(logits_fn, category, batch_size, num_cls=40, num_votes=1, rank=0, world=1, keep_votes=False):
    """`evaluate` stated in numpy: vote_reference over the batches of rank `rank`.  category [P]: the pool's classes;
    logits_fn(batch_index, vote) -> [b, C] fp32, the logits the model gave for that vote of that batch."""
    evalvote.check_share(batch_size, rank, world, "evaluate_reference")
    _check_loop_args(1, num_cls, num_votes)
    category = np.asarray(category, dtype=np.int32).reshape(-1)
    P, C, V = category.shape[0], int(num_cls), int(num_votes)
    mine, ids = _share(P, batch_size, rank, world)
    pred = np.full((P,), -1, dtype=np.int32)
    votes = np.zeros((P, V, C), np.float32) if keep_votes else None
    done = []
    for i, s in zip(mine, ids):
        logits = [np.asarray(logits_fn(i, v), dtype=np.float32) for v in range(V)]
        d = vote_reference(logits, category[s], C)
        pred[s] = d.pred
        if keep_votes:
            votes[s] = np.stack(logits, axis=1)
        done.append(d)
    total = lambda name, zero: sum((getattr(d, name) for d in done), zero)
    return ClsResult(pred, category, total("seen", 0), total("correct", 0), total("nonfinite", 0), total("bad_label", 0),
                     total("class_seen", np.zeros((C,), np.int64)), total("class_correct", np.zeros((C,), np.int64)),
                     np.concatenate(ids) if ids else np.zeros((0,), np.int64), mine, votes)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
_CLS_OUT = ((3,),)                  # the shape after [B, N] of points (fp32)


def assemble(rows, offsets, shape_ids, num_point, seed, step, recipe, order=1, swap_yz=False, out=None, want_index=False):
    """sph3d_clsfeed_assemble on torch's current stream.  rows [T, 8] fp32, offsets [P+1] int64, shape_ids [B] int32, all on the
    device.  recipe: a host array of B masks or one mask for all — checked here, a mask that asks for jitter or lies outside
    [0, 15] is refused with Sph3dError (the library has no such path), then uploaded —, or an int32 device tensor [B] that this
    check has seen before its upload.  out: points [B, N, 3] fp32 to write into, else a new tensor.
    -> points (and index [B, N] i32 with want_index)"""
    import torch
    from .. import _lib
    B, N, (points,), index = feed.assemble_args(_lib, rows, offsets, shape_ids, "shape_ids", num_point,
                                                None if out is None else (out,), _CLS_OUT, want_index)
    if order not in (0, 1):
        raise ValueError("assemble: order is 0 (the feed's draw) or 1 (stored order)")
    if torch.is_tensor(recipe):
        _lib.require_device(recipe)
        if recipe.dtype != torch.int32 or tuple(recipe.shape) != (B,) or not recipe.is_contiguous():
            raise ValueError("assemble: a device recipe is a contiguous int32 [B]")
    else:
        r = objfeed.check_recipe(recipe, B)
        if r.max() > MASKS:
            raise _lib.Sph3dError("clsfeed_assemble: masks are in [0, %d] (turn, tilt, scale, shift); there is no jitter" % MASKS)
        recipe = torch.from_numpy(r).to(rows.device)
    _lib.check(_lib.lib().sph3d_clsfeed_assemble(B, N, int(offsets.shape[0]) - 1, int(rows.shape[0]), _lib.ptr(rows),
                                                 _lib.ptr(offsets), _lib.ptr(shape_ids), seed & 0xffffffffffffffff,
                                                 step & 0xffffffffffffffff, _lib.ptr(recipe), int(order), 1 if swap_yz else 0,
                                                 _lib.ptr(points), _lib.ptr(index), _lib.stream_ptr()))
    return (points, index) if want_index else points


class ClassVoter:
    """The device buffers of one classification evaluation and its loop.  Everything the loop needs is uploaded by the
    constructor, in one copy each: the shape ids of all batches of this rank's share, and the two recipes (plain, EVAL_AUGMENT).
    The voter owns, on the device: `sums` [B, C] float64 (reused by every batch), one int32 state vector — pred [P] (-1: not
    visited) | counters [4] | class_seen [C] | class_correct [C] — and, with keep_votes, `votes_out` [P, V, C] fp32.

    run_batch(model_fn, batch_index) issues, for each vote, assemble -> model_fn(points) -> accumulate, then one finalize; it
    performs no device-to-host read and no synchronising copy.  result() reads the state (and the votes) once.
    In stored order (order = 1) every shape of the pool must have at least num_point rows."""

    def __init__(self, pool, batch_size, num_point, num_cls, num_votes, order=1, swap_yz=False, keep_votes=False, seed=0,
                 rank=0, world=1):
        import torch
        _check_loop_args(num_point, num_cls, num_votes)
        evalvote.check_share(batch_size, rank, world, "ClassVoter")
        if order not in (0, 1):
            raise ValueError("ClassVoter: order is 0 (the feed's draw) or 1 (stored order)")
        self.pool, self.B, self.N, self.C, self.V = pool, int(batch_size), int(num_point), int(num_cls), int(num_votes)
        self.order, self.swap_yz, self.seed = int(order), bool(swap_yz), int(seed)
        if self.order and int(np.min(pool.sizes)) < self.N:
            raise ValueError("ClassVoter: in stored order every shape needs at least num_point=%d rows, the smallest has %d"
                             % (self.N, int(np.min(pool.sizes))))
        P, dev = len(pool), pool.device
        self.batches, ids = _share(P, self.B, rank, world)
        if self.batches and self.batches[-1] >= 1 << (63 - evalvote.PASS_BITS):
            raise ValueError("ClassVoter: batch number out of range")
        self._span, at = {}, 0
        for i, s in zip(self.batches, ids):
            self._span[i] = (at, len(s))
            at += len(s)
        self.shapes = np.concatenate(ids).astype(np.int64) if ids else np.zeros((0,), np.int64)
        self.ids_dev = torch.from_numpy(self.shapes.astype(np.int32)).to(dev)
        self.recipes = torch.from_numpy(np.stack([check_recipe(vote_recipe(v), self.B) for v in (0, 1)])).to(dev)
        self.sums = torch.zeros((self.B, self.C), dtype=torch.float64, device=dev)
        self.state = torch.zeros((P + 4 + 2 * self.C,), dtype=torch.int32, device=dev)
        self.pred, self.counters = self.state[:P], self.state[P:P + 4]
        self.class_seen, self.class_correct = self.state[P + 4:P + 4 + self.C], self.state[P + 4 + self.C:]
        self.pred.fill_(-1)
        self.votes_out = torch.zeros((P, self.V, self.C), dtype=torch.float32, device=dev) if keep_votes else None
        self.points = torch.empty((self.B, self.N, 3), dtype=torch.float32, device=dev)
        self.done = []

    def run_batch(self, model_fn, batch_index):
        """all votes of batch `batch_index` (one of this voter's share), then its predictions and counts; nothing is read back"""
        import torch
        from .. import _lib
        if batch_index not in self._span:
            raise ValueError("run_batch: batch %r is not in this voter's share" % (batch_index,))
        if batch_index in self.done:
            raise ValueError("run_batch: batch %d has been evaluated" % batch_index)
        at, b = self._span[batch_index]
        p, l, C, P = self.pool, _lib.lib(), self.C, len(self.pool)
        ids, points = self.ids_dev[at:at + b], self.points[:b]
        for v in range(self.V):
            assemble(p.rows, p.offsets, ids, self.N, self.seed, evalvote.pass_step(batch_index, v), self.recipes[min(v, 1), :b],
                     self.order, self.swap_yz, out=points)
            with torch.no_grad():
                logits = model_fn(points)
            _lib.require_device(logits)
            if tuple(logits.shape) != (b, C):
                raise ValueError("model_fn: logits [%d, %d] expected, got %s" % (b, C, tuple(logits.shape)))
            logits = _lib.f32(logits.detach())
            _lib.check(l.sph3d_cls_vote_accumulate(b, C, _lib.ptr(logits), v, self.V, _lib.ptr(self.sums), _lib.ptr(ids),
                                                   _lib.ptr(self.votes_out), P, _lib.stream_ptr()))
        _lib.check(l.sph3d_cls_vote_finalize(b, C, _lib.ptr(self.sums), _lib.ptr(ids), _lib.ptr(p.category_dev), P,
                                             _lib.ptr(self.pred), _lib.ptr(self.counters), _lib.ptr(self.class_seen),
                                             _lib.ptr(self.class_correct), _lib.stream_ptr()))
        self.done.append(batch_index)

    def result(self):
        """-> ClsResult of the batches run so far: one read of the state vector (and one of the votes with keep_votes)"""
        P, C = len(self.pool), self.C
        state = self.state.cpu().numpy()
        votes = self.votes_out.cpu().numpy() if self.votes_out is not None else None
        counters = state[P:P + 4]
        shapes = [self.shapes[self._span[i][0]:self._span[i][0] + self._span[i][1]] for i in sorted(self.done)]
        return ClsResult(state[:P].copy(), self.pool.category, counters[SEEN], counters[CORRECT], counters[NONFINITE],
                         counters[BAD_LABEL], state[P + 4:P + 4 + C].astype(np.int64), state[P + 4 + C:].astype(np.int64),
                         np.concatenate(shapes) if shapes else np.zeros((0,), np.int64), sorted(self.done), votes)


def evaluate(model_fn, pool, batch_size, num_point, seed, num_cls=40, num_votes=1, rank=0, world=1, order=1, swap_yz=False,
             keep_votes=False):
    """Evaluate a classification network on every shape of `pool` (objfeed.ShapePool) -> ClsResult.

        pool = objio.shape_pool_from_records(test_paths, "modelnet")
        res = evaluate(lambda p: model(p, is_training=False)[0], pool, 32, 10000, seed=0, num_votes=12, swap_yz=True)
        print(res.accuracy, res.mean_class_acc, res.class_acc)

    model_fn(points [b, N, 3] fp32) -> logits [b, num_cls] on the device; it is called under torch.no_grad() on the current
    stream, once per vote, and the tensor it gets is overwritten by the next vote.  Vote 0 sees the plain shape, the votes after
    it EVAL_AUGMENT with the draws of (seed, evalvote.pass_step(batch_index, vote)).  Batch i is shapes
    [i * batch_size, (i + 1) * batch_size) of the pool, the last one at its own size; rank r of `world` takes batches r,
    r + world, ... and ClsResult.merge of the ranks' results equals the world = 1 result.  order = 1 takes the first num_point
    rows of every shape as they are stored (the reference's records hold exactly num_point), order = 0 the feed's sample;
    swap_yz exchanges the y and z columns first, as the reference does for its own records.  keep_votes: the logits of every
    vote come to the host (`pred_votes`).  The host reads the device once, after the last batch."""
    voter = ClassVoter(pool, batch_size, num_point, num_cls, num_votes, order, swap_yz, keep_votes, seed, rank, world)
    for i in voter.batches:
        voter.run_batch(model_fn, i)
    return voter.result()
