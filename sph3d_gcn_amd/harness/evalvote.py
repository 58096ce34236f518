"""Overlap-voting evaluation of the segmentation networks with the votes kept on the device (csrc/vote.hip, include/sph3d.h:
sph3d_vote_begin / _accumulate / _finalize) — what s3dis_seg/evaluate_s3dis_with_overlap.py:219-345 and its ScanNet twin do with
numpy on the host after copying every pass's logits back.

Every test block is sampled to `num_point` points again and again until each of its INNER rows (column 7 of the pool's rows
== 1) has been drawn `min_votes` times (1 for S3DIS; 2 is ScanNet's coverage rule, but its script evaluates three views per draw:
harness/scannet.py); the logits of all passes are summed per block row, the
first maximum of the sums is the row's prediction, and the inner rows' (label, prediction) pairs fill a confusion matrix from
which overall accuracy, class accuracy and IoU follow in float64.  Passes repeat for the whole batch while any of its blocks is
uncovered; blocks that are covered already keep voting.

  * ``vote_reference``: the SPECIFICATION in numpy, no GPU — the pass loop of one batch around a caller's `logits_of_pass`;
    the kernels reproduce counts, coverage, passes, predictions and the confusion matrix exactly and the fp32 vote sums as bit
    patterns (tests/test_gpu_evalvote.py);
  * ``vote_update``: one pass's update of one block under the duplicate rule below;
  * ``metrics``: the reference's formulas on a confusion matrix;
  * ``Voter``: the device buffers of one evaluation and the pass loop of one batch;
  * ``evaluate``: all batches of a pool (or a rank's share of them) -> ``EvalResult``.

THE DUPLICATE RULE.  The reference updates with `sum[index] += logits` and `count[index] += 1`.  With a repeated index numpy's
fancy-index `+=` is not an accumulation: it keeps the LAST occurrence only.  So slot j of a block votes iff no later slot of the
same block drew the same row, and a drawn row receives exactly one logits vector and one count per pass (blocks with fewer
rows than num_point are sampled with replacement, so this happens in every such block).  It is kept, and it makes the sums
reproducible: one fp32 add per row and pass, passes in order, no dependence on thread order.

What differs from the reference, on purpose: the draws are harness/feed.py's counter-based ones with
step = (batch_index << 20) | pass, not numpy's generator, so a batch's votes are a pure function of (seed, batch_index) and do
not depend on how many ranks share the evaluation; the last, smaller batch runs with its own b clouds (the reference pads it
with stale clouds whose outputs it throws away); inner_size is counted from the rows, not read from a block list; the "eval mean
loss" line (the loss of the last pass only) and the .mat dump are not reproduced — `keep_votes` returns the sums instead; and
`max_passes` ends a batch that does not get covered (the result then says `complete == False`), where the reference would loop
on.  The loop reads one word per pass from the device (how many blocks are still uncovered): a host synchronisation per pass.
"""
import collections

import numpy as np

from . import feed

MAX_PASSES = 1 << 12
PASS_BITS = 20
MAX_CLASSES = 64


# ---------------------------------------------------------------------------------------------------------------
# the statement (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def vote_update(votes, count, index, logits):
    """one pass of one block, in place: votes [n, C] fp32, count [n] int32, index [N] (entries outside [0, n) vote nothing),
    logits [N, C] fp32.  The last slot that drew a row votes for it; -> the rows that were drawn"""
    index = np.asarray(index).reshape(-1)
    n, N = votes.shape[0], index.shape[0]
    slots = np.nonzero((index >= 0) & (index < n))[0]
    if slots.size == 0:
        return slots
    # np.unique of the reversed draws gives every row once, with its first position from the end = its last slot
    rows, first = np.unique(index[slots][::-1], return_index=True)
    last = slots[slots.size - 1 - first]
    votes[rows] = votes[rows] + np.asarray(logits, dtype=np.float32).reshape(N, -1)[last]        # one fp32 add per element
    count[rows] += 1
    return rows


def draw_index(sizes, block_ids, num_point, seed, step):
    """-> index [b, N] int32 of one pass: feed.assemble_reference(..., augment=False).index, with rows of -1 for block ids
    outside the pool (what sph3d_feed_assemble writes for them)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    block_ids = np.asarray(block_ids, dtype=np.int64).reshape(-1)
    index = np.full((block_ids.shape[0], int(num_point)), -1, dtype=np.int32)
    for k, i in enumerate(block_ids):
        if 0 <= i < sizes.shape[0]:
            n, ck = int(sizes[i]), feed.cloud_key(seed, step, k)
            index[k] = (feed.sample_without_replacement(ck, n, num_point) if n >= num_point
                        else feed.sample_with_replacement(ck, n, num_point))
    return index


def pass_step(batch_index, p):
    return (int(batch_index) << PASS_BITS) | int(p)


def _check_loop_args(num_point, num_cls, min_votes, max_passes):
    if num_point <= 0 or not 0 < num_cls <= MAX_CLASSES:
        raise ValueError("num_point>0 and 0<num_cls<=%d required" % MAX_CLASSES)
    if min_votes < 1:
        raise ValueError("min_votes>=1 required")
    if not 0 < max_passes < (1 << PASS_BITS):
        raise ValueError("0<max_passes<2^%d required" % PASS_BITS)


def check_share(batch_size, rank, world, what):
    """the arguments that say which share of an evaluation a rank takes"""
    if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError("%s: bad batch_size / rank / world" % what)


def merge_order(results, keys="batches", what="batch", kept="votes"):
    """What the `merge` of the ranks' results has in common.  `keys` names the attribute that lists what a result evaluated
    (batch or scene numbers), `kept` the dict it may have kept per key.  -> (results as a list,
    pick: name -> that per-key attribute of all results in ascending key order — position (key, rank, position) —,
    the `kept` dicts joined, None unless every result has one).  A key that occurs twice is refused."""
    results = list(results)
    if not results:
        raise ValueError("merge: no results")
    rows = sorted((k, r, i) for r, res in enumerate(results) for i, k in enumerate(getattr(res, keys)))
    if len(set(k for k, _, _ in rows)) != len(rows):
        raise ValueError("merge: a %s occurs in two results" % what)
    joined = None
    if all(getattr(res, kept) is not None for res in results):
        joined = {k: v for res in results for k, v in getattr(res, kept).items()}
    return results, (lambda name: [getattr(results[r], name)[i] for _, r, i in rows]), joined


BatchVotes = collections.namedtuple("BatchVotes", "votes count pred passes covered inner_size confusion complete nonfinite_rows")


def vote_reference(sizes, rows_label, rows_inner, block_ids, num_point, seed, batch_index, logits_of_pass, num_cls, min_votes=1,
                   max_passes=MAX_PASSES):
    """The pass loop of one batch.  sizes [P]: rows per block of the pool; rows_label, rows_inner [T]: columns 6 and 7 of the
    pool's rows; block_ids [b]: the batch's blocks (distinct); logits_of_pass(pass, index [b, N] int32) -> [b, N, C] float32.
    -> BatchVotes(votes: per block [n_k, C] fp32 sums, added in pass order with fp32 adds; count: per block [n_k] int32;
                  pred: per block [n_k] int32; passes; covered, inner_size [b] int32; confusion [C, C] int64 (label, pred) of
                  the inner rows with a label in [0, C); complete; nonfinite_rows: rows whose sums are not all finite)
    A block id outside the pool has no rows: empty arrays, inner_size 0."""
    _check_loop_args(num_point, num_cls, min_votes, max_passes)
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
        index = draw_index(sizes, block_ids, num_point, seed, pass_step(batch_index, passes))
        logits = np.asarray(logits_of_pass(passes, index), dtype=np.float32)
        if logits.shape != (b, num_point, C):
            raise ValueError("logits_of_pass: [b, N, C] expected, got %s" % (logits.shape,))
        for k in range(b):
            vote_update(votes[k], count[k], index[k], logits[k])
            covered[k] = np.sum(count[k][inner[k]] >= min_votes)
        passes += 1
    confusion = np.zeros((C, C), dtype=np.int64)
    pred, nonfinite = [], 0
    for k in range(b):
        pr = np.argmax(votes[k], axis=1).astype(np.int32) if votes[k].shape[0] else np.zeros((0,), dtype=np.int32)
        pred.append(pr)
        nonfinite += int((~np.isfinite(votes[k]).all(axis=1)).sum())
        use = inner[k] & (label[k] >= 0) & (label[k] < C)
        np.add.at(confusion, (label[k][use].astype(np.int64), pr[use].astype(np.int64)), 1)
    return BatchVotes(votes, count, pred, passes, covered, inner_size, confusion, not (covered < inner_size).any(), nonfinite)


Metrics = collections.namedtuple("Metrics", "overall_acc class_acc class_iou miou mean_class_acc")


def metrics(confusion):
    """confusion [C, C] (label, prediction) -> Metrics, in float64 with the reference's formulas and its eps
    (evaluate_s3dis_with_overlap.py:331-342): a class that does not occur has accuracy and IoU 0 and counts in the means"""
    cm = np.asarray(confusion, dtype=np.float64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError("metrics: a square confusion matrix expected")
    eps = np.finfo(float).eps
    diag, seen, predicted = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    total = cm.sum()
    overall = float(diag.sum() / total) if total > 0 else float("nan")
    acc = diag / (seen + eps)
    iou = diag / (seen + predicted - diag + eps)
    return Metrics(overall, acc, iou, float(iou.mean()), float(acc.mean()))


# ---------------------------------------------------------------------------------------------------------------
# the result
# ---------------------------------------------------------------------------------------------------------------
class EvalResult:
    """confusion [C, C] int64; passes / covered / inner_size: per evaluated batch, `batches` its number; complete: every batch
    got covered within max_passes; nonfinite_rows: block rows whose vote sums are not all finite (a broken checkpoint shows
    here, not as class 0); votes: {batch number: BatchVotes of host arrays} with keep_votes, else None"""

    def __init__(self, confusion, batches, passes, covered, inner_size, nonfinite_rows, votes=None):
        self.confusion = np.asarray(confusion, dtype=np.int64)
        self.batches, self.passes = list(batches), list(passes)
        self.covered, self.inner_size = list(covered), list(inner_size)
        self.nonfinite_rows, self.votes = int(nonfinite_rows), votes
        self.complete = all((np.asarray(c) >= np.asarray(s)).all() for c, s in zip(self.covered, self.inner_size))
        m = metrics(self.confusion)
        self.overall_acc, self.class_acc, self.class_iou, self.miou, self.mean_class_acc = m

    @classmethod
    def merge(cls, results):
        """the result of the ranks' shares together: equal to the world = 1 result"""
        results, pick, votes = merge_order(results)
        return cls(sum(res.confusion for res in results), pick("batches"), pick("passes"), pick("covered"), pick("inner_size"),
                   sum(res.nonfinite_rows for res in results), votes)


def batch_blocks(num_blocks, batch_size, batch_index):
    """the blocks of batch `batch_index`: consecutive, in pool order (evaluation does not shuffle)"""
    return np.arange(batch_index * batch_size, min(num_blocks, (batch_index + 1) * batch_size), dtype=np.int32)


def evaluate_reference(logits_fn, sizes, rows_label, rows_inner, batch_size, num_point, seed, num_cls=13, min_votes=1,
                       max_passes=MAX_PASSES, rank=0, world=1, keep_votes=False):
    """`evaluate` stated in numpy: vote_reference over the batches of rank `rank`;
    logits_fn(batch_index, pass, index [b, N]) -> [b, N, C] float32"""
    check_share(batch_size, rank, world, "evaluate_reference")
    P, C = len(sizes), int(num_cls)
    mine = list(range(rank, feed.batches_per_epoch(P, batch_size), world))
    done = [vote_reference(sizes, rows_label, rows_inner, batch_blocks(P, batch_size, i), num_point, seed, i,
                           lambda p, index, _i=i: logits_fn(_i, p, index), C, min_votes, max_passes) for i in mine]
    return EvalResult(sum((d.confusion for d in done), np.zeros((C, C), np.int64)), mine, [d.passes for d in done],
                      [d.covered for d in done], [d.inner_size for d in done], sum(d.nonfinite_rows for d in done),
                      dict(zip(mine, done)) if keep_votes else None)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
class Voter:
    """The device buffers of one evaluation — vote sums [capacity_rows, C] fp32, counts, predictions, stamps, the feed's output
    set, the confusion matrix — allocated once and reused by every batch, and the pass loop of one batch.  A batch's blocks
    must lie inside `capacity_rows` consecutive rows of the pool (evaluate sizes it to its largest batch).

    The loop is stated here once; shapeeval.ShapeVoter runs the same one.  What a subclass may replace: `_alloc` (the output set
    and what the closing kernel writes), `_open` (per batch, before anything is launched), `_pass` (what one pass draws and
    feeds to model_fn), `_close` and `_empty` (how a finished batch, or one without rows, becomes a result)."""
    what = "blocks"

    def __init__(self, pool, batch_size, num_point, num_cls, capacity_rows, min_votes=1):
        import torch
        from .. import _lib
        _check_loop_args(num_point, num_cls, min_votes, 1)
        if batch_size <= 0 or capacity_rows <= 0:
            raise ValueError("%s: batch_size>0 and capacity_rows>0 required" % type(self).__name__)
        self.pool, self.B, self.N, self.C = pool, int(batch_size), int(num_point), int(num_cls)
        self.cap, self.min_votes = int(capacity_rows), int(min_votes)
        dev = pool.device
        self.votes = torch.empty((self.cap, self.C), dtype=torch.float32, device=dev)
        self.count = torch.empty((self.cap,), dtype=torch.int32, device=dev)
        self.pred = torch.empty((self.cap,), dtype=torch.int32, device=dev)
        self.ws_bytes = int(_lib.lib().sph3d_vote_workspace(self.cap))
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=dev)
        self.state = torch.zeros((2 * self.B + 1,), dtype=torch.int32, device=dev)        # covered | inner_size | remaining
        self.covered, self.inner_size, self.remaining = self.state[:self.B], self.state[self.B:2 * self.B], self.state[2 * self.B:]
        self.nonfinite = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._alloc(dev)

    def _alloc(self, dev):
        import torch
        self.confusion = torch.zeros((self.C * self.C,), dtype=torch.int64, device=dev)
        self.out = (torch.empty((self.B, self.N, 6), dtype=torch.float32, device=dev),
                    torch.empty((self.B, self.N), dtype=torch.int32, device=dev),
                    torch.empty((self.B, self.N), dtype=torch.int32, device=dev))

    def row_range(self, block_ids):
        """-> (row_base, batch_rows) of the batch's blocks in the pool's rows, None if none of them is in the pool"""
        ids = [int(i) for i in block_ids if 0 <= int(i) < len(self.pool)]
        if len(set(ids)) != len(ids):
            raise ValueError("the %s of a batch are distinct" % self.what)
        if not ids:
            return None
        lo = min(int(self.pool.host_offsets[i]) for i in ids)
        hi = max(int(self.pool.host_offsets[i + 1]) for i in ids)
        if hi - lo > self.cap:
            raise ValueError("the batch's %s span %d rows of the pool, the buffers hold %d" % (self.what, hi - lo, self.cap))
        return lo, hi - lo

    def _open(self, block_ids):
        """per batch, before anything is launched"""

    def _pass(self, model_fn, ids_dev, out, seed, batch_index, p, vote):
        """pass p of a batch: one sample without augmentation, voted as pass p"""
        points, label, inner, index = feed.assemble(self.pool.rows, self.pool.offsets, ids_dev, self.N, seed, pass_step(batch_index, p),
                                                    augment=False, out=out, want_index=True)
        vote(p, index, lambda: model_fn(points, label, inner))

    def _empty(self, b):
        return BatchVotes(None, None, None, 0, np.zeros((b,), np.int32), np.zeros((b,), np.int32), None, True, 0)

    def _close(self, block_ids, common, passes, keep_votes):
        """the batch's predictions and confusion counts (added to self.confusion / self.nonfinite) -> BatchVotes; confusion is
        None (the matrix is accumulated on the device)"""
        from .. import _lib
        before = int(self.nonfinite.item()) if keep_votes else 0
        _lib.check(_lib.lib().sph3d_vote_finalize(len(block_ids), self.C, *common, _lib.ptr(self.votes), _lib.ptr(self.pred),
                                                  _lib.ptr(self.confusion), _lib.ptr(self.nonfinite), _lib.stream_ptr()))
        covered, inner_size = self._coverage(len(block_ids))
        votes, count, pred = self._kept(block_ids, common, keep_votes)
        nonfinite = int(self.nonfinite.item()) - before if keep_votes else 0
        return BatchVotes(votes, count, pred, passes, covered, inner_size, None, bool((covered >= inner_size).all()), nonfinite)

    def _coverage(self, b):
        """-> covered, inner_size [b] of the batch (host)"""
        state = self.state.cpu().numpy()
        return state[:b].copy(), state[self.B:self.B + b].copy()

    def _kept(self, block_ids, common, keep_votes):
        """-> the batch's sums, counts and predictions as per-block host arrays with keep_votes, else None three times"""
        if not keep_votes:
            return None, None, None
        P, base, nrows, offsets = common[0], common[5], common[6], self.pool.host_offsets
        hv, hc, hp = self.votes[:nrows].cpu().numpy(), self.count[:nrows].cpu().numpy(), self.pred[:nrows].cpu().numpy()
        votes, count, pred = [], [], []
        for i in block_ids:
            lo, hi = (int(offsets[i]) - base, int(offsets[i + 1]) - base) if 0 <= i < P else (0, 0)
            votes.append(hv[lo:hi].copy())
            count.append(hc[lo:hi].copy())
            pred.append(hp[lo:hi].copy())
        return votes, count, pred

    def run_batch(self, model_fn, block_ids, seed, batch_index, max_passes=MAX_PASSES, keep_votes=False, on_pass=None):
        """all passes of one batch, then what `_close` makes of it; votes / count / pred of the result are per-block host arrays
        with keep_votes, else None"""
        import torch
        from .. import _lib
        _check_loop_args(self.N, self.C, self.min_votes, max_passes)
        block_ids = np.ascontiguousarray(np.asarray(block_ids).reshape(-1), dtype=np.int32)
        b = int(block_ids.shape[0])
        if not 0 < b <= self.B:
            raise ValueError("a batch has 1..%d %s, got %d" % (self.B, self.what, b))
        if batch_index < 0 or batch_index >= 1 << (63 - PASS_BITS):
            raise ValueError("batch_index out of range")
        self._open(block_ids)
        rng = self.row_range(block_ids)
        if rng is None:
            return self._empty(b)
        p, l = self.pool, _lib.lib()
        ids_dev = torch.from_numpy(block_ids).to(p.device)
        common = (len(p), int(p.rows.shape[0]), _lib.ptr(p.rows), _lib.ptr(p.offsets), _lib.ptr(ids_dev)) + rng
        bufs = (_lib.ptr(self.votes), _lib.ptr(self.count), _lib.ptr(self.covered), _lib.ptr(self.inner_size),
                _lib.ptr(self.remaining), _lib.ptr(self.ws), self.ws_bytes)
        _lib.check(l.sph3d_vote_begin(b, self.C, *common, *bufs, _lib.stream_ptr()))

        def vote(q, index, call):
            with torch.no_grad():
                logits = call()
            _lib.require_device(logits)
            if tuple(logits.shape) != (b, self.N, self.C):
                raise ValueError("model_fn: logits [%d, %d, %d] expected, got %s" % (b, self.N, self.C, tuple(logits.shape)))
            logits = _lib.f32(logits.detach())
            if on_pass is not None:
                on_pass(batch_index, q, index, logits)
            _lib.check(l.sph3d_vote_accumulate(b, self.N, self.C, *common, q, _lib.ptr(index), _lib.ptr(logits), self.min_votes,
                                               *bufs, _lib.stream_ptr()))

        out = tuple(t[:b] for t in self.out)
        passes = 0
        remaining = int(self.remaining.item())
        while remaining > 0 and passes < max_passes:
            self._pass(model_fn, ids_dev, out, seed, batch_index, passes, vote)
            remaining = int(self.remaining.item())               # the loop's one word per pass: a host synchronisation
            passes += 1
        return self._close(block_ids, common, passes, keep_votes)

    def totals(self):
        """-> confusion [C, C] int64 and the non-finite rows counted so far (host)"""
        return self.confusion.cpu().numpy().reshape(self.C, self.C).copy(), int(self.nonfinite.item())


def evaluate(model_fn, pool, batch_size, num_point, seed, num_cls=13, min_votes=1, max_passes=MAX_PASSES, rank=0, world=1,
             keep_votes=False, on_pass=None):
    """Evaluate a network on every block of `pool` (feed.BlockPool) -> EvalResult.

        pool = feed.BlockPool.from_records(test_paths)
        res = evaluate(lambda p, l, i: model(p, is_training=False)[0], pool, 16, 8192, seed=0)
        print(res.miou, res.overall_acc, res.class_iou, res.complete)

    model_fn(points [b, N, 6] fp32, label [b, N] i32, inner [b, N] i32) -> logits [b, N, num_cls] on the device; it is called
    under torch.no_grad() on the current stream, and the tensors it gets are overwritten by the next pass (when it returns,
    everything that reads them must be ordered before later work on the current stream — the project's nets are).
    Batch i is blocks [i * batch_size, (i + 1) * batch_size) of the pool; rank r of `world` takes batches r, r + world, ... and
    EvalResult.merge of the ranks' results equals the world = 1 result.  min_votes: 1 for S3DIS (ScanNet: scannet.evaluate).
    on_pass(batch_index, pass, index, logits): a hook that sees each pass's device tensors before they are voted.
    keep_votes: the finished batches' sums, counts and predictions are copied to the host (result.votes)."""
    _check_loop_args(num_point, num_cls, min_votes, max_passes)
    check_share(batch_size, rank, world, "evaluate")
    mine = list(range(rank, feed.batches_per_epoch(len(pool), batch_size), world))
    C = int(num_cls)
    if not mine:
        return EvalResult(np.zeros((C, C), np.int64), [], [], [], [], 0, {} if keep_votes else None)
    spans = [batch_blocks(len(pool), batch_size, i) for i in mine]
    cap = max(int(pool.host_offsets[ids[-1] + 1] - pool.host_offsets[ids[0]]) for ids in spans)
    voter = Voter(pool, batch_size, num_point, C, cap, min_votes)
    done = [voter.run_batch(model_fn, ids, seed, i, max_passes, keep_votes, on_pass) for i, ids in zip(mine, spans)]
    confusion, nonfinite = voter.totals()
    return EvalResult(confusion, mine, [d.passes for d in done], [d.covered for d in done], [d.inner_size for d in done], nonfinite,
                      dict(zip(mine, done)) if keep_votes else None)
