"""The training loop of the reference's train_*.py on the device: the learning-rate schedule, the per-step training metrics and
the per-epoch validation, checkpoint and resume — the loop that joins the feeds (harness/feed.py, objfeed.py, facadefeed.py), the
models with their losses, GraphPlan's `points_ready` / `sample_key`, dist.FlatGradAllReduce and the reference's optimisers
(harness/optim.py: FlatTFAdam, FlatNesterov).

    trainer = Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, eps=1e-4), Schedule.for_dataset("s3dis"), 13,
                      line=s3dis_line, prime=(points, label, inner), seed=1)
    trainer.fit(lambda epoch: feed.DeviceFeed(pool, 16, 8192, seed=1), epochs=501,
                eval_feed_factory=lambda epoch: feed.DeviceFeed(test_pool, 16, 8192, seed=2, augment=False), ckpt_dir="log_s3dis")

Reproduced of the reference's loop (s3dis_seg/train_s3dis.py; the other five scripts differ in their flags and the batch's
layout): the staircase schedule with its 1e-6 floor (:95-103), total_loss = the model's loss + the 'losses' collection +
weight_decay * the regularisation losses (:206-210), the update of tf.train.AdamOptimizer / MomentumOptimizer (:223-226), the
accuracy over the inner points and the log lines every 50 batches (:371-384), the one-pass validation with per-class accuracy and
IoU (:461-492), one checkpoint per epoch with max_to_keep = 500 and resume at the epoch after the newest one (:232, :255-288).
NOT reproduced: numpy's random generator (the feeds draw from (seed, step)), TensorBoard summaries, the division of the 50-batch
loss sum by 10 in the training line (:380: its slip; the true mean is reported), and the stale rows a short last batch leaves in
the reference's fixed-size placeholders (:356-358; the feeds hand out the short batch as it is).

No step reads from the device: the counters live there (csrc/train.hip: sph3d_train_metrics), and every `log_every` steps ONE
copy brings the confusion matrix, the counters, the loss sum and the optimiser's count of non-finite gradients to the host.
"""
import collections
import contextlib
import inspect
import os
import re

import numpy as np
import torch

from .. import _lib, _tgraph, tf_gemm, tf_norm
from . import dist as hdist
from . import optim as hoptim

# ---------------------------------------------------------------------------------------------------------------
# the schedule (train_s3dis.py:95-103)
# ---------------------------------------------------------------------------------------------------------------
# the scripts' flags: batch_size, learning_rate, decay_step, decay_rate, momentum and the epsilon of their AdamOptimizer.
# train_shapenet.py has no decay_step flag: it is 36 x the number of training shapes of the category (:94), the caller's to give.
DEFAULTS = {
    "s3dis": dict(batch_size=16, base=1e-3, decay_step=250000, decay_rate=0.7, momentum=0.9, eps=1e-4),
    "ruemonge": dict(batch_size=16, base=1e-3, decay_step=250000, decay_rate=0.7, momentum=0.9, eps=1e-4),
    "scannet": dict(batch_size=16, base=1e-3, decay_step=500000, decay_rate=0.7, momentum=0.9, eps=1e-4),
    "shapenet_onehot": dict(batch_size=32, base=1e-3, decay_step=320000, decay_rate=0.7, momentum=0.9, eps=1e-4),
    "shapenet": dict(batch_size=32, base=1e-3, decay_step=None, decay_rate=0.7, momentum=0.9, eps=1e-8),
    "modelnet": dict(batch_size=32, base=1e-3, decay_step=250000, decay_rate=0.7, momentum=0.9, eps=1e-8),
}


def learning_rate(global_step, base, batch_size, decay_step, decay_rate, floor=1e-6):
    """max(base * decay_rate ** floor(global_step * batch_size / decay_step), floor): tf.train.exponential_decay(staircase=True)
    clipped from below.  global_step is the number of updates already done: 0 for the first."""
    if global_step < 0 or batch_size <= 0 or decay_step <= 0:
        raise ValueError("learning_rate: global_step >= 0, batch_size > 0 and decay_step > 0 required")
    return max(float(base) * float(decay_rate) ** ((int(global_step) * int(batch_size)) // int(decay_step)), float(floor))


class Schedule:
    """learning_rate with its settings bound: schedule(global_step) -> the step's learning rate"""

    def __init__(self, base=1e-3, batch_size=16, decay_step=250000, decay_rate=0.7, floor=1e-6):
        if decay_step is None:
            raise ValueError("Schedule: decay_step required (train_shapenet.py: 36 x the category's training shapes)")
        self.base, self.batch_size, self.decay_step = float(base), int(batch_size), int(decay_step)
        self.decay_rate, self.floor = float(decay_rate), float(floor)

    @classmethod
    def for_dataset(cls, name, **override):
        d = dict(DEFAULTS[name], **override)
        return cls(d["base"], d["batch_size"], d["decay_step"], d["decay_rate"])

    def settings(self):
        return dict(base=self.base, batch_size=self.batch_size, decay_step=self.decay_step, decay_rate=self.decay_rate, floor=self.floor)

    def __call__(self, global_step):
        return learning_rate(global_step, **self.settings())


# ---------------------------------------------------------------------------------------------------------------
# the metrics: the numpy statement and the device counters
# ---------------------------------------------------------------------------------------------------------------
NUM_COUNTERS = 5            # seen, correct, bad_label, nonfinite, batches
MAX_CLASSES = 64            # csrc/common.hpp: kVoteMaxClasses


def metrics_reference(logits, label, inner=None, loss_part=None, state=None):
    """What one sph3d_train_metrics call adds, in numpy.  logits [B, N, C] fp32, label [B, N], inner [B, N] or None (every row
    counts), loss_part: fp32 values or None.  state: (confusion int64 [C, C], counters int64 [5], loss_sum float64 [1]) to add
    to (modified in place and returned), default zeros.  A counted row (inner > 0) with a label outside [0, C) adds to
    counters[2] and nothing else; any other counted row adds to confusion[label, first maximum of its logits (np.argmax: a NaN
    counts as a maximum)], to seen, to correct when they agree, and to counters[3] when a logit of the row is not finite.
    counters[4] counts the calls; loss_sum grows by the loss parts, added in index order in float64."""
    logits = np.asarray(logits, dtype=np.float32)
    B, N, C = logits.shape
    label = np.asarray(label).reshape(B * N).astype(np.int64)
    if state is None:
        state = (np.zeros((C, C), np.int64), np.zeros((NUM_COUNTERS,), np.int64), np.zeros((1,), np.float64))
    confusion, counters, loss_sum = state
    counted = np.ones((B * N,), bool) if inner is None else np.asarray(inner).reshape(B * N) > 0
    rows = logits.reshape(B * N, C)
    in_range = (label >= 0) & (label < C)
    use = counted & in_range
    pred = np.argmax(rows[use], axis=1) if use.any() else np.zeros((0,), np.int64)
    np.add.at(confusion, (label[use], pred), 1)
    counters[0] += int(use.sum())
    counters[1] += int((pred == label[use]).sum())
    counters[2] += int((counted & ~in_range).sum())
    counters[3] += int((~np.isfinite(rows[use]).all(axis=1)).sum())
    counters[4] += 1
    if loss_part is not None:
        acc = float(loss_sum[0])
        for x in np.asarray(loss_part, dtype=np.float32).reshape(-1):
            acc += float(x)
        loss_sum[0] = acc
    return state


MetricsResult = collections.namedtuple(
    "MetricsResult", "confusion seen correct bad_label nonfinite batches loss_sum update_nonfinite accuracy class_acc class_iou "
                     "mean_class_acc mean_iou mean_loss")


def derive(confusion, counters, loss_sum, update_nonfinite=0):
    """the figures the reference prints (train_s3dis.py:381, :479-492), in float64, from the counts: overall accuracy
    correct / seen; per class correct_c / (seen_c + eps) and correct_c / (union_c + eps) with eps = np.finfo(float).eps, and their
    means over ALL C classes; the mean loss per batch — the true mean (the reference's training line divides the sum of 50
    batches by 10, :380: its slip, not reproduced)."""
    confusion = np.asarray(confusion, dtype=np.int64)
    seen, correct, bad_label, nonfinite, batches = (int(x) for x in counters)
    eps = np.finfo(float).eps
    seen_c = confusion.sum(axis=1).astype(np.float64)              # rows: the label
    pred_c = confusion.sum(axis=0).astype(np.float64)
    correct_c = np.diag(confusion).astype(np.float64)
    union_c = seen_c + pred_c - correct_c
    class_acc = correct_c / (seen_c + eps)
    class_iou = correct_c / (union_c + eps)
    return MetricsResult(confusion, seen, correct, bad_label, nonfinite, batches, float(loss_sum), int(update_nonfinite),
                         correct / float(seen) if seen else float("nan"), class_acc, class_iou, float(class_acc.mean()),
                         float(class_iou.mean()), float(loss_sum) / batches if batches else float("nan"))


class TrainMetrics:
    """The counters of the training metrics on `device`, in ONE int64 buffer: confusion [C*C], the five counters, the loss sum
    (a double in an 8-byte word) and `update_nonfinite`, a word an optimiser may count its non-finite gradients in
    (optim.FlatTFAdam.nonfinite).  add() is one launch (on CPU tensors: metrics_reference), read() the one copy to the host."""

    def __init__(self, C, device):
        if not 0 < int(C) <= MAX_CLASSES:
            raise _lib.Sph3dError("TrainMetrics: 0 < C <= %d classes are supported, got %d" % (MAX_CLASSES, C))
        self.C, self.device = int(C), torch.device(device)
        cc = self.C * self.C
        self.buf = torch.zeros(cc + NUM_COUNTERS + 2, dtype=torch.int64, device=self.device)
        self.confusion = self.buf[:cc]
        self.counters = self.buf[cc:cc + NUM_COUNTERS]
        self.loss_sum = self.buf[cc + NUM_COUNTERS:cc + NUM_COUNTERS + 1].view(torch.float64)
        self.update_nonfinite = self.buf[cc + NUM_COUNTERS + 1:]

    def reset(self):
        self.buf.zero_()            # (an asynchronous fill on the current stream)

    def add(self, pred, label, inner=None, loss_part=None):
        """pred [B, N, C] (or [B, C]: N = 1) logits, label [B, N] ([B]), inner [B, N] or None, loss_part: fp32 values or None.
        The feeds yield int32 labels and fp32 logits: anything else is converted here."""
        pred = pred.detach()
        if pred.dim() == 2:
            pred = pred.unsqueeze(1)
        B, N, C = pred.shape
        if C != self.C or label.numel() != B * N or (inner is not None and inner.numel() != B * N):
            raise ValueError("TrainMetrics.add: pred [B, N, %d], label and inner [B, N] expected" % self.C)
        if loss_part is not None:
            loss_part = loss_part.detach().reshape(-1)
        if not pred.is_cuda:
            cc = self.C * self.C
            host = self.buf.numpy()
            state = (host[:cc].reshape(self.C, self.C), host[cc:cc + NUM_COUNTERS], host[cc + NUM_COUNTERS:cc + NUM_COUNTERS + 1].view(np.float64))
            metrics_reference(pred.float().numpy(), label.numpy(), None if inner is None else inner.numpy(),
                              None if loss_part is None else loss_part.float().numpy(), state)
            return
        pred, label = _lib.f32(pred), _lib.i32(label)
        inner = _lib.i32(inner) if inner is not None else None
        loss_part = _lib.f32(loss_part) if loss_part is not None else None
        _lib.check(_lib.lib().sph3d_train_metrics(B, N, C, _lib.ptr(pred), _lib.ptr(label), _lib.ptr(inner), _lib.ptr(loss_part),
                                                  loss_part.numel() if loss_part is not None else 0, _lib.ptr(self.confusion),
                                                  _lib.ptr(self.counters), _lib.ptr(self.loss_sum), _lib.stream_ptr()))

    def read(self):
        """-> MetricsResult: confusion [C, C] (rows: the label), seen, correct, bad_label, nonfinite, batches, loss_sum,
        update_nonfinite, and what derive() makes of them.  The one host read (it waits for the work issued so far)."""
        host = self.buf.cpu().numpy()
        cc = self.C * self.C
        return derive(host[:cc].reshape(self.C, self.C).copy(), host[cc:cc + NUM_COUNTERS],
                      host[cc + NUM_COUNTERS:cc + NUM_COUNTERS + 1].view(np.float64)[0], host[cc + NUM_COUNTERS + 1])


# ---------------------------------------------------------------------------------------------------------------
# the dataset lines: what an item of a feed (without its ready event) is to the model, the loss and the metrics
# ---------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "inputs loss_args label inner")


def s3dis_line(item):
    """S3DIS (feed.DeviceFeed) / ScanNet (scannet.ScanNetFeed): points [B, N, 6], label, inner [B, N]"""
    points, label, inner = item
    return Batch((points,), (label, inner), label, inner)


def shapenet_line(item):
    """ShapeNet, one network per category (objfeed.ObjectFeed): points [B, N, 3], label [B, N], category [B]"""
    points, label, _category = item
    return Batch((points,), (label,), label, None)


def shapenet_onehot_line(item):
    """ShapeNet one-hot: the category goes into the model"""
    points, label, category = item
    return Batch((points, category), (label,), label, None)


def modelnet_line(item):
    """ModelNet40 (objfeed.ObjectFeed, dataset="modelnet"): the shape's class is repeated on every point of label"""
    points, label, _category = item
    cls = label[:, 0].contiguous()
    return Batch((points,), (cls,), cls, None)


def ruemonge_line(item):
    """RueMonge2014 (facadefeed.FacadeFeed): points [B, N, 9], label [B, N]"""
    points, label = item
    return Batch((points,), (label,), label, None)


LINES = {"s3dis": s3dis_line, "scannet": s3dis_line, "shapenet": shapenet_line, "shapenet_onehot": shapenet_onehot_line,
         "modelnet": modelnet_line, "ruemonge": ruemonge_line}

# ---------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------
_CKPT = re.compile(r"^model\.ckpt-(\d+)\.pt$")


def checkpoint_path(ckpt_dir, epoch):
    return os.path.join(ckpt_dir, "model.ckpt-%d.pt" % epoch)


def checkpoints(ckpt_dir):
    """-> [(epoch, path)] of the directory's checkpoints, oldest epoch first"""
    if not os.path.isdir(ckpt_dir):
        return []
    found = [(int(m.group(1)), os.path.join(ckpt_dir, f)) for f in os.listdir(ckpt_dir) for m in [_CKPT.match(f)] if m]
    return sorted(found)


def latest_checkpoint(ckpt_dir):
    """the checkpoint of the highest epoch, or None (tf.train.latest_checkpoint)"""
    found = checkpoints(ckpt_dir)
    return found[-1][1] if found else None


# ---------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------
class Trainer:
    """model: one of the harness's nets (its variables are created by its first forward); loss_fn(pred, *loss_args): the model's
    classification loss — the 'losses' collection and weight_decay * the regularisation losses are added here when the model's
    config has a weight_decay (so for the ModelNet net pass modelnet_net.get_loss, not model.loss, which adds them itself);
    optimizer_factory(flat_param) -> an optimiser of harness/optim.py; schedule(global_step) -> the learning rate; num_cls: C.
    line: the dataset line (LINES); prime: one item of the feed without its event — any batch of the training shapes: the
    constructor runs ONE forward on it in inference mode without gradients, which creates the variables in their usual order
    and leaves the moving statistics untouched, then moves the parameters into the flat buffers.  No update, no step counted.
    seed: the feed's seed, with global_step the `sample_key` of every plan.  grad_scale: what the optimiser multiplies the summed
    gradient by (1 / world size for a loss that is a mean over the global batch).  sync_bn: train_step runs its forward and
    backward pass under tf_norm.sync(hdist.stat_all_reduce) — batch-norm statistics over the global batch; every
    rank must then run the same layer sequence with at least one row per layer (the ranks' row counts may differ: the count
    travels in the collective's buffer).  Evaluation is inference mode and issues no collective.  deterministic: train_step,
    eval_one_epoch and fit run under sph3d_gcn_amd.deterministic() — on one rank the same seed then gives the same bits, run after
    run and across a resume; the mode is back at its previous value when they return.  keyed_dropout: a model
    whose forward takes `dropout_key` (the ModelNet net) is called with dropout_key = (seed, global_step) and dropout_row0 =
    rank * B, so its dropout masks are draws of (seed, step) like the feed's — a checkpoint holds no generator state, and only
    then does a resumed run drop what the uninterrupted one drops; None follows `deterministic`.  Other models are called as
    before.  matmul_precision: "highest" | "high" | "medium" — train_step, eval_one_epoch and fit run under
    sph3d_gcn_amd.float32_matmul_precision(level) and the process setting is back at its previous value when they
    return; None leaves the process setting alone.  clip_norm, skip_nonfinite, ema_decay: the guarded update (optim.Guard,
    DESIGN.md 4.29) — with all three absent no guard exists and the step is the plain one.  The guard runs after the gradient's
    all-reduce, so every rank takes the same decision from the same summed gradient.  With skip_nonfinite the model's float32
    buffers (the batch-norm moving statistics, written by the forward pass before anyone knows the step is bad) become views of
    one flat buffer: a device copy is taken before the forward pass and put back after a skipped update, decided on the device
    like the skip itself; train_one_epoch then raises when more than skip_limit steps of a log interval were skipped.  With
    ema_decay, eval_one_epoch evaluates the averaged weights (`with trainer.ema_weights():`)."""

    def __init__(self, model, loss_fn, optimizer_factory, schedule, num_cls, line=s3dis_line, prime=None, seed=0, log_every=50,
                 max_to_keep=500, grad_scale=1.0, class_names=None, log=print, sync_bn=False, deterministic=False, keyed_dropout=None,
                 matmul_precision=None, clip_norm=None, skip_nonfinite=False, ema_decay=None, skip_limit=10):
        if prime is None:
            raise ValueError("Trainer: `prime` (one batch of the training shapes) is needed to create the variables")
        self.model, self.loss_fn, self.schedule, self.line = model, loss_fn, schedule, line
        self.num_cls, self.seed, self.log_every, self.max_to_keep = int(num_cls), int(seed), int(log_every), int(max_to_keep)
        self.class_names = list(class_names) if class_names is not None else ["class %d" % c for c in range(self.num_cls)]
        self.log = log
        self.sync_bn = bool(sync_bn)
        self.deterministic = bool(deterministic)
        if matmul_precision is not None and matmul_precision not in ("highest", "high", "medium"):
            raise ValueError("Trainer: matmul_precision should be None, 'highest', 'high' or 'medium', got %r" % (matmul_precision,))
        self.matmul_precision = matmul_precision
        self.keyed_dropout = (self.deterministic if keyed_dropout is None else bool(keyed_dropout)) and \
            "dropout_key" in inspect.signature(model.forward).parameters
        self.global_step, self.epoch = 0, -1           # updates done; the last finished epoch
        self.rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        batch = self.line(tuple(prime))
        with torch.no_grad():
            self.model(*batch.inputs, is_training=False)
        self.flat = hdist.FlatGradAllReduce(self.model.parameters())
        self.device = self.flat.flat_param.device
        self.opt = optimizer_factory(self.flat.flat_param)
        self.metrics = TrainMetrics(self.num_cls, self.device)
        self.eval_metrics = TrainMetrics(self.num_cls, self.device)
        if hasattr(self.opt, "grad_scale"):
            self.opt.grad_scale = float(grad_scale)
        if hasattr(self.opt, "nonfinite"):
            self.opt.nonfinite = self.metrics.update_nonfinite          # (read with the metrics: no copy of its own)
        self.flat.broadcast_params()
        self.guard, self.skip_limit = None, int(skip_limit)
        self._buf_flat = self._buf_copy = None
        self._guard_seen = None                                         # the GuardStats of the last log interval's read
        if clip_norm is not None or skip_nonfinite or ema_decay is not None:
            guard = hoptim.Guard(clip_norm, skip_nonfinite, ema_decay)
            if not isinstance(self.opt, hoptim._FlatRule):
                raise ValueError("Trainer: clip_norm / skip_nonfinite / ema_decay need FlatTFAdam or FlatNesterov, %s has no guarded "
                                 "update" % type(self.opt).__name__)
            self.opt.guard = guard
            self.guard = guard.bind(self.flat.flat_param)               # (after the broadcast: the EMA starts from rank 0's weights)
            self._guard_seen = hoptim.GuardStats(0, 0, 0, 0.0, 0.0)
            if guard.skip_nonfinite:
                self._flatten_buffers()

    def _flatten_buffers(self):
        """the model's float32 buffers as views of ONE flat buffer, each on a 16-byte boundary (as FlatGradAllReduce lays the
        parameters out), and a second buffer of the same size for the copy a step takes before its forward pass"""
        bufs = [b for _n, b in self.model.named_buffers() if b.dtype == torch.float32]
        n = sum((b.numel() + 3) // 4 * 4 for b in bufs)
        if n == 0:
            return
        self._buf_flat = torch.zeros(n, dtype=torch.float32, device=self.device)
        off = 0
        with torch.no_grad():
            for b in bufs:
                k = b.numel()
                self._buf_flat[off:off + k].copy_(b.reshape(-1))
                b.data = self._buf_flat[off:off + k].view_as(b)
                off += (k + 3) // 4 * 4
        self._buf_copy = torch.empty_like(self._buf_flat)

    # ---- one step --------------------------------------------------------------------------------------------
    def _total_loss(self, pred, batch):
        loss = self.loss_fn(pred, *batch.loss_args)
        wd = getattr(self.model.config, "weight_decay", None)
        store = getattr(self.model, "store", None)
        if wd is not None and store is not None:          # train_s3dis.py:206-210
            extra = store.collect_losses()
            if extra is not None:
                loss = loss + extra
            reg = store.regularization_loss()
            if reg is not None:
                loss = loss + wd * reg
        return loss

    def _forward(self, item, is_training):
        ready = item[-1]
        batch = self.line(tuple(item[:-1]))
        extra = {}
        if self.keyed_dropout:
            extra = dict(dropout_key=(self.seed, self.global_step), dropout_row0=self.rank * batch.inputs[0].shape[0])
        pred, _ = self.model(*batch.inputs, is_training=is_training, points_ready=ready, sample_key=(self.seed, self.global_step), **extra)
        if ready is not None and pred.is_cuda:
            torch.cuda.current_stream().wait_event(ready)       # (the loss reads the labels on this stream)
        return batch, pred, self._total_loss(pred, batch), ready

    def _mode(self):
        if self.matmul_precision is None:
            return _tgraph.deterministic(True) if self.deterministic else contextlib.nullcontext()
        stack = contextlib.ExitStack()          # (entered here, left by the caller's `with`)
        stack.enter_context(tf_gemm.float32_matmul_precision(self.matmul_precision))
        if self.deterministic:
            stack.enter_context(_tgraph.deterministic(True))
        return stack

    def train_step(self, item, feed=None):
        """plan / forward, loss, backward, all-reduce, update, metrics; nothing is read from the device"""
        with self._mode():
            self._train_step(item, feed)

    def _train_step(self, item, feed):
        # sync_bn: every training-mode batch norm takes its statistics over all ranks' rows, one small all-reduce per layer and
        # direction (every rank runs the same layers, each with at least one row; the row counts may differ)
        if self._buf_flat is not None:
            self._buf_copy.copy_(self._buf_flat)         # the moving statistics as they are before the forward pass touches them
        with (tf_norm.sync(hdist.stat_all_reduce) if self.sync_bn else contextlib.nullcontext()):
            batch, pred, loss, ready = self._forward(item, True)
            self.flat.backward(loss)
        self.flat.all_reduce()
        self.opt.lr = self.schedule(self.global_step)
        self.opt.step()
        if self._buf_flat is not None:
            self.guard.restore(self._buf_flat, self._buf_copy)          # (writes only when the update was skipped)
        self.metrics.add(pred, batch.label, batch.inner, loss.detach().reshape(1))
        if ready is not None and feed is not None and hasattr(feed, "done"):
            feed.done(ready)
        self.global_step += 1

    def _check(self, r, first_step, skipped=None):
        """skipped: the steps of the interval that a skip_nonfinite guard skipped, None without such a guard.  Those steps changed
        nothing, so their non-finite rows and gradient elements are no reason to stop (every step whose gradient had one WAS
        skipped; non-finite rows without a skipped step stop the run as before); too many of them are."""
        if skipped is not None:
            if skipped > self.skip_limit:
                raise _lib.Sph3dError("training skipped %d of the steps %d..%d (skip_limit %d): %d rows with non-finite logits, %d "
                                      "non-finite gradient elements" % (skipped, first_step, self.global_step - 1, self.skip_limit,
                                                                        r.nonfinite, r.update_nonfinite))
            if skipped > 0 or not r.nonfinite:
                return
        if r.nonfinite or r.update_nonfinite:
            raise _lib.Sph3dError("training diverged in steps %d..%d: %d rows with non-finite logits, %d non-finite gradient elements"
                                  % (first_step, self.global_step - 1, r.nonfinite, r.update_nonfinite))

    def _guard_interval(self):
        """with a guard: one read of its state, the interval's log line -> the steps skipped since the last read (None unless
        the guard skips)"""
        if self.guard is None:
            return None
        now, was = self.guard.read(), self._guard_seen
        self._guard_seen = now
        if self.rank == 0:
            self.log('guard: applied %d skipped %d clipped %d (run: %d / %d / %d) last norm %g max norm %g'
                     % (now.applied - was.applied, now.skipped - was.skipped, now.clipped_steps - was.clipped_steps, now.applied,
                        now.skipped, now.clipped_steps, now.last_norm, now.max_norm_seen))
        return now.skipped - was.skipped if self.guard.skip_nonfinite else None

    def train_one_epoch(self, feed):
        """feed: any iterable of a feed's items (the last element: the ready event or None).  Every log_every steps one read,
        the reference's two log lines (:379-381, with the true mean loss) and a reset; a last read at the end of the epoch.
        -> the MetricsResult of every read"""
        self.metrics.reset()
        out, first, idx = [], self.global_step, 0
        for idx, item in enumerate(feed, 1):
            self.train_step(item, feed)
            if idx % self.log_every == 0:
                r = self.metrics.read()
                self.metrics.reset()
                out.append(r)
                if self.rank == 0:
                    self.log(' ---- batch: %03d ----' % idx)
                    self.log('mean loss: %f' % r.mean_loss)
                    self.log('accuracy: %f' % r.accuracy)
                self._check(r, first, self._guard_interval())
                first = self.global_step
        if idx % self.log_every != 0:
            r = self.metrics.read()
            self.metrics.reset()
            out.append(r)
            self._check(r, first, self._guard_interval())
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """inside, the model's parameters are the averaged weights and the guard's EMA buffer holds the live ones; on the way
        out they are exchanged back, bit for bit.  Take no training step inside."""
        if self.guard is None or self.guard.ema is None:
            raise _lib.Sph3dError("Trainer.ema_weights: no EMA (construct the Trainer with ema_decay)")
        p, e = self.flat.flat_param.data, self.guard.ema

        def exchange():
            with torch.no_grad():
                tmp = p.clone()
                p.copy_(e)
                e.copy_(tmp)
        exchange()
        try:
            yield
        finally:
            exchange()

    def eval_one_epoch(self, feed, use_ema=None):
        """one pass without voting (train_s3dis.py:394-495): inference mode, no gradients (the loss without its gradient pass),
        one read at the end and the reference's evaluation lines -> MetricsResult.  use_ema: evaluate the averaged weights
        (ema_weights()); None: yes when an EMA exists"""
        has_ema = self.guard is not None and self.guard.ema is not None
        if use_ema is None:
            use_ema = has_ema
        with (self.ema_weights() if use_ema else contextlib.nullcontext()):
            return self._eval_one_epoch(feed)

    def _eval_one_epoch(self, feed):
        m = self.eval_metrics
        m.reset()
        with self._mode(), torch.no_grad():
            for item in feed:
                batch, pred, loss, ready = self._forward(item, False)
                m.add(pred, batch.label, batch.inner, loss.reshape(1))
                if ready is not None and hasattr(feed, "done"):
                    feed.done(ready)
        r = m.read()
        if self.rank == 0:
            self.log('eval mean loss: %f' % r.mean_loss)
            self.log('eval overall accuracy: %f' % r.accuracy)
            self.log('eval avg class acc: %f' % r.mean_class_acc)
            for c, name in enumerate(self.class_names):
                self.log('eval mIoU of %s:\t %f' % (name, r.class_iou[c]))
            self.log('eval mIoU of all classes: %f' % r.mean_iou)
        if r.nonfinite:
            raise _lib.Sph3dError("evaluation after step %d: %d rows with non-finite logits" % (self.global_step, r.nonfinite))
        return r

    # ---- checkpoints ------------------------------------------------------------------------------------------
    def save(self, ckpt_dir, epoch=None):
        """model.ckpt-<epoch>.pt: the model's state_dict (moving statistics included), the optimiser's (with a guard: its state
        and the averaged weights, so both copies of the weights), global_step, epoch, the schedule's settings and the feed seed;
        rank 0 writes, and prunes the oldest beyond max_to_keep -> the path"""
        epoch = self.epoch if epoch is None else int(epoch)
        path = checkpoint_path(ckpt_dir, epoch)
        if self.rank != 0:
            return path
        os.makedirs(ckpt_dir, exist_ok=True)
        state = {"model": {k: v.detach().clone() for k, v in self.model.state_dict().items()}, "optimizer": self.opt.state_dict(),
                 "global_step": self.global_step, "epoch": epoch, "seed": self.seed, "num_cls": self.num_cls}
        if hasattr(self.schedule, "settings"):
            state["schedule"] = self.schedule.settings()
        torch.save(state, path + ".tmp")
        os.replace(path + ".tmp", path)
        found = checkpoints(ckpt_dir)
        for _e, old in found[:max(0, len(found) - self.max_to_keep)]:
            os.remove(old)
        return path

    def load(self, path):
        """copies the saved values INTO the live tensors (the parameters stay views of the flat buffer), restores the optimiser,
        global_step, epoch, the schedule's settings and the seed, then broadcasts the parameters from rank 0"""
        state = torch.load(path, map_location=self.device, weights_only=True)
        live = self.model.state_dict()
        if set(live) != set(state["model"]):
            raise _lib.Sph3dError("checkpoint %s holds other variables than the model" % path)
        with torch.no_grad():
            for k, t in live.items():
                if t.shape != state["model"][k].shape:
                    raise _lib.Sph3dError("checkpoint %s: %s has another shape" % (path, k))
                t.copy_(state["model"][k])
        self.opt.load_state_dict(state["optimizer"])
        self.global_step, self.epoch, self.seed = int(state["global_step"]), int(state["epoch"]), int(state["seed"])
        if "schedule" in state and hasattr(self.schedule, "settings"):
            self.schedule.__init__(**state["schedule"])
        self.flat.broadcast_params()
        if self.guard is not None:
            self._guard_seen = self.guard.read()
        return state

    def fit(self, train_feed_factory, epochs, eval_feed_factory=None, ckpt_dir=None):
        """train_feed_factory(epoch) / eval_feed_factory(epoch) -> the epoch's iterable (a feed whose `epoch` attribute counts
        its epochs is set to `epoch`: its batches are functions of (seed, epoch, step) alone).  With ckpt_dir the newest
        checkpoint there is loaded first and training continues at the epoch after it (train_s3dis.py:255-288); one checkpoint
        is written per epoch."""
        with self._mode():
            self._fit(train_feed_factory, epochs, eval_feed_factory, ckpt_dir)

    def _fit(self, train_feed_factory, epochs, eval_feed_factory, ckpt_dir):
        if ckpt_dir is not None:
            newest = latest_checkpoint(ckpt_dir)
            if newest is not None:
                self.load(newest)
        for epoch in range(self.epoch + 1, int(epochs)):
            if self.rank == 0:
                self.log('**** EPOCH %03d ****' % epoch)
            feed = train_feed_factory(epoch)
            if hasattr(feed, "epoch"):
                feed.epoch = epoch
            self.train_one_epoch(feed)
            if eval_feed_factory is not None:
                self.eval_one_epoch(eval_feed_factory(epoch))
            self.epoch = epoch
            if ckpt_dir is not None:
                self.save(ckpt_dir, epoch)
