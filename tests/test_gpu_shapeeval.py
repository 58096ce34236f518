"""csrc/shapeeval.hip and harness/shapeeval.py on the device against the numpy statement (shapeeval.shape_vote_reference /
evaluate_reference): the logits of every evaluation are recorded through `on_pass` and replayed through the statement, so counts,
coverage, draws, predictions, the part counts and every figure of ShapeResult must be equal and the fp32 vote sums equal as bit
patterns.  tests/test_shapeeval.py asserts without a GPU that these loops complete within the caps used here.  Every launch here
is an ordinary one."""
import numpy as np
import pytest

import _shapeeval_cases as cases
from sph3d_gcn_amd.harness import evalvote, feed, objfeed, shapeeval

pytestmark = pytest.mark.gpu


class _Toy:
    """a fixed torch expression of the points: a [3, C] matrix plus a per-row term; it reads the category too"""

    def __init__(self, C, dev, seed=0):
        import torch
        self.w = torch.from_numpy(np.random.RandomState(seed).randn(3, C).astype(np.float32)).to(dev)

    def __call__(self, points, label, category):
        import torch
        phase = torch.arange(self.w.shape[1], device=points.device, dtype=torch.float32) * 0.37
        row = torch.sin(phase + 3.0 * points[:, :, 2:3] + category.reshape(-1, 1, 1).float())
        return (points.unsqueeze(-1) * self.w).sum(dim=2) + row * (1.0 + points[:, :, 0:1])


class _Recorder:
    def __init__(self):
        self.index, self.logits = {}, {}

    def __call__(self, batch_index, q, index, logits):
        assert q == len(self.index.setdefault(batch_index, []))
        self.index[batch_index].append(index.cpu().numpy())
        self.logits.setdefault(batch_index, []).append(logits.cpu().numpy())


def _same_votes(got, want, b):
    assert got.passes == want.passes and got.complete == want.complete
    assert np.array_equal(got.covered, want.covered) and np.array_equal(got.size, want.size)
    for k in range(b):
        assert np.array_equal(got.count[k], want.count[k]), k
        # bit patterns; a NaN only has to be a NaN in both (IEEE 754 leaves the sign and payload of a generated NaN to the machine)
        nan = np.isnan(want.votes[k])
        assert np.array_equal(np.isnan(got.votes[k]), nan), k
        assert np.array_equal(got.votes[k].view(np.int32)[~nan], want.votes[k].view(np.int32)[~nan]), k
        assert np.array_equal(got.pred[k], want.pred[k]), k
    for name in ("inter", "pred_cnt", "gt_cnt", "correct"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.shape_iou, want.shape_iou, equal_nan=True) and got.nonfinite_rows == want.nonfinite_rows


def _same_result(got, want):
    for name in ("shapes", "category", "shape_iou", "correct", "seen", "class_correct", "class_seen"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.category_miou, want.category_miou, equal_nan=True)
    assert np.array_equal(got.class_acc, want.class_acc, equal_nan=True)
    for name in ("mean_category_miou", "instance_miou", "accuracy", "nonfinite_rows", "num_categories", "batches", "passes", "complete"):
        assert getattr(got, name) == getattr(want, name), name
    for c, s, c2, s2 in zip(got.covered, got.size, want.covered, want.size):
        assert np.array_equal(c, c2) and np.array_equal(s, s2)


def _evaluate_and_replay(dev, sizes, C, category, table, min_count, max_passes, seed_shapes, **kw):
    blocks, cat = cases.shapes(sizes, seed_shapes, C, category)
    label = np.concatenate([b[:, 6] for b in blocks])
    pool = objfeed.ShapePool(blocks, cat, table[0], table[1], device=dev)
    rec = _Recorder()
    res = shapeeval.evaluate(_Toy(C, dev), pool, cases.BATCH, cases.NUM_POINT, cases.SEED, C, min_count=min_count,
                             max_passes=max_passes, keep_votes=True, on_pass=rec, **kw)

    def fn(i, q, index):
        assert np.array_equal(index, rec.index[i][q])                      # (the feed's own guarantee: both draws of a pair too)
        return rec.logits[i][q]
    want = shapeeval.evaluate_reference(fn, sizes, label, cat, cases.BATCH, cases.NUM_POINT, cases.SEED, C, table[0], table[1],
                                        min_count, max_passes, keep_votes=True, **kw)
    for i in want.batches:
        assert len(rec.index[i]) == 2 * want.passes[i]
        assert all(np.array_equal(rec.index[i][2 * p], rec.index[i][2 * p + 1]) for p in range(want.passes[i]))
        _same_votes(res.votes[i], want.votes[i], len(want.votes[i].votes))
    _same_result(res, want)
    return res, label


@pytest.mark.parametrize("onehot", [False, True])
def test_the_evaluation_equals_the_numpy_statement_bit_for_bit(dev, onehot):
    """n in {1, 2, 37, 255, 256, 257, 400, 700}, N = 256, batches of 3 (the last one smaller), min_count 3: C = 6 with a
    per-category model, C = 50 with a one-hot table of 16 categories (where every 11th label lies outside its shape's range)"""
    C = 50 if onehot else 6
    category = [3, 10, 0, 15, 7, 3, 10, 1] if onehot else None
    table = (cases.PART_LO, cases.PART_N) if onehot else (None, None)
    res, label = _evaluate_and_replay(dev, cases.SIZES, C, category, table, cases.MIN_COUNT, cases.MAX_PASSES, 4)
    print("C=%d: draws per batch %s, instance mIoU %.4f, accuracy %.4f" % (C, res.passes, res.instance_miou, res.accuracy))
    assert res.complete and res.batches == [0, 1, 2] and res.nonfinite_rows == 0
    assert res.shapes.tolist() == list(range(8)) and res.seen.tolist() == cases.SIZES
    assert 0.0 < res.instance_miou < 1.0 and 0.0 < res.accuracy < 1.0
    if onehot:
        assert res.num_categories == 16 and int(res.class_seen.sum()) < sum(cases.SIZES)       # labels outside the range exist
    else:
        assert int(res.class_seen.sum()) == sum(cases.SIZES)


def test_the_default_min_count_on_one_batch(dev):
    """one batch of shapes with n <= 300 at min_count = 11: every row is drawn more than 10 times"""
    res, _ = _evaluate_and_replay(dev, cases.DEFAULT_SIZES, 6, None, (None, None), shapeeval.MIN_COUNT, cases.DEFAULT_MAX_PASSES, 5)
    assert res.complete and res.batches == [0] and res.passes[0] >= 11
    for k in range(3):
        assert (res.votes[0].count[k] >= 22).all() and (res.votes[0].count[k] % 2 == 0).all()


def test_merged_ranks_equal_one_rank_on_the_device(dev):
    C = 6
    blocks, cat = cases.shapes(cases.SIZES, 4, C, [0, 1, 2, 0, 1, 2, 0, 1])
    pool = objfeed.ShapePool(blocks, cat, device=dev)
    run = lambda rank, world: shapeeval.evaluate(_Toy(C, dev), pool, cases.BATCH, cases.NUM_POINT, cases.SEED, C,
                                                 min_count=cases.MIN_COUNT, max_passes=cases.MAX_PASSES, rank=rank, world=world)
    one = run(0, 1)
    merged = shapeeval.ShapeResult.merge([run(1, 3), run(2, 3), run(0, 3)])
    _same_result(merged, one)
    assert one.complete and one.num_categories == 3 and not np.isnan(one.category_miou).any()


def test_shape_iou_alone_on_hand_made_votes(dev):
    """sph3d_shape_iou on votes written by hand: NaN (a maximum), ties (the first part of the range wins), part_lo > 0, a label
    outside the range, a shape outside the batch's row range and one with an impossible part range (both count nothing and
    write no prediction; the NaN of the latter is not counted either), and stale values in the count buffers (zeroed by the call)"""
    import torch
    from sph3d_gcn_amd import _lib
    C, nan = 5, float("nan")
    sizes = [4, 3, 2, 300, 2]
    gt = [[1, 2, 3, 0], [0, 4, 4], [0, 0], list(np.arange(300) % C), [1, 1]]
    blocks = [objfeed.shape_blocks(np.zeros((n, 3), np.float32), g) for n, g in zip(sizes, gt)]
    pool = feed.BlockPool(blocks, dev)
    votes = np.zeros((sum(sizes), C), np.float32)
    votes[0:4] = [[9, 1, nan, 0, 9], [9, 2, 2, 2, 9], [9, 0, 1, 3, 9], [nan, 0, 0, 0, 9]]          # shape 0, range [1, 4)
    votes[4:7] = [[1, 1, 0, 0, 0], [0, 0, 0, 0, 7], [0, np.inf, 0, 0, 0]]                           # shape 1, range [0, 5)
    votes[7:9] = [[5, 0, 0, 0, nan], [5, 0, 0, 0, 0]]                                               # shape 2: range [3, 3 + 4) > C
    votes[9:309] = np.random.RandomState(0).randn(300, C).astype(np.float32)                        # shape 3, range [0, 5)
    votes[309:311] = [[0, 5, 0, 0, 0], [0, 5, 0, 0, 0]]                                             # shape 4: outside the batch range
    ids = np.array([0, 1, 2, 3, 4, -1, 7], dtype=np.int32)
    b = len(ids)
    plo = np.array([1, 0, 3, 0, 0, 0, 0], dtype=np.int32)
    pn = np.array([3, 5, 4, 5, 5, 5, 5], dtype=np.int32)
    base, nrows = 0, 309                                           # shapes 0..3 only; the votes buffer is [nrows, C]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dv, dids, dlo, dn = t(votes[:nrows]), t(ids), t(plo), t(pn)
    pred = torch.full((nrows,), -7, dtype=torch.int32, device=dev)
    inter, pc, gc = (torch.full((b, C), 99, dtype=torch.int32, device=dev) for _ in range(3))
    correct = torch.full((b,), 99, dtype=torch.int32, device=dev)
    nonfinite = torch.tensor([10], dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().sph3d_shape_iou(b, C, len(pool), int(pool.rows.shape[0]), _lib.ptr(pool.rows), _lib.ptr(pool.offsets),
                                          _lib.ptr(dids), base, nrows, _lib.ptr(dv), _lib.ptr(dlo), _lib.ptr(dn), _lib.ptr(pred),
                                          _lib.ptr(inter), _lib.ptr(pc), _lib.ptr(gc), _lib.ptr(correct), _lib.ptr(nonfinite),
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()
    pred, inter, pc, gc, correct = (x.cpu().numpy() for x in (pred, inter, pc, gc, correct))
    assert pred[0:4].tolist() == [2, 1, 3, 1] and pred[4:7].tolist() == [0, 4, 1] and pred[7:9].tolist() == [-7, -7]
    want_inter, want_pc, want_gc = (np.zeros((b, C), np.int32) for _ in range(3))
    want_correct = np.zeros(b, np.int32)
    for k in (0, 1, 3):
        lo = int(pool.host_offsets[k])
        pr, want_inter[k], want_pc[k], want_gc[k], want_correct[k] = shapeeval.part_counts(
            votes[lo:lo + sizes[k]], np.asarray(gt[k], np.float32), int(plo[k]), int(pn[k]))
        assert np.array_equal(pred[lo:lo + sizes[k]], pr), k
    assert np.array_equal(inter, want_inter) and np.array_equal(pc, want_pc) and np.array_equal(gc, want_gc)
    assert np.array_equal(correct, want_correct) and want_pc[3].sum() == 300
    for k in (2, 4, 5, 6):
        assert not inter[k].any() and not pc[k].any() and not gc[k].any() and correct[k] == 0
    assert want_gc[0].tolist() == [0, 1, 1, 1, 0] and want_correct[0] == 1 and want_correct[1] == 2       # (label 0 of shape 0 is outside [1, 4))
    assert int(nonfinite.item()) == 10 + 3                          # rows 0 and 3 of shape 0 (NaN), row 2 of shape 1 (inf)
    # arguments that describe no launch are refused on the host
    rc = _lib.lib().sph3d_shape_iou(b, 65, len(pool), int(pool.rows.shape[0]), _lib.ptr(pool.rows), _lib.ptr(pool.offsets), _lib.ptr(dids),
                                    base, nrows, _lib.ptr(dv), _lib.ptr(dlo), _lib.ptr(dn), _lib.ptr(t(np.zeros(nrows, np.int32))),
                                    _lib.ptr(t(inter)), _lib.ptr(t(pc)), _lib.ptr(t(gc)), _lib.ptr(t(correct)), _lib.ptr(nonfinite),
                                    _lib.stream_ptr())
    assert rc == -1
    with pytest.raises(ValueError):
        _lib.check(rc)
