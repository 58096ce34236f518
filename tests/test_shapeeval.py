"""harness/shapeeval.py without a GPU: the numpy statement of the ShapeNet evaluation against a literal restatement of the
reference's loop (shapenet_seg/evaluate_shapenet.py:228-289, evaluate_shapenet_onehot.py:283-334) with this module's draws
injected, hand cases, the merge of ranks, and the completeness of the loops tests/test_gpu_shapeeval.py runs."""
import numpy as np
import pytest

import _shapeeval_cases as cases
from sph3d_gcn_amd.harness import evalvote, shapeeval


def _logits(b, N, C, q, index, salt=0):
    """a deterministic float32 "network": a function of the drawn row, the class and the evaluation number"""
    c = np.arange(C, dtype=np.float64)
    x = np.sin(0.37 * index[:, :, None].astype(np.float64) + 1.3 * c + 0.61 * q + salt) * (1.0 + 0.01 * q)
    return x.astype(np.float32)


def _reference_loop(padded_gt, num_point, num_classes, draw, run, seg_range=None):
    """evaluate_shapenet.py:219-289 for one batch, literally, with `draw(p)` -> sample indices [bsize, N] in place of
    np.random.choice and `run(q)` -> pred_val in place of sess.run (q counts its calls).  seg_range: per shape (startIdx, endIdx)
    of evaluate_shapenet_onehot.py:285-314, None for the per-category script."""
    bsize = len(padded_gt)
    NUM_POINT, NUM_CLASSES = num_point, num_classes
    batch_gt_label, batch_pred_sum, batch_sample_count, batch_sample_index = [], [], [], []
    batch_point_size = np.zeros((bsize,), np.int32)
    batch_point_covered = np.zeros((bsize,), np.int32)
    for b in range(bsize):
        num = padded_gt[b].shape[0]
        batch_point_size[b] = num
        batch_gt_label.append(padded_gt[b])
        batch_pred_sum.append(np.zeros((num, NUM_CLASSES), dtype=np.float32))
        batch_sample_count.append(np.zeros((num,), dtype=np.int32))
        batch_sample_index.append(np.zeros((num,), dtype=np.int32))
    draws = 0
    while any(batch_point_covered < batch_point_size):
        samples = draw(draws)
        for b in range(bsize):
            sample_index = samples[b]
            batch_sample_count[b][sample_index] += 1
            batch_sample_index[b] = sample_index
            batch_point_covered[b] = np.sum(batch_sample_count[b] > 10)
        for a, augType in enumerate(['none', 'augment']):
            pred_val = run(2 * draws + a)
            for b in range(bsize):
                batch_pred_sum[b][batch_sample_index[b]] += pred_val[b, ...]
        draws += 1
    total_correct, total_seen = 0, 0
    total_seen_class = [0 for _ in range(NUM_CLASSES)]
    total_correct_class = [0 for _ in range(NUM_CLASSES)]
    shape_ious, preds = [], []
    for b in range(bsize):
        startIdx, endIdx = seg_range[b] if seg_range is not None else (0, NUM_CLASSES)
        logits = batch_pred_sum[b][:, startIdx:endIdx]
        pred_label = np.argmax(logits, 1) + startIdx
        preds.append(pred_label)
        correct = np.sum(pred_label == batch_gt_label[b])
        total_correct += correct
        total_seen += batch_point_size[b]
        part_ious = [0.0 for _ in range(endIdx - startIdx)]
        for l in range(startIdx, endIdx):
            union = (pred_label == l) | (batch_gt_label[b] == l)
            intersect = (pred_label == l) & (batch_gt_label[b] == l)
            total_seen_class[l] += np.sum(batch_gt_label[b] == l)
            total_correct_class[l] += np.sum(intersect)
            if np.sum(union) == 0:
                part_ious[l - startIdx] = 1.0
            else:
                part_ious[l - startIdx] = np.sum(intersect) / float(np.sum(union))
        shape_ious.append(np.mean(part_ious))
    return dict(sums=batch_pred_sum, count=batch_sample_count, pred=preds, draws=draws, shape_ious=shape_ious,
                total_correct=total_correct, total_seen=total_seen, total_seen_class=total_seen_class,
                total_correct_class=total_correct_class)


@pytest.mark.parametrize("onehot", [False, True])
def test_the_statement_equals_the_references_loop(onehot):
    sizes, N, seed, batch_index = [40, 7, 64, 65, 1], 64, 9, 3
    C = 50 if onehot else 6
    category = [10, 0, 3, 15, 1] if onehot else None
    blocks, cat = cases.shapes(sizes, 2, C, category)
    label = np.concatenate([b[:, 6] for b in blocks])
    ids = np.arange(len(sizes))
    lo = cases.PART_LO[cat] if onehot else np.zeros(len(sizes), np.int32)
    n = cases.PART_N[cat] if onehot else np.full(len(sizes), C, np.int32)
    fn = lambda q, index: _logits(len(sizes), N, C, q, index)
    got = shapeeval.shape_vote_reference(sizes, label, ids, lo, n, N, seed, batch_index, fn, C)          # min_count = 11: `> 10`
    samples = {}

    def draw(p):
        samples[p] = evalvote.draw_index(sizes, ids, N, seed, evalvote.pass_step(batch_index, p))
        return samples[p]
    want = _reference_loop([b[:, 6] for b in blocks], N, C, draw, lambda q: fn(q, samples[q // 2]),
                           [(int(a), int(a + c)) for a, c in zip(lo, n)] if onehot else None)
    assert got.passes == want["draws"] >= 11 and got.complete
    for k in range(len(sizes)):
        assert got.votes[k].dtype == np.float32 and got.votes[k].tobytes() == want["sums"][k].tobytes()
        assert np.array_equal(got.count[k], 2 * want["count"][k])
        assert np.array_equal(got.pred[k], want["pred"][k])
        assert got.shape_iou[k] == want["shape_ious"][k]                                 # float64, bit for bit
    assert int(got.correct.sum()) == want["total_correct"] and int(got.size.sum()) == want["total_seen"]
    assert got.inter.sum(axis=0).tolist() == [int(x) for x in want["total_correct_class"]]
    assert got.gt_cnt.sum(axis=0).tolist() == [int(x) for x in want["total_seen_class"]]
    if onehot:
        assert (np.concatenate(got.pred) != label).any() and int(got.gt_cnt.sum()) < sum(sizes)      # labels outside the range exist
    # and the figures of the whole evaluation (one batch), as the scripts print them
    res = shapeeval.evaluate_reference(lambda i, q, index: fn(q, index), sizes, label, cat, len(sizes), N, seed, C,
                                       cases.PART_LO if onehot else None, cases.PART_N if onehot else None)
    res3 = shapeeval.shape_vote_reference(sizes, label, ids, lo, n, N, seed, 0, fn, C)
    assert np.array_equal(res.shape_iou, res3.shape_iou) and res.passes == [res3.passes]
    assert res.accuracy == int(res3.correct.sum()) / float(sum(sizes))
    assert res.instance_miou == np.mean(list(res3.shape_iou))
    by_cat = {}
    for k, c in enumerate(cat):
        by_cat.setdefault(int(c), []).append(res3.shape_iou[k])
    assert res.mean_category_miou == np.mean([np.mean(v) for _, v in sorted(by_cat.items())])
    for c, v in by_cat.items():
        assert res.category_miou[c] == np.mean(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        want_acc = np.array(res3.inter.sum(axis=0)) / np.array(res3.gt_cnt.sum(axis=0), dtype=float)
    assert np.array_equal(res.class_acc, want_acc, equal_nan=True)


def _one_shape(votes, gt, lo, n):
    votes = np.asarray(votes, dtype=np.float32)
    pred, inter, pc, gc, correct = shapeeval.part_counts(votes, np.asarray(gt, dtype=np.float32), lo, n)
    return pred, inter, pc, gc, correct, shapeeval.shape_iou(inter, pc, gc, lo, n)


def test_hand_cases():
    # an absent part (no row has it, none is predicted as it) has IoU 1
    pred, inter, pc, gc, correct, iou = _one_shape([[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0]], [0, 1, 1, 1], 0, 3)
    assert pred.tolist() == [0, 1, 0, 1] and inter.tolist() == [1, 2, 0] and pc.tolist() == [2, 2, 0] and gc.tolist() == [1, 3, 0]
    assert correct == 3 and iou == np.mean([1 / 2.0, 2 / 3.0, 1.0])
    # a one-hot table with part_lo > 0: the maximum outside the range does not count; ties take the first part of the range
    votes = [[9, 9, 1, 2, 0, 9], [9, 9, 3, 3, 3, 9], [9, 9, 0, 0, 5, 9]]
    pred, inter, pc, gc, correct, iou = _one_shape(votes, [3, 2, 4], 2, 3)
    assert pred.tolist() == [3, 2, 4] and correct == 3 and iou == 1.0 and inter.tolist() == [0, 0, 1, 1, 1, 0]
    # a ground-truth label outside the range matches no part (it is in no gt_cnt), and cannot be predicted
    pred, inter, pc, gc, correct, iou = _one_shape(votes, [0, 2, 5], 2, 3)
    assert pred.tolist() == [3, 2, 4] and correct == 1 and gc.tolist() == [0, 0, 1, 0, 0, 0] and pc.tolist() == [0, 0, 1, 1, 1, 0]
    assert iou == np.mean([1.0, 0.0, 0.0])
    # NaN logits: a NaN counts as a maximum (np.argmax), the first one
    nan = float("nan")
    pred, *_ = _one_shape([[0, nan, 5], [nan, nan, 1], [1, 2, nan], [1, 3, 2]], [0, 0, 0, 0], 0, 3)
    assert pred.tolist() == [1, 0, 2, 1]
    pred, *_ = _one_shape([[nan, 0, 1, nan]], [1], 1, 2)
    assert pred.tolist() == [2]


def test_a_shape_with_fewer_rows_than_num_point_and_non_finite_sums():
    """n < N: sampled with replacement, the last slot that drew a row votes; NaN sums are counted and predicted"""
    sizes, N, C = [5, 30], 16, 3
    blocks, cat = cases.shapes(sizes, 1, C)
    label = np.concatenate([b[:, 6] for b in blocks])

    def fn(q, index):
        x = _logits(2, N, C, q, index)
        if q == 1:
            x[0, index[0] == 2, 1] = np.inf
        if q == 2:
            x[0, index[0] == 2, 1] = -np.inf
        return x
    got = shapeeval.shape_vote_reference(sizes, label, [0, 1], [0, 0], [C, C], N, 4, 0, fn, C, min_count=2, max_passes=64)
    assert got.complete and got.passes >= 2 and (got.count[0] >= 4).all() and (got.count[0] % 2 == 0).all()
    assert got.size.tolist() == [5, 30] and got.covered.tolist() == [5, 30]
    assert np.isnan(got.votes[0][2, 1]) and got.pred[0][2] == 1 and got.nonfinite_rows == 1
    # replaying by hand: per draw a row of shape 0 gets the logits of the LAST slot that drew it, plain then augmented
    sums = np.zeros((5, C), np.float32)
    for p in range(got.passes):
        index = evalvote.draw_index(sizes, [0, 1], N, 4, evalvote.pass_step(0, p))
        for a in range(2):
            x = fn(2 * p + a, index)
            for r in range(5):
                slots = np.nonzero(index[0] == r)[0]
                if slots.size:
                    sums[r] = sums[r] + x[0, slots[-1]]
    ok = ~np.isnan(sums)
    assert np.array_equal(np.isnan(got.votes[0]), ~ok) and np.array_equal(got.votes[0][ok].view(np.int32), sums[ok].view(np.int32))
    # the cap ends a loop that is not covered, and says so
    short = shapeeval.shape_vote_reference(sizes, label, [0, 1], [0, 0], [C, C], N, 4, 0, fn, C, min_count=2, max_passes=1)
    assert short.passes == 1 and not short.complete
    with pytest.raises(ValueError):
        shapeeval.shape_vote_reference(sizes, label, [0, 1], [0, 2], [C, C], N, 4, 0, fn, C)
    with pytest.raises(ValueError):
        shapeeval.shape_vote_reference(sizes, label, [0, 0], [0, 0], [C, C], N, 4, 0, fn, C)
    with pytest.raises(ValueError):
        shapeeval.shape_vote_reference(sizes, label, [0, 1], [0, 0], [C, C], N, 4, 0, fn, C, max_passes=(1 << 19) + 1)


def test_merged_ranks_equal_one_rank():
    C = 50
    category = [3, 10, 0, 15, 7, 3, 10, 1]
    blocks, cat = cases.shapes(cases.SIZES, 4, C, category)
    label = np.concatenate([b[:, 6] for b in blocks])
    fn = lambda i, q, index: _logits(index.shape[0], cases.NUM_POINT, C, q, index, salt=i)
    args = (fn, cases.SIZES, label, cat, cases.BATCH, cases.NUM_POINT, cases.SEED, C, cases.PART_LO, cases.PART_N, 2, 64)
    one = shapeeval.evaluate_reference(*args, keep_votes=True)
    parts = [shapeeval.evaluate_reference(*args, rank=r, world=3, keep_votes=True) for r in (2, 0, 1)]
    assert [p.batches for p in parts] == [[2], [0], [1]]
    merged = shapeeval.ShapeResult.merge(parts)
    assert one.complete and merged.complete and one.batches == merged.batches == [0, 1, 2] and one.passes == merged.passes
    for name in ("shapes", "category", "shape_iou", "correct", "seen", "class_correct", "class_seen"):
        assert np.array_equal(getattr(one, name), getattr(merged, name)), name
    assert np.array_equal(one.category_miou, merged.category_miou, equal_nan=True)
    assert np.array_equal(one.class_acc, merged.class_acc, equal_nan=True)
    for name in ("mean_category_miou", "instance_miou", "accuracy", "nonfinite_rows", "num_categories"):
        assert getattr(one, name) == getattr(merged, name), name
    assert 0.0 < one.instance_miou < 1.0 and one.shapes.tolist() == list(range(8)) and one.num_categories == 16
    for i in one.batches:
        for x, y in zip(one.votes[i].votes, merged.votes[i].votes):
            assert x.tobytes() == y.tobytes()
    with pytest.raises(ValueError):
        shapeeval.ShapeResult.merge([parts[0], parts[0]])


def test_the_loops_of_the_gpu_test_complete_within_their_caps():
    """coverage depends on the draws alone, so zero logits decide it: every batch tests/test_gpu_shapeeval.py evaluates is
    covered within the max_passes it passes"""
    zero = lambda C: (lambda i, q, index: np.zeros(index.shape + (C,), np.float32))
    for C, table in ((6, (None, None)), (50, (cases.PART_LO, cases.PART_N))):
        label = np.zeros((sum(cases.SIZES),), np.float32)
        res = shapeeval.evaluate_reference(zero(C), cases.SIZES, label, np.zeros(len(cases.SIZES), np.int32), cases.BATCH,
                                           cases.NUM_POINT, cases.SEED, C, *table, cases.MIN_COUNT, cases.MAX_PASSES)
        assert res.complete and res.batches == [0, 1, 2] and max(res.passes) < cases.MAX_PASSES, res.passes
        assert min(res.passes) >= cases.MIN_COUNT
    label = np.zeros((sum(cases.DEFAULT_SIZES),), np.float32)
    res = shapeeval.evaluate_reference(zero(6), cases.DEFAULT_SIZES, label, np.zeros(3, np.int32), cases.BATCH, cases.NUM_POINT,
                                       cases.SEED, 6, max_passes=cases.DEFAULT_MAX_PASSES)
    assert res.complete and 11 <= res.passes[0] < cases.DEFAULT_MAX_PASSES, res.passes
    print("draws per batch:", res.passes)
