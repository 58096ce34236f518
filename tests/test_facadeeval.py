"""harness/facadeeval.py without a GPU: the numpy statement of the facade evaluation — evalvote.vote_reference around
facadefeed.apply_reference with the evaluation's recipe, min_votes = 11 over all rows — and the merge of two ranks' shares."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import evalvote, facadeeval, facadefeed

SIZES = [1, 40, 64, 65, 300]
N, C = 64, 7


def _facades(seed=0, sizes=SIZES):
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        normal = rng.randn(n, 3)
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        xyz = (rng.rand(n, 3) - [0.5, 0.5, 0.0]) * [2.0, 1.0, 1.5]
        out.append(facadefeed.facade_blocks(xyz.astype(np.float32), normal.astype(np.float32),
                                            (rng.rand(n, 3) * 2 - 1).astype(np.float32), rng.randint(0, C, n)))
    return [o[0] for o in out], [o[1] for o in out]


W = np.random.RandomState(9).randn(9, C)


def _logits(i, p, points, label, index):
    """a deterministic function of the pass's points and of (batch, pass)"""
    return (np.dot(points, W) + np.sin(np.arange(C) * 0.37 + 0.61 * (1000 * i + p))).astype(np.float32)


def test_the_statement_votes_until_every_row_has_eleven_and_counts_every_row_once():
    blocks, normals = _facades()
    seen = []

    def fn(i, p, points, label, index):
        if p < 2:
            seen.append((i, p, points.copy(), label.copy(), index.copy()))
        return _logits(i, p, points, label, index)
    res = facadeeval.evaluate_reference(fn, blocks, normals, 2, N, seed=4, keep_votes=True)
    assert res.batches == [0, 1, 2] and res.complete and res.nonfinite_rows == 0
    assert res.confusion.shape == (C, C) and res.confusion.sum() == sum(SIZES)
    rows = np.concatenate(blocks)
    assert np.array_equal(res.confusion.sum(axis=1), np.bincount(rows[:, 6].astype(np.int64), minlength=C))
    for i in res.batches:
        v = res.votes[i]
        ids = evalvote.batch_blocks(len(SIZES), 2, i)
        assert np.array_equal(v.inner_size, np.array(SIZES)[ids]) and np.array_equal(v.covered, v.inner_size)
        assert all(c.min() >= facadeeval.MIN_VOTES for c in v.count) and v.passes >= facadeeval.MIN_VOTES
        # the loop ends with the pass that brought the last row to 11 votes: some row has exactly 11
        assert min(c.min() for c in v.count) == facadeeval.MIN_VOTES
    m = evalvote.metrics(res.confusion)
    assert res.miou == m.miou and res.overall_acc == m.overall_acc and len(res.class_iou) == C
    # what the network is shown: the pass's sample turned and tilted, normals included; rgb and labels copied
    assert len(seen) == 6
    for i, p, points, label, index in seen:
        ids = evalvote.batch_blocks(len(SIZES), 2, i)
        ref = facadefeed.assemble_reference(SIZES, ids, N, 4, evalvote.pass_step(i, p), facadefeed.EVAL_AUGMENT)
        want, want_label = facadefeed.apply_reference(blocks, normals, ids, ref)
        assert np.array_equal(index, ref.index) and np.array_equal(points, want) and np.array_equal(label, want_label)
        for k, b in enumerate(ids):
            assert np.array_equal(points[k, :, 6:9], blocks[b][index[k], 3:6])
            assert not np.array_equal(points[k, :, 3:6], normals[b][index[k], 0:3])
    # without augmentation the plain draw
    plain = []
    facadeeval.evaluate_reference(lambda i, p, pts, l, idx: (plain.append((i, p, pts, idx)), _logits(i, p, pts, l, idx))[1],
                                  blocks, normals, 5, N, seed=4, augment=False, max_passes=2)
    i, p, pts, idx = plain[1]
    for k in range(5):
        want = np.concatenate((blocks[k][idx[k], 0:3], normals[k][idx[k], 0:3], blocks[k][idx[k], 3:6]), axis=1)
        assert np.array_equal(pts[k], want.astype(np.float64))


def test_max_passes_ends_an_uncovered_batch_and_says_so():
    blocks, normals = _facades()
    res = facadeeval.evaluate_reference(_logits, blocks, normals, 5, N, seed=1, max_passes=5)
    assert res.passes == [5] and not res.complete
    with pytest.raises(ValueError):
        facadeeval.evaluate_reference(_logits, blocks, normals, 5, N, seed=1, min_votes=0)


def test_merged_ranks_equal_one_rank():
    blocks, normals = _facades(3)
    one = facadeeval.evaluate_reference(_logits, blocks, normals, 2, N, seed=7, keep_votes=True)
    parts = [facadeeval.evaluate_reference(_logits, blocks, normals, 2, N, seed=7, rank=r, world=2, keep_votes=True) for r in (1, 0)]
    assert parts[0].batches == [1] and parts[1].batches == [0, 2]
    merged = evalvote.EvalResult.merge(parts)
    assert merged.batches == one.batches and merged.passes == one.passes and merged.complete == one.complete
    assert np.array_equal(merged.confusion, one.confusion) and merged.miou == one.miou and merged.overall_acc == one.overall_acc
    assert np.array_equal(merged.class_iou, one.class_iou) and merged.nonfinite_rows == one.nonfinite_rows
    for i in one.batches:
        for x, y in zip(one.votes[i].votes + one.votes[i].count + one.votes[i].pred,
                        merged.votes[i].votes + merged.votes[i].count + merged.votes[i].pred):
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(one.votes[i].covered, merged.votes[i].covered)
