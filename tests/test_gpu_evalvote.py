"""csrc/vote.hip and harness/evalvote.py on the device against the numpy statement (evalvote.vote_reference): the logits of every
pass are recorded through `on_pass` and replayed through the statement, so counts, coverage, passes, predictions and the
confusion matrix must be equal and the fp32 vote sums equal as bit patterns — every row sees the same fp32 adds in the same
order.  Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import evalvote, feed

pytestmark = pytest.mark.gpu

SIZES = {1024: [1500, 1024, 900, 2000, 3000, 1100, 5000, 700, 1, 2, 3, 1023, 1025, 64, 2500, 1800],
         8192: [8192, 8193, 12000, 20000, 30000, 500, 9000, 8191, 1, 2, 3, 6000, 16384, 700, 10000, 4096]}


def _blocks(seed, sizes, num_cls=13, extent=(2.1, 2.1, 3.0)):
    """blockio.parse_block-shaped blocks: xyz in an S3DIS-like slab, rgb in [0, 1], label 0..num_cls-1, inner 0/1"""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        b = np.empty((n, 8), dtype=np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array(extent)
        b[:, 3:6] = rng.rand(n, 3)
        b[:, 6] = rng.randint(0, num_cls, n)
        b[:, 7] = rng.randint(0, 2, n)
        out.append(b)
    return out


def _columns(blocks):
    rows = np.concatenate(blocks, axis=0)
    return rows[:, 6].copy(), rows[:, 7].copy()


class _Toy:
    """a cheap deterministic "network": a fixed [6, C] matrix on the points plus a term that differs from pass to pass"""

    def __init__(self, C, dev, seed=0):
        import torch
        self.w = torch.from_numpy(np.random.RandomState(seed).randn(6, C).astype(np.float32)).to(dev)
        self.calls = 0

    def __call__(self, points, label, inner):
        import torch
        self.calls += 1
        phase = torch.arange(self.w.shape[1], device=points.device, dtype=torch.float32) * 0.37 + 0.61 * self.calls
        return (points.unsqueeze(-1) * self.w).sum(dim=2) + torch.sin(phase) * (1.0 + points[:, :, 0:1])


class _Recorder:
    def __init__(self):
        self.index, self.logits = {}, {}

    def __call__(self, batch_index, p, index, logits):
        assert p == len(self.index.setdefault(batch_index, []))
        self.index[batch_index].append(index.cpu().numpy())
        self.logits.setdefault(batch_index, []).append(logits.cpu().numpy())


def _replay_and_compare(got, rec, batch_index, sizes, label, inner, ids, N, seed, C, min_votes, max_passes=evalvote.MAX_PASSES):
    """got: BatchVotes of the device (host arrays) -> the statement's BatchVotes, after asserting they are equal"""
    index, logits = rec.index.get(batch_index, []), rec.logits.get(batch_index, [])

    def fn(p, idx):
        assert np.array_equal(idx, index[p])                      # (the feed's own guarantee)
        return logits[p]
    want = evalvote.vote_reference(sizes, label, inner, ids, N, seed, batch_index, fn, C, min_votes, max_passes)
    assert got.passes == want.passes == len(index)
    assert np.array_equal(got.covered, want.covered) and np.array_equal(got.inner_size, want.inner_size)
    assert got.complete == want.complete
    for k in range(len(ids)):
        assert np.array_equal(got.count[k], want.count[k]), k
        # bit patterns; a NaN only has to be a NaN in both (IEEE 754 leaves the sign and payload of a generated NaN to the machine)
        nan = np.isnan(want.votes[k])
        assert np.array_equal(np.isnan(got.votes[k]), nan), k
        assert np.array_equal(got.votes[k].view(np.int32)[~nan], want.votes[k].view(np.int32)[~nan]), k
        assert np.array_equal(got.pred[k], want.pred[k]), k
    assert got.nonfinite_rows == want.nonfinite_rows
    return want


@pytest.mark.parametrize("min_votes", [1, 2])
@pytest.mark.parametrize("C", [13, 21])
@pytest.mark.parametrize("b", [16, 7])
@pytest.mark.parametrize("N", [1024, 8192])
def test_kernels_equal_the_numpy_statement_bit_for_bit(dev, N, b, C, min_votes):
    sizes, seed = SIZES[N], 3
    assert {1, 2, 3, N - 1, N, N + 1} <= set(sizes)
    blocks = _blocks(N + C, sizes, C)
    label, inner = _columns(blocks)
    pool = feed.BlockPool.from_blocks(blocks, dev)
    rec = _Recorder()
    res = evalvote.evaluate(_Toy(C, dev), pool, b, N, seed, num_cls=C, min_votes=min_votes, keep_votes=True, on_pass=rec)
    per = feed.batches_per_epoch(len(sizes), b)
    assert res.batches == list(range(per)) and res.complete
    confusion = np.zeros((C, C), np.int64)
    for i in range(per):
        ids = evalvote.batch_blocks(len(sizes), b, i)
        want = _replay_and_compare(res.votes[i], rec, i, sizes, label, inner, ids, N, seed, C, min_votes)
        assert want.complete and res.passes[i] == want.passes
        confusion += want.confusion
    print("N=%d b=%d C=%d min_votes=%d: passes per batch %s" % (N, b, C, min_votes, res.passes))
    assert np.array_equal(res.confusion, confusion) and res.confusion.sum() == int((inner == 1).sum())
    assert res.nonfinite_rows == 0
    m = evalvote.metrics(confusion)
    assert res.miou == m.miou and res.overall_acc == m.overall_acc and np.array_equal(res.class_iou, m.class_iou)
    assert np.array_equal(res.class_acc, m.class_acc)


def test_ties_take_the_first_class_and_non_finite_rows_are_counted(dev):
    """constant logits [0, 1, 1, 0.5]: classes 1 and 2 tie in every sum and 1 wins.  Block 0 has exactly N rows, so all of its
    rows are drawn in every pass: rows 5, 6, 7 get +inf in pass 0 and -inf in pass 1 on class 3 (inf - inf: NaN, which np.argmax
    takes as the maximum), row 9 gets +inf on class 0 in pass 0 only.  Those four rows are the non-finite ones."""
    import torch
    N, C, seed = 256, 4, 11
    sizes = [256, 2000, 100]
    blocks = _blocks(1, sizes, C)
    label, inner = _columns(blocks)
    pool = feed.BlockPool.from_blocks(blocks, dev)
    base = torch.tensor([0.0, 1.0, 1.0, 0.5], device=dev)
    rec = _Recorder()

    def hook(i, p, index, logits):
        if p < 2:
            nan_rows = (index[0] >= 5) & (index[0] <= 7)
            logits[0, nan_rows, 3] = float("inf") if p == 0 else float("-inf")
        if p == 0:
            logits[0, index[0] == 9, 0] = float("inf")
        rec(i, p, index, logits)
    voter = evalvote.Voter(pool, 3, N, C, sum(sizes))
    got = voter.run_batch(lambda p, l, i: base.expand(p.shape[0], N, C).contiguous(), [0, 1, 2], seed, 0, keep_votes=True, on_pass=hook)
    assert got.passes >= 2 and got.complete
    want = _replay_and_compare(got, rec, 0, sizes, label, inner, [0, 1, 2], N, seed, C, 1)
    assert got.nonfinite_rows == 4
    assert np.isnan(got.votes[0][5:8, 3]).all() and got.pred[0][5:8].tolist() == [3, 3, 3]
    assert np.isposinf(got.votes[0][9, 0]) and got.pred[0][9] == 0
    others = np.ones(256, bool)
    others[[5, 6, 7, 9]] = False
    assert (got.pred[0][others] == 1).all() and np.isfinite(got.votes[0][others]).all()
    for k in (1, 2):
        drawn = got.count[k] > 0
        assert (got.pred[k][drawn] == 1).all() and (got.pred[k][~drawn] == 0).all()
        assert np.array_equal(got.votes[k][:, 1], got.votes[k][:, 2])
    confusion, nonfinite = voter.totals()
    assert np.array_equal(confusion, want.confusion) and nonfinite == 4


def test_block_ids_outside_the_pool_vote_nothing_and_do_not_hang_the_loop(dev):
    N, C, seed = 512, 13, 2
    sizes = [700, 300, 5000, 512, 900]
    blocks = _blocks(4, sizes, C)
    label, inner = _columns(blocks)
    pool = feed.BlockPool.from_blocks(blocks, dev)
    voter = evalvote.Voter(pool, 4, N, C, sum(sizes))
    rec = _Recorder()
    ids = [0, -1, len(sizes), 3]
    got = voter.run_batch(_Toy(C, dev), ids, seed, 5, keep_votes=True, on_pass=rec)
    assert 0 < got.passes < 64 and got.complete
    assert got.inner_size[1] == got.inner_size[2] == 0 and got.votes[1].shape == (0, C) and got.votes[2].shape == (0, C)
    for index in rec.index[5]:
        assert (index[1] == -1).all() and (index[2] == -1).all()
    want = _replay_and_compare(got, rec, 5, sizes, label, inner, ids, N, seed, C, 1)
    confusion, _ = voter.totals()
    inner_rows = int((blocks[0][:, 7] == 1).sum() + (blocks[3][:, 7] == 1).sum())
    assert np.array_equal(confusion, want.confusion) and confusion.sum() == inner_rows
    # blocks 1 and 2 lie between the batch's blocks in the pool: their rows got no vote
    assert not voter.votes[sizes[0]:sizes[0] + sizes[1] + sizes[2]].any() and not voter.count[sizes[0]:sum(sizes[:3])].any()
    # a batch with no block of the pool needs no pass; max_passes ends a batch early and says so
    none = voter.run_batch(_Toy(C, dev), [-1, len(sizes)], seed, 6, keep_votes=True)
    assert none.passes == 0 and none.complete
    rec2 = _Recorder()
    short = voter.run_batch(_Toy(C, dev), [2, 3], seed, 7, max_passes=2, keep_votes=True, on_pass=rec2)
    assert short.passes == 2 and not short.complete and short.covered[0] < short.inner_size[0]
    _replay_and_compare(short, rec2, 7, sizes, label, inner, [2, 3], N, seed, C, 1, max_passes=2)
    with pytest.raises(ValueError):
        voter.run_batch(_Toy(C, dev), [1, 1], seed, 8)


def test_two_runs_give_identical_bytes_and_merged_ranks_equal_one_rank(dev):
    N, C, seed = 1024, 13, 9
    sizes = SIZES[1024]
    pool = feed.BlockPool.from_blocks(_blocks(6, sizes, C), dev)
    def run(rank, world):
        import torch
        toy = _Toy(C, dev)

        def fn(points, label, inner):
            toy.calls = 0                      # the same function of the points in every call ...
            return toy(points, label, inner)

        def hook(i, p, index, logits):         # ... and a term from (batch, pass), which a rank's share sees as one rank does
            logits.add_(torch.cos(torch.arange(C, device=dev, dtype=torch.float32) * 0.37 + 0.61 * (1000 * i + p)))
        return evalvote.evaluate(fn, pool, 3, N, seed, rank=rank, world=world, keep_votes=True, on_pass=hook)
    a, b = run(0, 1), run(0, 1)
    assert a.passes == b.passes and np.array_equal(a.confusion, b.confusion)
    for i in a.batches:
        for x, y in zip(a.votes[i].votes + a.votes[i].count + a.votes[i].pred, b.votes[i].votes + b.votes[i].count + b.votes[i].pred):
            assert x.tobytes() == y.tobytes()
    assert a.batches == list(range(6)) and a.complete
    merged = evalvote.EvalResult.merge([run(1, 2), run(0, 2)])
    assert merged.batches == a.batches and merged.passes == a.passes and np.array_equal(merged.confusion, a.confusion)
    assert merged.miou == a.miou and merged.overall_acc == a.overall_acc and merged.complete
    for i in a.batches:
        for x, y in zip(a.votes[i].votes, merged.votes[i].votes):
            assert x.tobytes() == y.tobytes()


def test_the_real_network_is_evaluated(dev):
    """SPH3DS3DIS (reduced plan) in inference mode on a 12-block pool: the evaluation completes, counts every inner row once,
    gives metrics in [0, 1], and the replay of the logits that were voted matches exactly"""
    import torch
    from sph3d_gcn_amd.harness import s3dis_net
    N, seed, C = 1024, 21, 13
    sizes = [1500, 1024, 900, 2000, 3000, 1100, 5000, 1300, 700, 2500, 1800, 1024]
    blocks = _blocks(3, sizes, C, extent=(1.0, 1.0, 1.5))
    label, inner = _columns(blocks)
    pool = feed.BlockPool.from_blocks(blocks, dev)
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N), device=dev, seed=3)
    rec = _Recorder()
    res = evalvote.evaluate(lambda p, l, i: model(p, is_training=False)[0], pool, 4, N, seed, keep_votes=True, on_pass=rec)
    torch.cuda.synchronize()
    print("passes %s miou %.4f overall %.4f" % (res.passes, res.miou, res.overall_acc))
    assert res.complete and res.batches == [0, 1, 2] and all(p > 1 for p in res.passes)
    assert res.confusion.sum() == int((inner == 1).sum()) and res.nonfinite_rows == 0
    for v in [res.miou, res.overall_acc, res.mean_class_acc] + list(res.class_iou) + list(res.class_acc):
        assert np.isfinite(v) and 0.0 <= v <= 1.0
    confusion = np.zeros((C, C), np.int64)
    for i in range(3):
        confusion += _replay_and_compare(res.votes[i], rec, i, sizes, label, inner, evalvote.batch_blocks(12, 4, i), N, seed, C, 1).confusion
    assert np.array_equal(res.confusion, confusion)
