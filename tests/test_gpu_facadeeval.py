"""harness/facadeeval.py on the device against the numpy statement (evalvote.vote_reference): the logits of every pass are
recorded through `on_pass` and replayed through the statement, so counts, coverage, passes, predictions and the confusion matrix
must be equal and the fp32 vote sums equal as bit patterns; and what the network is shown in pass p is the kernel's batch of that
step with the evaluation's recipe, byte for byte.  Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import evalvote, facadeeval, facadefeed
from test_facadeeval import C, N, SIZES, _facades
from test_gpu_evalvote import _Recorder, _replay_and_compare

pytestmark = pytest.mark.gpu


class _Toy:
    """a cheap deterministic "network": a fixed [9, C] matrix on the points plus a term that differs from pass to pass; it keeps
    a copy of the points of its first `keep` calls"""

    def __init__(self, dev, keep=0, seed=0):
        import torch
        self.w = torch.from_numpy(np.random.RandomState(seed).randn(9, C).astype(np.float32)).to(dev)
        self.calls, self.keep, self.kept = 0, keep, []

    def __call__(self, points, label):
        import torch
        if self.calls < self.keep:
            self.kept.append((points.clone(), label.clone()))
        self.calls += 1
        phase = torch.arange(C, device=points.device, dtype=torch.float32) * 0.37 + 0.61 * self.calls
        return (points.unsqueeze(-1) * self.w).sum(dim=2) + torch.sin(phase) * (1.0 + points[:, :, 0:1])


@pytest.fixture(scope="module")
def pool(dev):
    blocks, normals = _facades()
    rows = np.concatenate(blocks)
    return blocks, rows[:, 6].copy(), rows[:, 7].copy(), facadefeed.FacadePool(blocks, normals, device=dev)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_vote_loop_equals_the_numpy_statement_bit_for_bit(pool, dev, seed):
    """one batch of all five facades at batch_index 3, min_votes = 11: the statement needs 93-105 passes for these seeds and
    ends complete, so the loop's cap is not in play"""
    import torch
    blocks, label, inner, p = pool
    assert (inner == 1).all()
    voter = facadeeval.FacadeVoter(p, len(SIZES), N, C, sum(SIZES))
    assert voter.min_votes == 11 and voter.out[0].shape == (len(SIZES), N, 9)
    rec, toy = _Recorder(), _Toy(dev, keep=3)
    ids = np.arange(len(SIZES), dtype=np.int32)
    got = voter.run_batch(toy, ids, seed, 3, keep_votes=True, on_pass=rec)
    want = _replay_and_compare(got, rec, 3, SIZES, label, inner, ids, N, seed, C, 11)
    print("seed %d: %d passes" % (seed, got.passes))
    assert got.complete and want.complete and 93 <= got.passes <= 105 and toy.calls == got.passes
    assert np.array_equal(got.inner_size, np.array(SIZES)) and all(c.min() >= 11 for c in got.count)
    confusion, nonfinite = voter.totals()
    assert np.array_equal(confusion, want.confusion) and confusion.sum() == sum(SIZES) and nonfinite == 0
    # what the network was shown in passes 0..2: the kernel's batch of that step with EVAL_AUGMENT, byte for byte
    ids_dev = torch.from_numpy(ids).to(dev)
    for q, (pts, lab) in enumerate(toy.kept):
        step = evalvote.pass_step(3, q)
        w = facadefeed.assemble(p.rows, p.normals, p.offsets, ids_dev, N, seed, step, facadefeed.EVAL_AUGMENT, want_index=True)
        assert torch.equal(pts.view(torch.int32), w[0].view(torch.int32)) and torch.equal(lab, w[1])
        assert np.array_equal(w[2].cpu().numpy(), rec.index[3][q])
        plain = facadefeed.assemble(p.rows, p.normals, p.offsets, ids_dev, N, seed, step, 0)
        assert not torch.equal(pts[:, :, 0:6], plain[0][:, :, 0:6]) and torch.equal(pts[:, :, 6:9], plain[0][:, :, 6:9])


def test_evaluate_over_batches_without_augmentation_and_with_a_cap(pool, dev):
    import torch
    blocks, label, inner, p = pool
    seed = 5
    rec, toy = _Recorder(), _Toy(dev)
    res = facadeeval.evaluate(toy, p, 2, N, seed, keep_votes=True, on_pass=rec)
    assert res.batches == [0, 1, 2] and res.complete and res.nonfinite_rows == 0
    confusion = np.zeros((C, C), np.int64)
    for i in res.batches:
        ids = evalvote.batch_blocks(len(SIZES), 2, i)
        confusion += _replay_and_compare(res.votes[i], rec, i, SIZES, label, inner, ids, N, seed, C, 11).confusion
    assert np.array_equal(res.confusion, confusion) and res.confusion.sum() == sum(SIZES)
    m = evalvote.metrics(confusion)
    assert res.miou == m.miou and res.overall_acc == m.overall_acc and np.array_equal(res.class_iou, m.class_iou)
    print("passes per batch %s" % res.passes)
    # augment=False: the plain draw, byte for byte
    toy = _Toy(dev, keep=2)
    short = facadeeval.evaluate(toy, p, 5, N, seed, augment=False, max_passes=5)
    assert short.passes == [5] and not short.complete and toy.calls == 5
    ids_dev = torch.arange(len(SIZES), dtype=torch.int32, device=dev)
    for q, (pts, lab) in enumerate(toy.kept):
        w = facadefeed.assemble(p.rows, p.normals, p.offsets, ids_dev, N, seed, evalvote.pass_step(0, q), 0)
        assert torch.equal(pts.view(torch.int32), w[0].view(torch.int32)) and torch.equal(lab, w[1])
    # the cap with augmentation as well
    capped = facadeeval.evaluate(_Toy(dev), p, 5, N, seed, max_passes=5)
    assert capped.passes == [5] and capped.complete is False
