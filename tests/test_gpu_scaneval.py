"""harness/scannet.py's three-view evaluation on the device against its numpy statement (scannet.scan_vote_reference /
evaluate_reference / evaluate_scenes_reference): fp32 vote sums as bit patterns, counts (multiples of 3), predictions, passes,
coverage and confusion all EQUAL.  The "network" is tests/_scannet_cases.py's toy — small-integer logits of (pool row, view, class),
computed on the device from the row number the pool carries in its first colour channel and in numpy from the index — so both
sides compute the logits themselves; tests/test_scannet.py asserts without a GPU that these loops complete within the caps used
here.  Every launch here is an ordinary one."""
import numpy as np
import pytest

import _scannet_cases as cases
from sph3d_gcn_amd.harness import evalvote, feed, scannet, scenemerge

pytestmark = pytest.mark.gpu

C, N = cases.C, cases.NUM_POINT


class _Toy:
    """cases.toy_logits on the device: the pool row from the first colour channel (copied into every view), the view from the
    number of the call — three calls per draw, in view order"""

    def __init__(self):
        self.calls = 0

    def __call__(self, points, label, inner):
        import torch
        view = self.calls % 3
        self.calls += 1
        row = points[:, :, 3].long().unsqueeze(-1)
        c = torch.arange(C, device=points.device, dtype=torch.int64)
        return (((row * 7 + view * 13 + c * 5) % 11) - 5).float()


class _Hook:
    """on_pass: the pass numbers are 3 p + v in order, and the device logits are the statement's"""

    def __init__(self, fn):
        self.fn, self.seen = fn, {}

    def __call__(self, batch_index, q, index, logits):
        assert q == self.seen.get(batch_index, 0)
        self.seen[batch_index] = q + 1
        assert np.array_equal(logits.cpu().numpy(), self.fn(batch_index, q, index.cpu().numpy()))


def _same_votes(got, want):
    assert got.passes == want.passes and got.complete == want.complete
    assert np.array_equal(got.covered, want.covered) and np.array_equal(got.inner_size, want.inner_size)
    assert len(got.votes) == len(want.votes)
    for k in range(len(want.votes)):
        assert np.array_equal(got.count[k], want.count[k]) and (got.count[k] % 3 == 0).all(), k
        assert np.array_equal(got.votes[k].view(np.int32), want.votes[k].view(np.int32)), k
        assert np.array_equal(got.pred[k], want.pred[k]), k


def _same_result(got, want):
    assert got.batches == want.batches and got.passes == want.passes and got.complete == want.complete
    assert np.array_equal(got.confusion, want.confusion) and got.nonfinite_rows == want.nonfinite_rows
    for c, s, c2, s2 in zip(got.covered, got.inner_size, want.covered, want.inner_size):
        assert np.array_equal(c, c2) and np.array_equal(s, s2)


@pytest.fixture(scope="module")
def pool(dev):
    blocks = cases.blocks()
    rows = np.concatenate(blocks)
    p = feed.BlockPool(blocks, dev)
    return blocks, rows[:, 6].copy(), rows[:, 7].copy(), p, cases.logits_fn(p.host_offsets, cases.pool_batch_ids)


def test_evaluate_equals_the_numpy_statement_bit_for_bit(pool, dev):
    """blocks of 20 .. 300 rows, N = 64, batches of 4 (the last one has 2 blocks), 21 classes"""
    blocks, label, inner, p, fn = pool
    hook = _Hook(fn)
    res = scannet.evaluate(_Toy(), p, cases.BATCH, N, cases.SEED, max_passes=cases.MAX_PASSES, keep_votes=True, on_pass=hook)
    want = scannet.evaluate_reference(fn, cases.SIZES, label, inner, cases.BATCH, N, cases.SEED, C, max_passes=cases.MAX_PASSES,
                                      keep_votes=True)
    print("draws per batch %s" % (res.passes,))
    assert want.complete and want.batches == [0, 1] and all(p_ < cases.MAX_PASSES for p_ in want.passes)
    _same_result(res, want)
    for i in want.batches:
        assert hook.seen[i] == 3 * want.passes[i]
        _same_votes(res.votes[i], want.votes[i])
        for k in range(len(want.votes[i].votes)):
            assert (res.votes[i].count[k][blocks[cases.BATCH * i + k][:, 7] == 1] >= 6).all()
    assert len(res.votes[1].votes) == 2 and res.confusion.sum() == int(inner.sum())
    m, w = scannet.scannet_metrics(res.confusion), scannet.scannet_metrics(want.confusion)
    assert m.miou == w.miou and m.overall_acc == w.overall_acc and 0.0 <= m.miou <= 1.0


def test_run_batch_with_an_empty_id_and_merged_ranks(pool, dev):
    blocks, label, inner, p, fn = pool
    voter = scannet.ScanNetVoter(p, cases.BATCH, N, C, sum(cases.SIZES))
    assert voter.min_votes == 6 and voter.V == 3
    i = cases.EMPTY_BATCH_INDEX
    got = voter.run_batch(_Toy(), np.array(cases.EMPTY_IDS, np.int32), cases.SEED, i, cases.MAX_PASSES, keep_votes=True,
                          on_pass=_Hook(fn))
    want = scannet.scan_vote_reference(cases.SIZES, label, inner, cases.EMPTY_IDS, N, cases.SEED, i, lambda q, index: fn(i, q, index), C,
                                       max_passes=cases.MAX_PASSES)
    assert want.complete and want.passes < cases.MAX_PASSES and want.inner_size[1] == 0 and got.votes[1].shape == (0, C)
    _same_votes(got, want)
    confusion, _nonfinite = voter.totals()
    assert np.array_equal(confusion, want.confusion)
    # a cap that ends the batch early: the count is still a multiple of 3
    capped = voter.run_batch(_Toy(), np.array([2], np.int32), cases.SEED, 1, 2, keep_votes=True)
    assert capped.passes == 2 and not capped.complete and (capped.count[0] % 3 == 0).all() and capped.count[0].max() == 6
    with pytest.raises(ValueError):
        voter.run_batch(_Toy(), np.array([2], np.int32), cases.SEED, 1, (1 << 20) // 3 + 1)
    # world 2, merged
    run = lambda rank, world: scannet.evaluate(_Toy(), p, cases.BATCH, N, cases.SEED, max_passes=cases.MAX_PASSES, rank=rank, world=world)
    _same_result(evalvote.EvalResult.merge([run(1, 2), run(0, 2)]), run(0, 1))


class _SignToy:
    """logits that depend on the xyz the model is handed: class 1 + (sign of a fixed projection) gets a vote of 2, and it keeps
    the points of its first calls"""

    def __init__(self, keep):
        self.keep, self.kept = keep, []

    def __call__(self, points, label, inner):
        import torch
        if len(self.kept) < self.keep:
            self.kept.append(points.clone())
        side = (points[:, :, 0] * 0.6 - points[:, :, 1] * 0.3 + points[:, :, 2] * 0.74 > 0.8).long() + 1
        return torch.nn.functional.one_hot(side, C).float() * 2.0


class _Recorder:
    def __init__(self):
        self.logits = {}

    def __call__(self, batch_index, q, index, logits):
        self.logits.setdefault(batch_index, []).append(logits.cpu().numpy())


def test_the_three_views_reach_the_model_in_order(pool, dev):
    """a model that looks at xyz sees, per draw, the plain sample, then augment_fn1 of it, then augment_fn2 of THAT: its first six
    inputs are scannet.assemble's views at the draws' steps, and its votes replay through the statement"""
    import torch
    blocks, label, inner, p, _fn = pool
    ids, bi = np.array(cases.VIEW_IDS, dtype=np.int32), cases.VIEW_BATCH_INDEX
    voter = scannet.ScanNetVoter(p, cases.BATCH, N, C, sum(cases.SIZES))
    toy, rec = _SignToy(6), _Recorder()
    got = voter.run_batch(toy, ids, cases.SEED, bi, cases.MAX_PASSES, keep_votes=True, on_pass=rec)
    ids_dev = torch.from_numpy(ids).to(dev)
    recipes = scannet.eval_recipes(scannet.EVAL_VIEWS, 3)
    for draw in range(2):
        views, _l, _i, index = scannet.assemble(p.rows, p.offsets, ids_dev, N, cases.SEED, evalvote.pass_step(bi, draw), recipes,
                                                want_index=True)
        for v in range(3):
            assert torch.equal(toy.kept[3 * draw + v].view(torch.int32), views[v].view(torch.int32)), (draw, v)
        rows = p.rows[(p.offsets[ids_dev.long()].reshape(-1, 1) + index.long())]
        assert torch.equal(views[0].view(torch.int32), rows[:, :, 0:6].contiguous().view(torch.int32))
        assert not torch.equal(views[1][:, :, 0:3], views[0][:, :, 0:3]) and not torch.equal(views[2][:, :, 0:3], views[1][:, :, 0:3])
        # view 2 is built on view 1, not on the plain sample: it is (all five transforms of) view 1 within the bound
        ref = scannet.assemble_reference(p.sizes, ids, N, cases.SEED, evalvote.pass_step(bi, draw), recipes)
        step = scannet.apply_reference(blocks, ids, ref, base=views.cpu().numpy())[0]
        assert np.allclose(views[2, :, :, 0:3].cpu().numpy(), step[2, :, :, 0:3], rtol=1e-5, atol=1e-5)
    want = scannet.scan_vote_reference(cases.SIZES, label, inner, ids, N, cases.SEED, bi, lambda q, index: rec.logits[bi][q], C,
                                       max_passes=cases.MAX_PASSES)
    assert want.complete and len(rec.logits[bi]) == 3 * want.passes
    _same_votes(got, want)
    # the views differ enough for the model to answer differently
    assert any(not np.array_equal(rec.logits[bi][0], rec.logits[bi][v]) for v in (1, 2))


def test_evaluate_scenes_on_the_three_view_votes(dev, tmp_path):
    """two tiny scenes: scannet.evaluate_scenes equals scenemerge.evaluate_scenes_reference fed with the three-view votes;
    pred_full goes through LABELID_SET; write_predictions round-trips"""
    blocks, index, sob, scenes = cases.scenes()
    p = feed.BlockPool(blocks, dev, index, sob)
    rows = np.concatenate(blocks)
    table = cases.scene_batch_ids(sob)
    fn = cases.logits_fn(p.host_offsets, lambda i: table[i])
    hook = _Hook(fn)
    res = scannet.evaluate_scenes(_Toy(), p, scenes, cases.SCENE_BATCH, N, cases.SCENE_SEED, max_passes=cases.MAX_PASSES,
                                  keep_pred=True, on_pass=hook)
    want = scannet.evaluate_scenes_reference(fn, [len(b) for b in blocks], rows[:, 6], rows[:, 7], np.concatenate(index), sob, scenes,
                                             cases.SCENE_BATCH, N, cases.SCENE_SEED, C, max_passes=cases.MAX_PASSES, keep_pred=True)
    assert all(want.complete) and res.scenes == want.scenes == [0, 1] and res.complete == want.complete
    assert res.unseen_rows == want.unseen_rows and res.skipped_rows == want.skipped_rows and res.out_of_scene == want.out_of_scene
    assert np.array_equal(res.confusion_full, want.confusion_full) and np.array_equal(res.confusion_voxel, want.confusion_voxel)
    assert np.array_equal(res.block.confusion, want.block.confusion) and res.block.passes == want.block.passes
    assert res.block.batches == want.block.batches == sorted(table) and all(hook.seen[i] == 3 * q for i, q in zip(res.block.batches, res.block.passes))
    lut = np.asarray(scannet.LABELID_SET, dtype=np.int32)
    for s in want.scenes:
        for key in ("merged", "hits", "pred_voxel", "pred_full", "idx"):
            a, b = res.pred[s][key], want.pred[s][key]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (s, key)
        assert np.array_equal(res.pred[s]["pred_full"], lut[res.pred[s]["pred_voxel"][res.pred[s]["idx"]]])
        assert set(res.pred[s]["pred_full"].tolist()) <= set(scannet.LABELID_SET)
    assert res.confusion_full.sum() == sum(len(s.full_xyz) for s in scenes)
    names = ["scene%04d_00" % s for s in range(2)]
    paths = scannet.write_predictions(str(tmp_path), names, res)
    assert len(paths) == 2
    for s, path in enumerate(paths):
        assert np.array_equal(scannet.read_predictions(path), res.pred[s]["pred_full"])
    m = scannet.scannet_metrics(res.confusion_full)
    assert 0.0 <= m.miou <= 1.0 and m.miou == scannet.scannet_metrics(want.confusion_full).miou


def test_scenemerge_without_a_voter_factory_is_unchanged(dev):
    """scenemerge.evaluate_scenes with its default equals the same call with an explicit evalvote.Voter factory: the keyword only
    names the voter it constructed before"""
    blocks, index, sob, scenes = cases.scenes()
    p = feed.BlockPool(blocks, dev, index, sob)
    made = []

    def factory(*a):
        made.append(a)
        return evalvote.Voter(*a)
    run = lambda **kw: scenemerge.evaluate_scenes(_Toy(), p, scenes, cases.SCENE_BATCH, N, cases.SCENE_SEED, C, min_votes=2,
                                                  max_passes=cases.MAX_PASSES, keep_pred=True, **kw)
    a, b = run(), run(voter_factory=factory)
    assert len(made) == 1 and made[0][0] is p and made[0][1:4] == (cases.SCENE_BATCH, N, C) and made[0][5] == 2
    assert a.scenes == b.scenes and a.complete == b.complete and all(a.complete)
    assert np.array_equal(a.confusion_full, b.confusion_full) and np.array_equal(a.confusion_voxel, b.confusion_voxel)
    assert np.array_equal(a.block.confusion, b.block.confusion) and a.block.passes == b.block.passes
    for s in a.scenes:
        for key in ("merged", "hits", "pred_voxel", "pred_full", "idx"):
            assert a.pred[s][key].tobytes() == b.pred[s][key].tobytes(), (s, key)
