"""The RueMonge2014 facade evaluation with the votes kept on the device: what
ruemonge2014_seg/evaluate_ruemonge2014.py:180-305 does with numpy on the host, on a pool of facade splits
(harness/facadefeed.py:FacadePool).

It is the S3DIS vote loop (harness/evalvote.py: the logits of every pass are summed per row under numpy's last-of-duplicates
rule, the first maximum of the sums is the row's prediction, the confusion matrix gives the S3DIS metrics over the 7 classes)
with two differences:
  * every pass is AUGMENTED: the sample is turned about z and tilted, normals included (facadefeed.EVAL_AUGMENT), at
    step = evalvote.pass_step(batch_index, pass) — the sample itself does not depend on the recipe;
  * passes continue until every row has `count > 10`: min_votes = 11 over all rows (a facade has no outer rows: column 7 of the
    pool's rows is 1 everywhere, so the voter's "inner rows" are all rows).
No new vote kernel: sph3d_vote_begin / _accumulate / _finalize take min_votes as it is.

  * ``evaluate_reference``: the SPECIFICATION in numpy, no GPU — evalvote.vote_reference around facadefeed.apply_reference;
  * ``FacadeVoter``: evalvote.Voter with a [B, N, 9] output set and the augmented pass;
  * ``evaluate``: the public call -> evalvote.EvalResult.
"""
import numpy as np

from . import evalvote, facadefeed, feed

MIN_VOTES = 11                       # `count > 10`
NUM_CLASSES = 7
MAX_PASSES = evalvote.MAX_PASSES


# ---------------------------------------------------------------------------------------------------------------
# the statement (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def evaluate_reference(logits_fn, blocks, normals, batch_size, num_point, seed, num_cls=NUM_CLASSES, min_votes=MIN_VOTES,
                       augment=True, max_passes=MAX_PASSES, rank=0, world=1, keep_votes=False):
    """`evaluate` stated in numpy.  blocks, normals: the host facades (facadefeed.facade_blocks);
    logits_fn(batch_index, pass, points [b, N, 9] float64, label [b, N] int32, index [b, N] int32) -> [b, N, C] float32, where
    points and label are facadefeed.apply_reference of the pass: EVAL_AUGMENT at pass_step(batch_index, pass), or recipe 0
    without `augment`"""
    evalvote.check_share(batch_size, rank, world, "evaluate_reference")
    sizes = np.array([len(b) for b in blocks], dtype=np.int64)
    rows = np.concatenate([np.asarray(b) for b in blocks], axis=0)
    P, C, recipe = len(blocks), int(num_cls), facadefeed.EVAL_AUGMENT if augment else 0
    mine = list(range(rank, feed.batches_per_epoch(P, batch_size), world))
    done = []
    for i in mine:
        ids = evalvote.batch_blocks(P, batch_size, i)

        def logits_of_pass(p, index, _i=i, _ids=ids):
            ref = facadefeed.assemble_reference(sizes, _ids, num_point, seed, evalvote.pass_step(_i, p), recipe)
            assert np.array_equal(ref.index, index)
            points, label = facadefeed.apply_reference(blocks, normals, _ids, ref)
            return logits_fn(_i, p, points, label, index)
        done.append(evalvote.vote_reference(sizes, rows[:, 6], rows[:, 7], ids, num_point, seed, i, logits_of_pass, C, min_votes,
                                            max_passes))
    return evalvote.EvalResult(sum((d.confusion for d in done), np.zeros((C, C), np.int64)), mine, [d.passes for d in done],
                               [d.covered for d in done], [d.inner_size for d in done], sum(d.nonfinite_rows for d in done),
                               dict(zip(mine, done)) if keep_votes else None)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
class FacadeVoter(evalvote.Voter):
    """evalvote.Voter's buffers and loop on a facadefeed.FacadePool: a pass draws the nine-channel sample with the evaluation's
    recipe (turn + tilt, normals included; 0 with augment=False) and votes it as pass p."""
    what = "facades"

    def __init__(self, pool, batch_size, num_point, num_cls, capacity_rows, min_votes=MIN_VOTES, augment=True):
        self.augment = bool(augment)
        super().__init__(pool, batch_size, num_point, num_cls, capacity_rows, min_votes)

    def _alloc(self, dev):
        import torch
        self.confusion = torch.zeros((self.C * self.C,), dtype=torch.int64, device=dev)
        self.out = (torch.empty((self.B, self.N, facadefeed.CHANNELS), dtype=torch.float32, device=dev),
                    torch.empty((self.B, self.N), dtype=torch.int32, device=dev))
        self.recipe = torch.full((self.B,), facadefeed.EVAL_AUGMENT if self.augment else 0, dtype=torch.int32, device=dev)

    def _pass(self, model_fn, ids_dev, out, seed, batch_index, p, vote):
        p_ = self.pool
        points, label, index = facadefeed.assemble(p_.rows, p_.normals, p_.offsets, ids_dev, self.N, seed,
                                                   evalvote.pass_step(batch_index, p), self.recipe[:int(ids_dev.shape[0])],
                                                   out=out, want_index=True)
        vote(p, index, lambda: model_fn(points, label))


def evaluate(model_fn, pool, batch_size, num_point, seed, num_cls=NUM_CLASSES, min_votes=MIN_VOTES, augment=True,
             max_passes=MAX_PASSES, rank=0, world=1, keep_votes=False, on_pass=None):
    """Evaluate a network on every facade of `pool` (facadefeed.FacadePool) -> evalvote.EvalResult.

        pool = facadefeed.FacadePool.from_records(test_paths)
        res = evaluate(lambda p, l: model(p, is_training=False)[0], pool, 16, 8192, seed=0)
        print(res.miou, res.overall_acc, res.class_iou, res.complete)

    model_fn(points [b, N, 9] fp32, label [b, N] i32) -> logits [b, N, num_cls] on the device; it is called under
    torch.no_grad() on the current stream, and the tensors it gets are overwritten by the next pass.  Batch i is facades
    [i * batch_size, (i + 1) * batch_size) of the pool; rank r of `world` takes batches r, r + world, ... and EvalResult.merge
    of the ranks' results equals the world = 1 result.  min_votes: the votes every row must have had (the reference's
    `count > 10`).  augment=False: the plain draw.  on_pass, keep_votes, max_passes: as evalvote.evaluate."""
    evalvote._check_loop_args(num_point, num_cls, min_votes, max_passes)
    evalvote.check_share(batch_size, rank, world, "evaluate")
    mine = list(range(rank, feed.batches_per_epoch(len(pool), batch_size), world))
    C = int(num_cls)
    if not mine:
        return evalvote.EvalResult(np.zeros((C, C), np.int64), [], [], [], [], 0, {} if keep_votes else None)
    spans = [evalvote.batch_blocks(len(pool), batch_size, i) for i in mine]
    cap = max(int(pool.host_offsets[ids[-1] + 1] - pool.host_offsets[ids[0]]) for ids in spans)
    voter = FacadeVoter(pool, batch_size, num_point, C, cap, min_votes, augment)
    done = [voter.run_batch(model_fn, ids, seed, i, max_passes, keep_votes, on_pass) for i, ids in zip(mine, spans)]
    confusion, nonfinite = voter.totals()
    return evalvote.EvalResult(confusion, mine, [d.passes for d in done], [d.covered for d in done],
                               [d.inner_size for d in done], nonfinite, dict(zip(mine, done)) if keep_votes else None)
