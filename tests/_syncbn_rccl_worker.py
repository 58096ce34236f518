"""One rank under torch.distributed.run with SPH3D_FORCE_COLLECTIVES=1 (test_trainer_sync_bn_one_rank_over_rccl): the small S3DIS
plan on the GPU, two Trainer.train_step's with sync_bn=True — every batch-norm statistics all-reduce goes through RCCL — against
two with sync_bn=False from equal seeds.  At world size 1 the sum is the identity."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph3d_gcn_amd.harness import dist as hdist  # noqa: E402
from sph3d_gcn_amd.harness import optim, s3dis_net, synth, train  # noqa: E402

N_PTS, BATCH = 1024, 2


def run(dev, sync_bn):
    items = []
    for step in range(2):
        xyz, label, inner = synth.s3dis_batch(10 + step * BATCH, BATCH, N_PTS, extent=(1.0, 1.0, 1.5))
        items.append((torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev), None))
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N_PTS), device=dev, seed=3)
    tr = train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, BATCH), 13,
                       prime=items[0][:3], seed=5, log=lambda s: None, sync_bn=sync_bn)
    kept, add = [], tr.metrics.add
    tr.metrics.add = lambda pred, label, inner, loss_part: (kept.append(pred.detach().clone()), add(pred, label, inner, loss_part))[1]
    layers = sum(1 for n in model.store.params if n.endswith("gamma"))
    calls = []
    first = None
    for item in items:
        before = hdist.STAT_STATS["stat_allreduce_calls"]
        tr.train_step(item)
        calls.append(hdist.STAT_STATS["stat_allreduce_calls"] - before)
        if first is None:
            first = (kept[0], torch.cat([b.reshape(-1) for _n, b in sorted(model.named_buffers())]).clone(),
                     tr.flat.unpadded(tr.flat.flat).clone())
    torch.cuda.synchronize()
    assert torch.isfinite(tr.flat.flat_param).all()
    return first, calls, layers


def main():
    rank, world, local_rank = hdist.init_from_env()
    assert world == 1 and dist.is_initialized() and dist.get_backend() == "nccl" and hdist.FORCE_COLLECTIVES
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    on, calls_on, layers = run(dev, True)
    off, calls_off, _ = run(dev, False)
    assert layers > 0 and calls_on == [2 * layers, 2 * layers], (calls_on, layers)
    assert calls_off == [0, 0], calls_off
    assert torch.equal(on[0], off[0])                                  # the first step's logits
    assert torch.equal(on[1], off[1])                                  # the moving statistics after it
    torch.testing.assert_close(on[2], off[2], rtol=1e-5, atol=1e-6)    # its gradient: the sums' order is not fixed from run to run
    print("SYNCBN_RCCL_OK layers=%d stat_all_reduces_per_step=%d" % (layers, calls_on[0]))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
