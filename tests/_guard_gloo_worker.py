"""world_size-2 gloo worker of test_gloo_world2_ranks_skip_together (CPU, oracle ops): a Trainer with a skipping guard and an
EMA on each rank, one cloud per rank; at the second step rank 1's LOCAL gradient holds a NaN.  The guard runs on the all-reduced
gradient, so both ranks skip that step, with no collective of their own, and their parameters, slots, EMA and guard states stay
the same bits."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import torch_ops  # noqa: E402
from sph3d_gcn_amd.harness import dist as hdist  # noqa: E402
from sph3d_gcn_amd.harness import optim, s3dis_net, synth, train  # noqa: E402

N = 512


def _item(seed, clouds):
    xyz, label, inner = synth.s3dis_batch(seed, clouds, N, extent=(0.8, 0.8, 1.0))
    return torch.from_numpy(xyz), torch.from_numpy(label).long(), torch.from_numpy(inner), None


def _same_on_both(t):
    other = t.clone()
    dist.broadcast(other, src=0)
    return torch.equal(other.view(torch.int32) if other.dtype == torch.float32 else other, t.view(torch.int32) if t.dtype == torch.float32 else t)


def main():
    rank, world, _ = hdist.init_from_env(backend="gloo")
    assert world == 2
    cfg = s3dis_net.small_config(N)
    cfg.num_sample = [128, 32]
    with torch_ops.patched_util():
        model = s3dis_net.SPH3DS3DIS(cfg, device=torch.device("cpu"), seed=7)
        tr = train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, 2, decay_step=100),
                           13, prime=_item(0, 1)[:3], seed=1, log=lambda s: None, grad_scale=0.5, skip_nonfinite=True, ema_decay=0.9)
        finish = tr.flat._finish_bucket
        planted = []

        def local_nan(bi, grads):
            if rank == 1 and tr.global_step == 1 and bi == 0:
                grads = list(grads)
                grads[0] = torch.full_like(tr.flat.params[tr.flat.buckets[0][0]], float("nan"))
                planted.append(bi)
            return finish(bi, grads)
        tr.flat._finish_bucket = local_nan
        snaps = []
        for step in range(3):
            tr.train_step(_item(10 * step + rank, 1))               # each rank its own cloud
            snaps.append((tr.flat.flat_param.detach().clone(), tr.opt.m.clone(), tr.guard.ema.clone(), tr.guard.words()))
            for t in (tr.flat.flat_param.detach(), tr.opt.m, tr.opt.v, tr.guard.ema, tr.guard.state):
                assert _same_on_both(t), (rank, step)
    assert planted == ([0] if rank == 1 else [])
    assert tr.guard.read()[:2] == (2, 1) and tr.opt.state_dict()["step"] == 2
    # the skipped step left everything as the first step had it; the third moved on; nothing is NaN
    for a, b in zip(snaps[0][:3], snaps[1][:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(snaps[1][0], snaps[2][0]) and torch.isfinite(snaps[2][0]).all() and torch.isfinite(snaps[2][2]).all()
    assert all(torch.isfinite(b).all() for _n, b in model.named_buffers() if b.dtype == torch.float32)
    assert int(tr.metrics.read().update_nonfinite) > 0
    assert int(np.asarray(snaps[1][3])[2]) == 1 and int(np.asarray(snaps[1][3])[3]) == 1
    dist.barrier()
    if rank == 0:
        print("GUARD_GLOO_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
