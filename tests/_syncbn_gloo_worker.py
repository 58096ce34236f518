"""world_size-2 worker of the synchronised batch-norm tests: 2 + 2 clouds in training mode under
tf_norm.sync(hdist.stat_all_reduce) against each rank's own plain run of the whole batch.  Without arguments: gloo, CPU, oracle ops
(test_gloo_world2_sync_bn_equals_whole_batch); with `cuda`: RCCL, one GPU per rank, the HIP ops."""
import contextlib
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph3d_gcn_amd import tf_norm  # noqa: E402
from sph3d_gcn_amd.harness import dist as hdist  # noqa: E402
from sph3d_gcn_amd.harness import s3dis_net, synth  # noqa: E402

CUDA = len(sys.argv) > 1 and sys.argv[1] == "cuda"


def _ops():
    if CUDA:
        return contextlib.nullcontext()
    from oracle import torch_ops
    return torch_ops.patched_util()


def _model_and_batch(blocks, cfg, dev):
    xyz, label, inner = synth.s3dis_batch(blocks[0], len(blocks), 512, extent=(0.8, 0.8, 1.0))
    model = s3dis_net.SPH3DS3DIS(cfg, device=dev, seed=7)
    pts = torch.from_numpy(xyz).to(dev)
    with torch.no_grad():
        model(pts, is_training=False)                 # creates the variables; the moving statistics stay as initialised
    return model, pts, torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)


def _buffers(model):
    return torch.cat([b.reshape(-1) for _n, b in sorted(model.named_buffers())])


def shard_run(blocks, cfg, dev, reducer):
    """the rank's clouds, training mode, bucketed flat gradient; reducer None: each rank's own statistics"""
    with _ops():
        model, pts, label, inner = _model_and_batch(blocks, cfg, dev)
        flat = hdist.FlatGradAllReduce(model.parameters(), bucket_bytes=64 << 10)
        with (tf_norm.sync(reducer) if reducer is not None else contextlib.nullcontext()):
            pred, _ = model(pts, is_training=True)
            flat.backward(model.loss(pred, label, inner))
    flat.all_reduce()
    return flat.unpadded(flat.flat).clone(), pred.detach(), _buffers(model)


def whole_run(blocks, cfg, dev):
    """plain autograd over the whole batch in one process"""
    with _ops():
        model, pts, label, inner = _model_and_batch(blocks, cfg, dev)
        pred, _ = model(pts, is_training=True)
        params = [p for p in model.parameters() if p.requires_grad]
        grads = torch.autograd.grad(model.loss(pred, label, inner), params, allow_unused=True)
    grad = torch.cat([(g if g is not None else torch.zeros_like(p)).reshape(-1) for g, p in zip(grads, params)])
    return grad, pred.detach(), _buffers(model)


def main():
    rank, world, local_rank = hdist.init_from_env(backend="nccl" if CUDA else "gloo")
    assert world == 2
    dev = torch.device("cuda", local_rank) if CUDA else torch.device("cpu")
    if CUDA:
        torch.cuda.set_device(dev)
    cfg = s3dis_net.small_config(512)
    cfg.num_sample = [128, 32]
    b, e = hdist.shard_range(4, rank, world)
    whole_grad, whole_pred, whole_buf = whole_run([0, 1, 2, 3], cfg, dev)

    calls = hdist.STAT_STATS["stat_allreduce_calls"]
    grad, pred, buf = shard_run(list(range(b, e)), cfg, dev, hdist.stat_all_reduce)
    calls = hdist.STAT_STATS["stat_allreduce_calls"] - calls
    assert calls > 0 and calls % 2 == 0, calls                       # one per batch norm and direction
    torch.testing.assert_close(grad, whole_grad, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(pred, whole_pred[b:e], rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(buf, whole_buf, rtol=1e-5, atol=1e-6)
    other = buf.clone()
    dist.broadcast(other, src=0)
    assert torch.equal(other, buf)                                    # the replicas' moving statistics are the same bits

    # sensitivity: with each rank's own statistics the summed gradient is another one
    grad0, _pred0, _buf0 = shard_run(list(range(b, e)), cfg, dev, None)
    miss = (grad0 - whole_grad).abs() > 2e-5 + 2e-4 * whole_grad.abs()
    frac = float(miss.double().mean())
    assert frac > 0.1, frac
    dist.barrier()
    if rank == 0:
        print("SYNCBN_GLOO_OK calls=%d unsynchronised_miss=%.3f" % (calls, frac))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
