"""What batch-norm statistics over all ranks' rows cost per step.

The Trainer's steady-state step on the headline plan (s3dis_config(8192), 16 blocks, DeviceFeed) with sync_bn off and on, in
alternating groups of ONE process and ONE trainer (the switch is per step), host clock around K steps that end in a device
synchronise; every group is printed.  Then, in passes of their own (the per-call events slow the host), the device time per call
of the four entry points of the cut and of the two plain ops they replace.

  python tools/exp_syncbn.py [groups] [steps per group]
      one replica, no process group: the reducer is the identity, the difference is the cut's extra launches and buffers
  SPH3D_FORCE_COLLECTIVES=1 python -m torch.distributed.run --nproc-per-node 1 tools/exp_syncbn.py [groups] [steps per group]
      one rank over RCCL: every statistics all-reduce is really issued (2 per batch-norm layer and step), a sum over one rank
No multi-GPU time comes out of this: both forms run on one GPU."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.distributed as dist
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import feed, dist as hdist, optim as hoptim, s3dis_net, synth, train

GROUPS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
K = int(sys.argv[2]) if len(sys.argv) > 2 else 30
B, N, SEED = 16, 8192, 1
rank, world, local_rank = hdist.init_from_env()
dev = torch.device("cuda", local_rank)
torch.cuda.set_device(dev)
print("process group: %s, world %d, SPH3D_FORCE_COLLECTIVES %s" % (dist.get_backend() if dist.is_initialized() else "none", world,
                                                                  hdist.FORCE_COLLECTIVES))


def med(v):
    return float(np.median(v))


prng = np.random.RandomState(0)
distinct = []
for k in range(32):
    rows = int(prng.randint(6000, 30001))
    xyz, lab, inn = synth.s3dis_block(5000 + k, rows, voxel=0.02)
    distinct.append(np.concatenate([xyz, prng.rand(rows, 3).astype(np.float32), lab.reshape(-1, 1).astype(np.float32),
                                    inn.reshape(-1, 1).astype(np.float32)], axis=1))
pool = feed.BlockPool.from_blocks(distinct * 8, dev)
ids = torch.from_numpy(feed.epoch_order(len(pool), SEED, 0)).to(dev)
prime = tuple(t.clone() for t in feed.assemble(pool.rows, pool.offsets, ids[:B], N, SEED, 0, True))
model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
trainer = train.Trainer(model, model.loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-4), train.Schedule.for_dataset("s3dis"),
                        13, prime=prime, seed=SEED, log=lambda s: None)
t_feed = feed.DeviceFeed(pool, B, N, SEED, augment=True)
layers = sum(1 for n in model.store.params if n.endswith("gamma"))


def run(k, sync_bn):
    trainer.sync_bn = sync_bn
    done = 0
    while done < k:
        for item in t_feed:
            trainer.train_step(item, t_feed)
            done += 1
            if trainer.global_step % trainer.log_every == 0:          # the loop's one read per log interval
                trainer.metrics.read()
                trainer.metrics.reset()
            if done == k:
                break


arms = [("sync_bn off", False), ("sync_bn on", True)]
for name, flag in arms:
    run(16, flag)
torch.cuda.synchronize()
c0 = hdist.STAT_STATS["stat_allreduce_calls"]
run(1, True)
print("batch-norm layers %d, stat_all_reduce calls per step %d" % (layers, hdist.STAT_STATS["stat_allreduce_calls"] - c0))
ms = {name: [] for name, _ in arms}
for grp in range(GROUPS):
    for name, flag in arms:
        run(3, flag)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(K, flag)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / K)
    print("group %d (%d steps each): " % (grp, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
base = med(ms["sync_bn off"])
for name, _ in arms:
    x = ms[name]
    print("%-11s median %.3f ms per step (min %.3f, max %.3f) = %.0f blocks/s; against off %+.3f ms (%+.2f %%)"
          % (name, med(x), min(x), max(x), B * 1e3 / med(x), med(x) - base, (med(x) / base - 1) * 100))

# device time per call, HIP events around every C-ABI call: a pass of its own per arm
for name, flag in arms:
    run(2, flag)
    torch.cuda.synchronize()
    _lib.timing_start()
    run(3, flag)
    rec = _lib.timing_stop()
    torch.cuda.synchronize()
    per = {}
    for nm, _args, e0, e1 in rec:
        if "elu_bn" in nm:
            per.setdefault(nm, []).append(e0.elapsed_time(e1) * 1e3)
    for nm in sorted(per):
        v = per[nm]
        print("%-11s %-32s %3d calls per step, %.1f us per call (median; min %.1f, max %.1f), %.3f ms per step"
              % (name, nm, len(v) // 3, med(v), min(v), max(v), sum(v) / 3e3))
if dist.is_initialized():
    dist.destroy_process_group()
