"""What deterministic mode costs, on the headline plan: s3dis_config(8192), 16 blocks.

  1. the Trainer's steady-state step over a DeviceFeed with the mode off and on, in alternating groups of ONE process and ONE
     trainer (the switch is per step), host clock around K steps that end in a device synchronise; every group is printed;
  2. device time (HIP events) of one transposed-graph build, count + scan + fill[+ canonical order], with the mode off and on, at
     the four encoder levels' intra graphs (the plan's own tensors);
  3. device time of the conv gradient of each level's first separable layer on arrival-order entries (mode off) against canonical
     entries (mode on): ascending rows may help or hurt the grad_output gathers.
Groups alternate in 2 and 3 as well.  Nothing here has a pass mark.

  python tools/exp_determinism.py [groups] [steps per group]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph, tf_conv3d
from sph3d_gcn_amd.harness import feed, optim as hoptim, s3dis_net, synth, train

GROUPS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
K = int(sys.argv[2]) if len(sys.argv) > 2 else 30
B, N, SEED = 16, 8192, 1
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def med(v):
    return float(np.median(v))


def line(name, off, on, unit="ms"):
    print("%-34s off %.3f %s (min %.3f, max %.3f)   on %.3f %s (min %.3f, max %.3f)   on - off %+.3f %s (%+.1f %%)"
          % (name, med(off), unit, min(off), max(off), med(on), unit, min(on), max(on), med(on) - med(off), unit,
             (med(on) / med(off) - 1) * 100))


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
config = s3dis_net.s3dis_config(N)
model = s3dis_net.SPH3DS3DIS(config, device=dev)
trainer = train.Trainer(model, model.loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-4), train.Schedule.for_dataset("s3dis"),
                        13, prime=prime, seed=SEED, log=lambda s: None)
t_feed = feed.DeviceFeed(pool, B, N, SEED, augment=True)


def run(k, flag):
    trainer.deterministic = flag
    done = 0
    while done < k:
        for item in t_feed:
            trainer.train_step(item, t_feed)
            done += 1
            if trainer.global_step % trainer.log_every == 0:
                trainer.metrics.read()
                trainer.metrics.reset()
            if done == k:
                break


# ---- 1. the step ----------------------------------------------------------------------------------------------------------------
arms = [("off", False), ("on", True)]
for _name, flag in arms:
    run(16, flag)
torch.cuda.synchronize()
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
line("Trainer step", ms["off"], ms["on"])
print("blocks/s: off %.0f, on %.0f" % (B * 1e3 / med(ms["off"]), B * 1e3 / med(ms["on"])))
pkg.set_deterministic(False)

# ---- 2. and 3.: the levels' graphs -------------------------------------------------------------------------------------------------
plan = s3dis_net.build_graphs(prime[0], config)
torch.cuda.synchronize()
levels = []
for l in range(len(config.radius)):
    g = plan.enc(l)
    levels.append((g["intra_idx"], g["intra_cnt"], g["filt_idx"]))
F = config.binSize
CONV = [(64, 2), (128, 2), (256, 2), (256, 2)]          # input channels and multiplier of each level's first separable layer


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def build(idx, cnt, bins):
    _tgraph._cache.clear()
    _tgraph._orders.clear()                 # (so that every build writes the balanced order too, as a step's first build does)
    idx.__dict__.pop("_sph3d_tg", None)
    _tgraph.transpose(idx, cnt, idx.shape[1], bin_index=bins, num_bins=F)


REPS = 10
for l, (idx, cnt, bins) in enumerate(levels):
    Bl, Nl, Kl = idx.shape
    deg = torch.bincount(idx[0][torch.arange(Kl, device=dev)[None, :] < cnt[0][:, None]].long(), minlength=Nl)
    C, r = CONV[l]
    rng = np.random.RandomState(7 + l)
    x = torch.from_numpy(rng.randn(Bl, Nl, C).astype(np.float32)).to(dev)
    w = torch.from_numpy(rng.randn(F, C, r).astype(np.float32)).to(dev)
    go = torch.from_numpy(rng.randn(Bl, Nl, C * r).astype(np.float32)).to(dev)
    tb = {"off": [], "on": []}
    tc = {"off": [], "on": []}
    for grp in range(GROUPS):
        for name, flag in arms:
            with pkg.deterministic(flag):
                build(idx, cnt, bins)
                tb[name].append(med(timed(lambda: build(idx, cnt, bins), REPS)))
                tf_conv3d.depthwise_conv3d_grad(x, w, go, idx, cnt, bins)           # (the graph of this mode is cached now)
                tc[name].append(med(timed(lambda: tf_conv3d.depthwise_conv3d_grad(x, w, go, idx, cnt, bins), REPS)))
    print("level %d: B=%d N=%d K=%d F=%d, mean in-degree %.1f, max %d (cloud 0)" % (l, Bl, Nl, Kl, F, float(deg.float().mean()), int(deg.max())))
    line("  transposed-graph build", tb["off"], tb["on"])
    line("  conv gradient C=%d r=%d" % (C, r), tc["off"], tc["on"])
pkg.set_deterministic(False)
