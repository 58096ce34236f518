"""The odd-width conv gradient and deterministic mode on the ModelNet plan, modelnet_config(10000), 32 clouds.

  1. device time (HIP events) of the conv gradient at the plan's two odd shapes with r = 1 — level 1: 32 x 2500 sources, C = 67;
     level 2: 32 x 625 sources, C = 131; K = 64, 33 bins, the plan's own graphs — through the C entry:
       generic   dwconv_bwd_t_generic, mode off (what the entry runs for these shapes by default)
       odd       dwconv_bwd_t_odd, mode on (what it refused before)
     and through the package (tf_conv3d.depthwise_conv3d_grad):
       mode off  zero-pads odd channel counts to a multiple of four (tf_conv3d._channel_pad): pads, the four-channels-per-lane
                 kernel at C + 1, slices
       mode on   no padding for these shapes: the odd kernel, the C entry's bits (printed: the two results' difference)
  2. Trainer.train_step over an ObjectFeed with the mode off and on (keyed dropout follows the mode), host clock around K steps
     that end in a device synchronise.
Alternating groups in one process; every group is printed.  Nothing here has a pass mark.

  python tools/exp_bwd_odd.py [groups] [steps per group]"""
import inspect, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph, tf_conv3d
from sph3d_gcn_amd.harness import modelnet_net, objfeed, optim as hoptim, synth, train
from sph3d_gcn_amd.harness.s3dis_net import GraphPlan

GROUPS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
K = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B, N, SEED, REPS = 32, 10000, 1, 10
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
P, S = _lib.ptr, _lib.stream_ptr


def med(v):
    return float(np.median(v))


def stat(name, v, unit="ms"):
    print("  %-34s %.3f %s (min %.3f, max %.3f)" % (name, med(v), unit, min(v), max(v)))


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


# ---- 1. the kernels at the plan's graphs ------------------------------------------------------------------------------------------
config = modelnet_net.modelnet_config(N)
pts = torch.from_numpy(synth.modelnet_batch(0, B, N)[:, :, :3].copy()).to(dev)
plan = GraphPlan(pts, config, decoder=False, global_kernel=[8, 2, 1], global_query="centroid", prepare_input=False,
                 xyz_transform=modelnet_net.normalize_xyz)
torch.cuda.synchronize()
F = config.binSize


def c_entry(x, w, go, idx, cnt, bins):
    """sph3d_depthwise_conv3d_grad_t at the shape as it is (no padding) on the package's transposed graph"""
    Bl, Nl, C = x.shape
    M = idx.shape[1]
    l = _lib.lib()
    off, key, scale, act = _tgraph.transpose(idx, cnt, Nl, bin_index=bins, num_bins=F)
    wsb = l.sph3d_depthwise_conv3d_grad_t_workspace(Bl, Nl, F, C, 1)
    ws = _lib.scratch(wsb, x.device)
    gi, gf = torch.empty_like(x), torch.empty_like(w)
    _lib.check(l.sph3d_depthwise_conv3d_grad_t(Bl, Nl, M, F, C, 1, P(off), P(key), P(scale), P(_tgraph.source_order(idx)), P(act), P(x), P(w),
                                               P(go), P(gi), P(gf), P(ws), wsb, S()))
    return gi, gf


for level, C in ((1, 67), (2, 131)):
    g = plan.enc(level)
    idx, cnt, bins = g["intra_idx"], g["intra_cnt"], g["filt_idx"]
    Bl, Nl, Kl = idx.shape
    rng = np.random.RandomState(7 + level)
    x = torch.from_numpy(rng.randn(Bl, Nl, C).astype(np.float32)).to(dev)
    w = torch.from_numpy(rng.randn(F, C, 1).astype(np.float32)).to(dev)
    go = torch.from_numpy(rng.randn(Bl, Nl, C).astype(np.float32)).to(dev)
    arms = [("generic, mode off", False, c_entry), ("odd, mode on", True, c_entry),
            ("package, mode off (padded)", False, tf_conv3d.depthwise_conv3d_grad), ("package, mode on (odd)", True, tf_conv3d.depthwise_conv3d_grad)]
    t = {name: [] for name, _f, _fn in arms}
    for grp in range(GROUPS):
        for name, flag, fn in arms:
            with pkg.deterministic(flag):
                fn(x, w, go, idx, cnt, bins)                                # (builds and caches this mode's transposed graph)
                t[name].append(med(timed(lambda: fn(x, w, go, idx, cnt, bins))))
    deg = torch.bincount(idx[0][torch.arange(Kl, device=dev)[None, :] < cnt[0][:, None]].long(), minlength=Nl)
    print("level %d: B=%d N=%d K=%d F=%d C=%d r=1, mean in-degree %.1f, max %d (cloud 0); medians of %d groups of %d launches"
          % (level, Bl, Nl, Kl, F, C, float(deg.float().mean()), int(deg.max()), GROUPS, REPS))
    for name, _f, _fn in arms:
        stat(name, t[name])
    with pkg.deterministic():
        a, b = c_entry(x, w, go, idx, cnt, bins), tf_conv3d.depthwise_conv3d_grad(x, w, go, idx, cnt, bins)
        print("  C entry against package, mode on: max |d grad_input| %.3e, max |d grad_filter| %.3e (of %.3e)"
              % (float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()), float(b[1].abs().max())))
pkg.set_deterministic(False)
del plan

# ---- 2. the step ----------------------------------------------------------------------------------------------------------------
shapes = [synth.modelnet_cloud(500 + k, 10000 + 137 * (k % 16)) for k in range(64)]
classes = [k % 40 for k in range(64)]
pool = objfeed.ShapePool.from_arrays(shapes, classes, classes, device=dev)
ids = torch.arange(B, dtype=torch.int32, device=dev)
points, label = objfeed.assemble(pool.rows, pool.offsets, ids, N, SEED, 0, 0)
model = modelnet_net.SPH3DModelNet(config, device=dev)
trainer = train.Trainer(model, modelnet_net.get_loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-8), train.Schedule.for_dataset("modelnet"),
                        40, line=train.modelnet_line, prime=(points, label, pool.category_dev[:B]), seed=SEED, log=lambda s: None)
t_feed = objfeed.ObjectFeed(pool, B, N, seed=SEED, dataset="modelnet")
has_key = "dropout_key" in inspect.signature(model.forward).parameters


def run(k, flag):
    trainer.deterministic = flag
    trainer.keyed_dropout = flag and has_key
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


arms = [("off", False), ("on", True)]
for _name, flag in arms:
    run(6, flag)
torch.cuda.synchronize()
ms = {name: [] for name, _ in arms}
for grp in range(GROUPS):
    for name, flag in arms:
        run(2, flag)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(K, flag)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / K)
    print("group %d (%d steps each): " % (grp, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
print("Trainer step, modelnet_config(%d), B=%d:" % (N, B))
stat("mode off", ms["off"])
stat("mode on (keyed dropout)", ms["on"])
print("  on - off %+.3f ms (%+.1f %%); clouds/s: off %.0f, on %.0f"
      % (med(ms["on"]) - med(ms["off"]), (med(ms["on"]) / med(ms["off"]) - 1) * 100, B * 1e3 / med(ms["off"]), B * 1e3 / med(ms["on"])))
pkg.set_deterministic(False)
