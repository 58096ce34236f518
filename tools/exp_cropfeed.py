"""The crop feed, measured, on synthetic rooms from harness/scenesynth.py.

  (a) call     device us of cropfeed.assemble at 16 x 8192 beside feed.assemble in the same run, by tools/exp_guard.py's method:
               200 calls back to back between one event pair, repeated; every arm twice, in turn.  The block pool of the feed
               arm is the SAME rooms cut by scenesynth.split_scene, so both arms gather from data of one kind.
  (b) step     Trainer.train_step on the headline plan (s3dis_config(8192), 16 clouds) fed by DeviceFeed over the block pool and
               by CropFeed over the scene pool, in alternating groups of one process, host clock around K steps that end in a
               device synchronise.  Every group is printed; the DeviceFeed arm's own spread across them is the yardstick.  A
               third arm tells the feed's cost from the data's: DeviceFeed over a block pool whose blocks ARE crops (the member
               rows of as many crops as there are blocks, drawn by the statement on the host) — the same launch as the first
               arm on clouds shaped like the second's.  The CropFeed arm runs epochs as long as DeviceFeed's (one crop per
               block of the block pool); a fourth arm runs CropFeed's own default epoch, max(1, round(T / N)) crops, which is
               shorter here: an epoch's start (the id table's upload) and its short last batch (another batch size: new plans)
               then come round more often.
usage: python tools/exp_cropfeed.py [pairs] [steps per group] [rooms]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import cropfeed, feed, optim as hoptim, s3dis_net, scenesynth, train

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
K = int(sys.argv[2]) if len(sys.argv) > 2 else 30
ROOMS = int(sys.argv[3]) if len(sys.argv) > 3 else 6
B, N, SEED = 16, 8192, 1
dev = torch.device("cuda:0"); l = _lib.lib()


def med(v):
    return float(np.median(v))


def timed(fn, launches=200, repeats=7):
    """us per call: `launches` back to back between one event pair, median / min / max of `repeats`"""
    for _ in range(20):
        fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return med(out), min(out), max(out)


# ---- the rooms: as a scene pool and, cut into the reference's squares, as a block pool -------------------------------------------
scenes, blocks = [], []
for s in range(ROOMS):
    ext = (5.0 + s % 3, 4.0 + s % 2, 3.0)
    _fx, _fl, vx, vl = scenesynth.synthetic_scene(100 + s, 900000, extent=ext, voxel=0.03)
    # the room's bottom centre to the origin, as sceneprep.normalise does
    vx = (vx - np.array([ext[0] / 2, ext[1] / 2, 0.0])).astype(np.float32)
    rgb = (np.random.RandomState(s).rand(len(vx), 3) * 2 - 1).astype(np.float32)
    scenes.append((vx, rgb, vl))
    blocks += scenesynth.split_scene(vx, vl, rgb)[0]
t0 = time.perf_counter()
spool = cropfeed.ScenePool.from_arrays(scenes, dev, keep_host=True)
print("scene pool: %d rooms, %d rows, %d columns; column sort + upload %.2f s on the host"
      % (len(spool), int(spool.sizes.sum()), int(spool.col_start.shape[0]), time.perf_counter() - t0))
bpool = feed.BlockPool.from_blocks(blocks, dev)
print("block pool: %d blocks, %d rows (%.1f x the scenes' rows)" % (len(bpool), int(bpool.sizes.sum()),
                                                                    bpool.sizes.sum() / float(spool.sizes.sum())))

# blocks that are crops: the members of crop k of room k % ROOMS under the default geometry, inner by the crop's rule
geo = cropfeed.crop_geometry(N, spool.cell)
crop_blocks = []
for k in range(len(bpool)):
    sc = spool.host[k % ROOMS]
    _a, _r, win, _T = cropfeed.choose(sc, feed.cloud_key(SEED + 1, k, 0), geo)
    mem = cropfeed.members(sc, win)
    blk = sc.rows[mem].copy()
    blk[:, 7] = cropfeed.inner_of(sc, mem, win, geo.inner_half)
    crop_blocks.append(blk)
cpool = feed.BlockPool.from_blocks(crop_blocks, dev)
print("crop-shaped block pool: %d blocks, rows min %d, median %d, max %d (the squares: min %d, median %d, max %d)"
      % (len(cpool), cpool.sizes.min(), int(np.median(cpool.sizes)), cpool.sizes.max(), bpool.sizes.min(),
         int(np.median(bpool.sizes)), bpool.sizes.max()))

# ---- (a) the call beside the feed ---------------------------------------------------------------------------------------------------
bids = torch.from_numpy(feed.epoch_order(len(bpool), SEED, 0)[:B].copy()).to(dev)
sids = torch.from_numpy((np.arange(B) % len(spool)).astype(np.int32)).to(dev)
out_b = tuple(t.clone() for t in feed.assemble(bpool.rows, bpool.offsets, bids, N, SEED, 0, True))
out_c = tuple(t.clone() for t in cropfeed.assemble(spool, sids, N, SEED, 0, True, geometry=geo))
crop = out_c[3].cpu().numpy()
print("(a) crops of step 0: T min %d, median %d, max %d; attempts used %s; inner share %.3f"
      % (crop[:, 3].min(), int(np.median(crop[:, 3])), crop[:, 3].max(), crop[:, 2].tolist(), float(out_c[2].float().mean())))
arms = [("feed.assemble 16 x 8192", lambda: feed.assemble(bpool.rows, bpool.offsets, bids, N, SEED, 0, True, out=out_b)),
        ("cropfeed.assemble 16 x 8192", lambda: cropfeed.assemble(spool, sids, N, SEED, 0, True, out=out_c, geometry=geo))]
res = {name: [] for name, _ in arms}
for rnd in range(2):                 # (every arm twice, in turn: drift shows)
    for name, fn in arms:
        t = timed(fn)
        res[name].append(t[0])
        print("(a) %-28s %.1f us (min %.1f, max %.1f)" % (name, t[0], t[1], t[2]))
fa, ca = med(res[arms[0][0]]), med(res[arms[1][0]])
print("(a) cropfeed.assemble / feed.assemble = %.1f / %.1f us = %.2f" % (ca, fa, ca / fa))

# ---- (b) the step: DeviceFeed against CropFeed ----------------------------------------------------------------------------------------
feed_stream = torch.cuda.Stream(device=dev)      # (one feed stream for both arms: tools/exp_feed.py says why)
prime = tuple(t.clone() for t in out_b)


def make(new_feed):
    model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
    tr = train.Trainer(model, model.loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-4), train.Schedule.for_dataset("s3dis"), 13,
                       prime=prime, seed=SEED, log=lambda s: None)
    f = new_feed()

    def run(k):
        done = 0
        while done < k:
            for item in f:
                tr.train_step(item, f)
                done += 1
                if tr.global_step % tr.log_every == 0:          # the loop's reads per log interval
                    tr.metrics.read()
                    tr.metrics.reset()
                if done == k:
                    break
    return tr, run


arms = [("DeviceFeed", make(lambda: feed.DeviceFeed(bpool, B, N, SEED, augment=True, stream=feed_stream))),
        ("CropFeed", make(lambda: cropfeed.CropFeed(spool, B, N, SEED, crops_per_epoch=len(bpool), augment=True, stream=feed_stream))),
        ("CropFeed, own epoch", make(lambda: cropfeed.CropFeed(spool, B, N, SEED, augment=True, stream=feed_stream))),
        ("DeviceFeed on crops", make(lambda: feed.DeviceFeed(cpool, B, N, SEED, augment=True, stream=feed_stream)))]
for name, (tr, run) in arms:
    run(16)
torch.cuda.synchronize()
ms = {name: [] for name, _ in arms}
for pair in range(PAIRS):
    for name, (tr, run) in arms:
        run(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(K)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / K)
    print("(b) group %d (%d steps each): " % (pair, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
d, c, x, o = ms["DeviceFeed"], ms["CropFeed"], ms["DeviceFeed on crops"], ms["CropFeed, own epoch"]
print("(b) batches per epoch: DeviceFeed %d, CropFeed %d, CropFeed with its own epoch %d"
      % (feed.batches_per_epoch(len(bpool), B), feed.batches_per_epoch(len(bpool), B),
         feed.batches_per_epoch(cropfeed.default_crops_per_epoch(spool.sizes.sum(), N), B)))
print("(b) DeviceFeed median %.3f ms per step (min %.3f, max %.3f: spread %.3f ms)" % (med(d), min(d), max(d), max(d) - min(d)))
print("(b) CropFeed   median %.3f ms per step (min %.3f, max %.3f); crop - block %+.3f ms = %+.2f %%"
      % (med(c), min(c), max(c), med(c) - med(d), (med(c) / med(d) - 1) * 100))
print("(b) DeviceFeed on crop-shaped blocks median %.3f ms per step (min %.3f, max %.3f); CropFeed - this %+.3f ms"
      % (med(x), min(x), max(x), med(c) - med(x)))
print("(b) CropFeed with its own epoch median %.3f ms per step (min %.3f, max %.3f); - DeviceFeed %+.3f ms"
      % (med(o), min(o), max(o), med(o) - med(d)))
