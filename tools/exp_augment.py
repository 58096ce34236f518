"""The augmentation stage, measured.

  (a) stage    device us of sph3d_augment_apply at 16 x 8192 x 6 (S3DIS layout) and 16 x 8192 x 9 (facade layout) beside
               feed.assemble in the same run, by tools/exp_guard.py's method: 200 calls back to back between one event pair,
               repeated; every arm twice, in turn.  The stage works in place, so each of its calls is preceded by a device copy
               that restores the batch; the copy alone is an arm of its own and is to be subtracted.
  (b) alone    each transform alone (its probability 1, the others disabled), same method, 6 channels.
  (c) host     harness/augment.py's numpy statement on the host, one batch, wall clock.
  (d) step     Trainer.train_step on the headline plan (s3dis_config(8192), 16 blocks, DeviceFeed) with the stage off and on, in
               alternating pairs of one process, host clock around K steps that end in a device synchronise.  Every pair is
               printed; the off arm's own spread across the pairs is the yardstick for the difference.
usage: python tools/exp_augment.py [pairs] [steps per group]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import augment, feed, optim as hoptim, s3dis_net, synth, train

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
K = int(sys.argv[2]) if len(sys.argv) > 2 else 30
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


prng = np.random.RandomState(0)
distinct = []
for k in range(32):
    rows = int(prng.randint(6000, 30001))
    xyz, lab, inn = synth.s3dis_block(5000 + k, rows, voxel=0.02)
    distinct.append(np.concatenate([xyz, (prng.rand(rows, 3) * 2 - 1).astype(np.float32), lab.reshape(-1, 1).astype(np.float32),
                                    inn.reshape(-1, 1).astype(np.float32)], axis=1))
pool = feed.BlockPool.from_blocks(distinct * 8, dev)
ids = torch.from_numpy(feed.epoch_order(len(pool), SEED, 0)).to(dev)
src6 = tuple(t.clone() for t in feed.assemble(pool.rows, pool.offsets, ids[:B], N, SEED, 0, True))
nrm = torch.nn.functional.normalize(torch.randn(B, N, 3, device=dev), dim=2)
src9 = (torch.cat([src6[0][..., 0:3], nrm, src6[0][..., 3:6]], dim=2).contiguous(), src6[1], src6[2])
out6 = tuple(torch.empty_like(t) for t in src6)


def stage_arm(src, opts):
    work = tuple(t.clone() for t in src)
    st = augment.Stage(opts, B, N, int(src[0].shape[2]), dev)

    def restore():
        for w, s in zip(work, src):
            w.copy_(s)

    def run():
        restore()
        st(SEED, 3, work)
    return restore, run, st


# ---- (a) the stage beside the feed ------------------------------------------------------------------------------------------------
r6, a6, st6 = stage_arm(src6, augment.default_options("s3dis"))
r9, a9, st9 = stage_arm(src9, augment.default_options("facade"))
arms = [("feed.assemble 16 x 8192 x 6", lambda: feed.assemble(pool.rows, pool.offsets, ids[:B], N, SEED, 0, True, out=out6)),
        ("restore copy, 6 channels", r6), ("restore + stage, 6 channels", a6),
        ("restore copy, 9 channels", r9), ("restore + stage, 9 channels", a9)]
for rnd in range(2):                 # (every arm twice, in turn: drift shows)
    for name, fn in arms:
        t = timed(fn)
        print("(a) %-30s %.1f us (min %.1f, max %.1f)" % (name, t[0], t[1], t[2]))
print("(a) counters after the arms: 6 channels %s, 9 channels %s" % (st6.read()[1:3], st9.read()[1:3]))
print("(a) gates of the 6-channel batch: %s" % augment.read_gates(st6.workspace, B).tolist())

# ---- (b) each transform alone ---------------------------------------------------------------------------------------------------
names = ("MIX", "FLIPX", "FLIPY", "ASCALE", "ELASTIC", "AUTOCONTRAST", "CTRANSLATE", "CJITTER", "CDROP")
base = timed(r6)
print("(b) restore copy alone %.1f us" % base[0])
for k, name in enumerate(names):
    opts = augment.default_options("s3dis", enable=1 << k)._replace(prob=(1.0,) * 9)
    _r, run, st = stage_arm(src6, opts)
    t = timed(run)
    print("(b) %-13s %.1f us with the copy (min %.1f, max %.1f), %.1f us without; counters %s"
          % (name, t[0], t[1], t[2], t[0] - base[0], st.read()[1:3]))

# ---- (c) the numpy statement on the host ------------------------------------------------------------------------------------------
host = tuple(t.cpu().numpy() for t in src6)
augment.apply_reference(*host, SEED, 3, augment.default_options("s3dis"))
t0 = time.perf_counter()
for step in range(3):
    augment.apply_reference(*host, SEED, step, augment.default_options("s3dis"))
print("(c) apply_reference, 16 x 8192 x 6 on the host: %.1f ms per batch" % ((time.perf_counter() - t0) * 1e3 / 3))

# ---- (d) the step: stage off against stage on --------------------------------------------------------------------------------------
feed_stream = torch.cuda.Stream(device=dev)      # (one feed stream for both arms: tools/exp_feed.py says why)
prime = tuple(t.clone() for t in src6)


def make(post):
    model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
    tr = train.Trainer(model, model.loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-4), train.Schedule.for_dataset("s3dis"), 13,
                       prime=prime, seed=SEED, log=lambda s: None)
    f = feed.DeviceFeed(pool, B, N, SEED, augment=True, stream=feed_stream, post=post)

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


stage = augment.Stage(augment.default_options("s3dis"), B, N, 6, dev)
arms = [("stage off", make(None)), ("stage on", make(stage))]
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
    print("(d) pair %d (%d steps each): " % (pair, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
off, on = ms["stage off"], ms["stage on"]
print("(d) stage off median %.3f ms per step (min %.3f, max %.3f: spread %.3f ms)" % (med(off), min(off), max(off), max(off) - min(off)))
print("(d) stage on  median %.3f ms per step (min %.3f, max %.3f); on - off %+.3f ms = %+.2f %%"
      % (med(on), min(on), max(on), med(on) - med(off), (med(on) / med(off) - 1) * 100))
print("(d) stage on: counters %s" % (stage.read()[1:3],))
