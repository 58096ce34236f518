"""The guarded update, measured.

  (a) update   device us of sph3d_train_update beside sph3d_train_update_guarded (its three launches together), without and
               with the EMA, in the same run at the S3DIS net's parameter count, by tools/exp_train.py's method: 200 calls back
               to back between one event pair, repeated; every arm twice, in turn.  Bytes: 28 B / parameter for the plain Adam
               update, 32 B guarded (the gradient is read twice), 40 B with the EMA.
  (b) step     Trainer.train_step on the headline plan (s3dis_config(8192), 16 blocks, DeviceFeed) with the guard off and on
               (clip_norm, skip_nonfinite, ema_decay all set: the moving statistics' copy and restore included), in alternating
               pairs of one process, host clock around K steps that end in a device synchronise.  Every pair is printed; the off
               arm's own spread across the pairs is the yardstick for the difference.
usage: python tools/exp_guard.py [pairs] [steps per group]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import feed, guard, optim as hoptim, s3dis_net, synth, train

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


# ---- (a) the update -----------------------------------------------------------------------------------------------------------
n = 3_900_000
rng = np.random.RandomState(0)
p = torch.from_numpy((rng.randn(n) * 0.1).astype(np.float32)).to(dev)
g = torch.from_numpy((rng.randn(n) * 1e-3).astype(np.float32)).to(dev)
m, v, e, q = torch.zeros_like(p), torch.zeros_like(p), p.clone(), torch.empty_like(p)
cnt = torch.zeros(1, dtype=torch.int64, device=dev)
state = torch.from_numpy(guard.new_state()).to(dev)
ws = torch.empty(l.sph3d_train_guard_workspace(n), dtype=torch.uint8, device=dev)
st = _lib.stream_ptr


def guarded(ema, clip):
    return lambda: l.sph3d_train_update_guarded(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema, 0, 1e-3, 0.9, 0.999, 1e-4,
                                                1.0, clip, 1, 0.999, state.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), st())


arms = [
    ("sph3d_train_update TF Adam", 28, lambda: l.sph3d_train_update(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-4, 5, 1.0, cnt.data_ptr(), st())),
    ("guarded, never clipping", 32, guarded(None, 1e30)),
    ("guarded, clipping every step", 32, guarded(None, 1e-3)),
    ("guarded + EMA, never clipping", 40, guarded(e.data_ptr(), 1e30)),
    ("copy p -> q (8 B / element)", 8, lambda: q.copy_(p)),
]
for rnd in range(2):                 # (every arm twice, in turn: drift shows)
    for name, bytes_per, fn in arms:
        t = timed(fn)
        print("(a) %-34s %.1f us (min %.1f, max %.1f) = %.2f TB/s at %d B / parameter" % (name, t[0], t[1], t[2], n * bytes_per / t[0] / 1e6, bytes_per))
print("(a) state after the arms: %s" % (guard.stats(state.cpu().numpy()),))

# ---- (b) the step: guard off against guard on -------------------------------------------------------------------------------------
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
feed_stream = torch.cuda.Stream(device=dev)      # (one feed stream for both arms: tools/exp_feed.py says why)


def make(**kw):
    model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
    tr = train.Trainer(model, model.loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-4), train.Schedule.for_dataset("s3dis"), 13,
                       prime=prime, seed=SEED, log=lambda s: None, **kw)
    f = feed.DeviceFeed(pool, B, N, SEED, augment=True, stream=feed_stream)

    def run(k):
        done = 0
        while done < k:
            for item in f:
                tr.train_step(item, f)
                done += 1
                if tr.global_step % tr.log_every == 0:          # the loop's reads per log interval
                    tr.metrics.read()
                    tr.metrics.reset()
                    if tr.guard is not None:
                        tr.guard.read()
                if done == k:
                    break
    return tr, run


arms = [("guard off", make()), ("guard on", make(clip_norm=10.0, skip_nonfinite=True, ema_decay=0.999))]
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
    print("(b) pair %d (%d steps each): " % (pair, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
off, on = ms["guard off"], ms["guard on"]
print("(b) guard off median %.3f ms per step (min %.3f, max %.3f: spread %.3f ms)" % (med(off), min(off), max(off), max(off) - min(off)))
print("(b) guard on  median %.3f ms per step (min %.3f, max %.3f); on - off %+.3f ms = %+.2f %%"
      % (med(on), min(on), max(on), med(on) - med(off), (med(on) / med(off) - 1) * 100))
print("(b) guard on: %s, %d buffer elements guarded" % (arms[1][1][0].guard.read(), arms[1][1][0]._buf_flat.numel()))
