"""The training loop's own kernels and the Trainer, measured.

  (a) update   sph3d_train_update (TF Adam, Nesterov momentum) against sph3d_adam_step in the same run at the S3DIS net's
               parameter count: 200 launches back to back between one event pair, repeated; what the bytes cost is
               28 B / parameter (Adam forms) and 20 B / parameter (momentum) at the achieved copy rate of the same run.
  (b) metrics  sph3d_train_metrics at 16 x 8192 x 13 and 32 x 1 x 40 by the same method, against the reference's form: the
               logits to the host and np.argmax + the per-block loops' counts (host clock, it ends in a copy).
  (c) step     the Trainer's steady-state step on the headline plan (s3dis_config(8192), 16 blocks, DeviceFeed) against the
               hand-written loop of tools/exp_feed.py with the same optimiser, in alternating groups of one process, host clock
               around K steps that end in a device synchronise.  Every group is printed.
usage: python tools/exp_train.py [groups] [steps per group]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import feed, dist as hdist, optim as hoptim, s3dis_net, synth, train

GROUPS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
K = int(sys.argv[2]) if len(sys.argv) > 2 else 30
B, N, SEED = 16, 8192, 1
dev = torch.device("cuda:0"); l = _lib.lib()


def med(v):
    return float(np.median(v))


def timed(fn, launches=200, repeats=7):
    """us per launch: `launches` back to back between one event pair, median / min / max of `repeats`"""
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
m, v, q = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
cnt = torch.zeros(1, dtype=torch.int64, device=dev)
st = _lib.stream_ptr
arms = [
    ("sph3d_adam_step (torch form)", 28, lambda: l.sph3d_adam_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 0.9, 0.999, 1e-4, 5, st())),
    ("sph3d_train_update TF Adam", 28, lambda: l.sph3d_train_update(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-4, 5, 1.0, cnt.data_ptr(), st())),
    ("sph3d_train_update TF Adam, no counter", 28, lambda: l.sph3d_train_update(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-4, 5, 1.0, None, st())),
    ("sph3d_train_update Nesterov", 20, lambda: l.sph3d_train_update(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), None, 1, 1e-3, 0.9, 0.0, 0.0, 5, 1.0, cnt.data_ptr(), st())),
    ("copy p -> q (8 B / element)", 8, lambda: q.copy_(p)),
]
for rnd in range(2):                 # (every arm twice, in turn: drift shows)
    for name, bytes_per, fn in arms:
        t = timed(fn)
        print("(a) %-42s %.1f us (min %.1f, max %.1f) = %.2f TB/s at %d B / parameter" % (name, t[0], t[1], t[2], n * bytes_per / t[0] / 1e6, bytes_per))

# ---- (b) the metrics -----------------------------------------------------------------------------------------------------------
for (b, npts, C) in ((16, 8192, 13), (32, 1, 40)):
    logits = torch.from_numpy(rng.randn(b, npts, C).astype(np.float32)).to(dev)
    label = torch.from_numpy(rng.randint(0, C, (b, npts)).astype(np.int32)).to(dev)
    inner = torch.from_numpy(rng.randint(0, 2, (b, npts)).astype(np.int32)).to(dev)
    part = torch.ones(1, dtype=torch.float32, device=dev)
    tm = train.TrainMetrics(C, dev)
    t = timed(lambda: tm.add(logits, label, inner, part))

    def host_form():
        pv = np.argmax(logits.cpu().numpy(), 2)
        lab, inn = label.cpu().numpy(), inner.cpu().numpy()
        correct = seen = 0
        for k in range(b):
            idx = inn[k] == 1
            correct += np.sum(pv[k, idx] == lab[k, idx])
            seen += sum(idx)
        return correct, seen
    host_form()
    hs = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_form()
        hs.append((time.perf_counter() - t0) * 1e6)
    print("(b) %d x %d x %d: sph3d_train_metrics %.1f us per call (min %.1f, max %.1f); .cpu() + numpy %.0f us (min %.0f, max %.0f)"
          % (b, npts, C, t[0], t[1], t[2], med(hs), min(hs), max(hs)))

# ---- (c) the step: Trainer against the hand-written loop ---------------------------------------------------------------------------
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

# the hand-written loop (tools/exp_feed.py's, with the reference's optimiser so that both arms launch the same update)
model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
model.loss(model(prime[0], is_training=True)[0], prime[1], prime[2]).backward()
flat = hdist.FlatGradAllReduce(model.parameters())
opt = hoptim.FlatTFAdam(flat.flat_param, lr=1e-3, eps=1e-4)
hand_feed = feed.DeviceFeed(pool, B, N, SEED, augment=True, stream=feed_stream)


def hand(k):
    done = 0
    while done < k:
        for pts, label, inner, ready in hand_feed:
            pred, _ = model(pts, is_training=True, points_ready=ready)
            loss = model.loss(pred, label, inner)
            hand_feed.done(ready)
            flat.backward(loss)
            flat.all_reduce()
            opt.step()
            done += 1
            if done == k:
                break


tmodel = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
trainer = train.Trainer(tmodel, tmodel.loss, lambda fp: hoptim.FlatTFAdam(fp, lr=1e-3, eps=1e-4), train.Schedule.for_dataset("s3dis"),
                        13, prime=prime, seed=SEED, log=lambda s: None)
t_feed = feed.DeviceFeed(pool, B, N, SEED, augment=True, stream=feed_stream)


def with_trainer(k):
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


arms = [("hand loop", hand), ("Trainer", with_trainer)]
for name, run in arms:
    run(16)
torch.cuda.synchronize()
ms = {name: [] for name, _ in arms}
for grp in range(GROUPS):
    for name, run in arms:
        run(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(K)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / K)
    print("(c) group %d (%d steps each): " % (grp, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
base = med(ms["hand loop"])
for name, _ in arms:
    x = ms[name]
    print("(c) %-9s median %.3f ms per step (min %.3f, max %.3f) = %.0f blocks/s; against the hand loop %+.2f %%"
          % (name, med(x), min(x), max(x), B * 1e3 / med(x), (med(x) / base - 1) * 100))
