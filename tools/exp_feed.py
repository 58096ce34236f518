"""The input side, measured: what a training batch costs on the host path and on the device feed, and what the
feed's side-stream kernel does to the headline step.

  (a) host     harness/blockio: parse_block -> sample_points -> augment_batch, one thread, ms per batch and per stage (median
               of 10 batches) on THIS machine's CPU;
  (b) kernel   sph3d_feed_assemble by device events, one event pair per launch, augment on / off;
  (c) step     the headline training step (s3dis_config(8192), 16 blocks, graph build + forward + backward + Adam; bench.py's
               loop built from the harness) on two RESIDENT batches used in turn against the same step fed by DeviceFeed on its
               side stream (with the consumer's event handed back after the loss, and without): alternating groups of steps in
               one process, host clock around K steps that end in a device synchronise.  Every group is printed, not only the medians.

The pool: 32 distinct synthetic blocks (harness/synth.py geometry on a 2 cm grid) of 6 000 .. 30 000 rows with random colours,
each listed 8 times (256 pool entries: 16 batches per epoch).
usage: python tools/exp_feed.py [groups] [steps per group]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import blockio, feed, dist as hdist, optim as hoptim, s3dis_net, synth

GROUPS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
K = int(sys.argv[2]) if len(sys.argv) > 2 else 30
B, N, SEED = 16, 8192, 1
dev = torch.device("cuda:0"); _lib.lib()


def med(v):
    return float(np.median(v))


# ---- the pool -------------------------------------------------------------------------------------------------------------------
rng = np.random.RandomState(0)
distinct = []
for k in range(32):
    n = int(rng.randint(6000, 30001))
    xyz, label, inner = synth.s3dis_block(5000 + k, n, voxel=0.02)
    distinct.append(np.concatenate([xyz, rng.rand(n, 3).astype(np.float32), label.reshape(-1, 1).astype(np.float32),
                                    inner.reshape(-1, 1).astype(np.float32)], axis=1))
blocks = distinct * 8
print("pool: %d entries (%d distinct), %d .. %d rows, %.1f MB of rows" % (len(blocks), len(distinct), min(map(len, distinct)),
                                                                          max(map(len, distinct)), sum(map(len, blocks)) * 32 / 1e6))

# ---- (a) the host path ----------------------------------------------------------------------------------------------------------
records = [blockio.encode_block(b[:, 0:3], b[:, 3:6], b[:, 6].astype(np.int32), b[:, 7].astype(np.int32)) for b in distinct]
t_parse, t_sample, t_aug = [], [], []
hrng = np.random.RandomState(1)
for it in range(11):
    pick = hrng.permutation(len(records))[:B]
    t0 = time.perf_counter()
    parsed = [blockio.parse_block(records[i]) for i in pick]
    t1 = time.perf_counter()
    s = [blockio.sample_points(p, N, hrng) for p in parsed]
    x, l, i = np.stack([a[0] for a in s]), np.stack([a[1] for a in s]), np.stack([a[2] for a in s])
    t2 = time.perf_counter()
    blockio.augment_batch(x, l, i, hrng)
    t3 = time.perf_counter()
    if it:                       # (the first batch warms the caches)
        t_parse.append((t1 - t0) * 1e3); t_sample.append((t2 - t1) * 1e3); t_aug.append((t3 - t2) * 1e3)
print("(a) host blockio, one thread, %d x %d, median of 10 batches: parse %.1f + sample %.1f + augment %.1f = %.1f ms per batch"
      % (B, N, med(t_parse), med(t_sample), med(t_aug), med(np.array(t_parse) + np.array(t_sample) + np.array(t_aug))))

# ---- (b) the kernel -------------------------------------------------------------------------------------------------------------
pool = feed.BlockPool.from_blocks(blocks, dev)
ids_all = torch.from_numpy(feed.epoch_order(len(pool), SEED, 0)).to(dev)
out = (torch.empty((B, N, 6), dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
       torch.empty((B, N), dtype=torch.int32, device=dev))
for augment in (True, False):
    for w in range(20):
        feed.assemble(pool.rows, pool.offsets, ids_all[(w % 16) * B:(w % 16 + 1) * B], N, SEED, w, augment, out=out)
    torch.cuda.synchronize()
    pairs = []
    for w in range(200):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        feed.assemble(pool.rows, pool.offsets, ids_all[(w % 16) * B:(w % 16 + 1) * B], N, SEED, 100 + w, augment, out=out)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in pairs])
    # and 200 launches back to back between ONE event pair (the per-launch pairs include the event packets)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for w in range(200):
        feed.assemble(pool.rows, pool.offsets, ids_all[(w % 16) * B:(w % 16 + 1) * B], N, SEED, 300 + w, augment, out=out)
    e1.record()
    torch.cuda.synchronize()
    moved = B * N * (32 + 36) / 1e6
    print("(b) sph3d_feed_assemble %d x %d augment=%d: per launch by event pairs median %.1f us (min %.1f, p90 %.1f); 200 back to back "
          "%.1f us each; %.1f MB read + written per batch" % (B, N, augment, med(us), us.min(), np.percentile(us, 90),
                                                             e0.elapsed_time(e1) * 1e3 / 200, moved))

# ---- (c) the headline step: resident batches against the feed ---------------------------------------------------------------------
model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)
resident = []
for w in range(2):
    resident.append(tuple(t.clone() for t in feed.assemble(pool.rows, pool.offsets, ids_all[w * B:(w + 1) * B], N, SEED, w, True)))
torch.cuda.synchronize()
ready0 = torch.cuda.Event(); ready0.record()
pts, label, inner = resident[0]
model.loss(model(pts, is_training=True)[0], label, inner).backward()           # creates the variables
flat = hdist.FlatGradAllReduce(model.parameters())
opt = hoptim.FlatAdam(flat.flat_param, lr=1e-3, eps=1e-4)


def train(pts, label, inner, ready, after_forward=None):
    pred, _ = model(pts, is_training=True, points_ready=ready)
    loss = model.loss(pred, label, inner)
    if after_forward is not None:        # the batch's last reader (the loss) is issued: its set may be handed back
        after_forward(ready)
    flat.backward(loss)
    flat.all_reduce()
    opt.step()
    return loss


count = [0]


def resident_steps(k):
    for _ in range(k):
        b = resident[count[0] % 2]
        count[0] += 1
        train(b[0], b[1], b[2], ready0)


def fed_steps(the_feed, hand_back):
    def run(k):
        done = 0
        while done < k:
            for pts, label, inner, ready in the_feed:
                train(pts, label, inner, ready, the_feed.done if hand_back else None)
                done += 1
                if done == k:
                    break            # (the epoch is abandoned: the next `for` starts the next one)
    return run


# (ONE feed stream for both fed arms: with the step's three streams that makes four, the number of hardware queues a process opens
# by default — a fifth stream would share a queue with one of the others and serialise behind it)
feed_stream = torch.cuda.Stream(device=dev)
arms = [("resident", resident_steps),
        ("fed+done", fed_steps(feed.DeviceFeed(pool, B, N, SEED, augment=True, stream=feed_stream), True)),
        ("fed", fed_steps(feed.DeviceFeed(pool, B, N, SEED, augment=True, stream=feed_stream), False))]
for name, run in arms:               # priming: allocator pools, the first collections (bench.py: PRIME_STEPS)
    run(16)
torch.cuda.synchronize()
ms = {name: [] for name, _ in arms}
for g in range(GROUPS):
    for name, run in arms:
        run(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(K)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / K)
    print("(c) group %d (%d steps each): " % (g, K) + "  ".join("%s %.3f ms" % (name, ms[name][-1]) for name, _ in arms))
base = med(ms["resident"])
for name, _ in arms:
    v = ms[name]
    print("(c) %-9s median %.3f ms per step (min %.3f, max %.3f) = %.0f blocks/s; against resident %+.2f %%"
          % (name, med(v), min(v), max(v), B * 1e3 / med(v), (med(v) / base - 1) * 100))
