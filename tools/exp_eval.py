"""The overlap-voting evaluation, measured: what a pass costs with the votes on the device (harness/evalvote.py,
csrc/vote.hip) and with the reference's host form (every pass's logits copied back, numpy scatter).

  (a) device time per pass of the three parts — sph3d_feed_assemble, the forward pass (inference mode), sph3d_vote_accumulate —
      and per batch of sph3d_vote_begin / _finalize: event pairs (the library's per-call timing for the C entries, one pair
      around the forward on the main stream, which has waited for the plan's side streams when the logits are issued);
  (b) wall time per pass of evalvote.evaluate, host clock around the whole evaluation, nothing else timed in that run;
  (c) the same loop with the host form of the voting: index and logits copied to the host after every pass, evalvote.vote_update
      and the coverage count in numpy — the reference's loop with this project's draws and network.

The pool: 32 synthetic blocks (harness/synth.py geometry on a 2 cm grid) of 6 000 .. 30 000 rows with random colours: two batches
of 16 at 8192 points, the full S3DIS plan.
usage: python tools/exp_eval.py [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import evalvote, feed, s3dis_net, synth

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B, N, C, SEED = 16, 8192, 13, 1
dev = torch.device("cuda:0"); _lib.lib()


def med(v):
    return float(np.median(v))


rng = np.random.RandomState(0)
blocks = []
for k in range(32):
    n = int(rng.randint(6000, 30001))
    xyz, label, inner = synth.s3dis_block(5000 + k, n, voxel=0.02)
    blocks.append(np.concatenate([xyz, rng.rand(n, 3).astype(np.float32), label.reshape(-1, 1).astype(np.float32),
                                  inner.reshape(-1, 1).astype(np.float32)], axis=1))
pool = feed.BlockPool.from_blocks(blocks, dev)
print("pool: %d blocks of %d .. %d rows, %d inner rows of %d" % (len(blocks), min(map(len, blocks)), max(map(len, blocks)),
                                                               int(sum((b[:, 7] == 1).sum() for b in blocks)), sum(map(len, blocks))))

model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(N), device=dev)


def net(points, label, inner):
    return model(points, is_training=False)[0]


# priming: the variables, the allocator's pools, the plan's arenas
prime = evalvote.evaluate(net, pool, B, N, SEED, max_passes=4)
torch.cuda.synchronize()
print("primed: %s passes (max_passes=4), complete=%s" % (prime.passes, prime.complete))

# ---- (a) device time of the parts --------------------------------------------------------------------------------------------------
fwd_pairs = []


def timed_net(points, label, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = net(points, label, inner)
    e1.record()
    fwd_pairs.append((e0, e1))
    return out


_lib.timing_start()
res_a = evalvote.evaluate(timed_net, pool, B, N, SEED)
calls = _lib.timing_stop()
torch.cuda.synchronize()
by_name = {}
for name, _args, e0, e1 in calls:
    by_name.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
fwd = np.array([a.elapsed_time(b) * 1e3 for a, b in fwd_pairs])
n_pass = sum(res_a.passes)
print("(a) %d passes in %d batches %s, complete=%s" % (n_pass, len(res_a.passes), res_a.passes, res_a.complete))
for name in ("sph3d_feed_assemble", "sph3d_vote_accumulate", "sph3d_vote_begin", "sph3d_vote_finalize"):
    v = np.array(by_name[name])
    print("(a) %-22s %4d calls: median %.1f us (min %.1f, p90 %.1f)" % (name, len(v), med(v), v.min(), np.percentile(v, 90)))
print("(a) forward (inference)    %4d calls: median %.1f us (min %.1f, p90 %.1f) [timed with every C entry inside it bracketed by "
      "events: an upper bound]" % (len(fwd), med(fwd), fwd.min(), np.percentile(fwd, 90)))
vote_per_pass = med(by_name["sph3d_vote_accumulate"]) + (med(by_name["sph3d_vote_begin"]) + med(by_name["sph3d_vote_finalize"])) * len(res_a.passes) / n_pass
print("(a) per pass: vote + (begin + finalize) / passes = %.1f us against assemble + forward = %.1f us"
      % (vote_per_pass, med(by_name["sph3d_feed_assemble"]) + med(fwd)))


# ---- (c)'s loop: the reference's host form --------------------------------------------------------------------------------------------
def evaluate_host(model_fn):
    """-> confusion, passes per batch; t_copy, t_numpy: host seconds spent in the copies and in numpy"""
    confusion, passes_all, t_copy, t_numpy = np.zeros((C, C), np.int64), [], 0.0, 0.0
    out = (torch.empty((B, N, 6), dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
           torch.empty((B, N), dtype=torch.int32, device=dev))
    for i in range(feed.batches_per_epoch(len(pool), B)):
        ids = evalvote.batch_blocks(len(pool), B, i)
        ids_dev = torch.from_numpy(ids).to(dev)
        mine = [blocks[k] for k in ids]
        votes = [np.zeros((len(b), C), np.float32) for b in mine]
        count = [np.zeros((len(b),), np.int32) for b in mine]
        is_in = [b[:, 7] == 1 for b in mine]
        inner_size = np.array([m.sum() for m in is_in])
        covered = np.zeros(len(mine), np.int64)
        p = 0
        while (covered < inner_size).any() and p < evalvote.MAX_PASSES:
            points, label, inner, index = feed.assemble(pool.rows, pool.offsets, ids_dev, N, SEED, evalvote.pass_step(i, p), False,
                                                        out=tuple(t[:len(ids)] for t in out), want_index=True)
            with torch.no_grad():
                logits = model_fn(points, label, inner)
            t0 = time.perf_counter()
            h_logits, h_index = logits.cpu().numpy(), index.cpu().numpy()
            t1 = time.perf_counter()
            for k in range(len(mine)):
                evalvote.vote_update(votes[k], count[k], h_index[k], h_logits[k])
                covered[k] = np.sum(count[k][is_in[k]] >= 1)
            t_copy, t_numpy = t_copy + (t1 - t0), t_numpy + (time.perf_counter() - t1)
            p += 1
        t0 = time.perf_counter()
        for k, b in enumerate(mine):
            pr = np.argmax(votes[k], axis=1)
            np.add.at(confusion, (b[is_in[k], 6].astype(np.int64), pr[is_in[k]]), 1)
        t_numpy += time.perf_counter() - t0
        passes_all.append(p)
    return confusion, passes_all, t_copy, t_numpy


evaluate_host(net)          # (priming of this loop's allocations)
torch.cuda.synchronize()

# ---- (b), (c): wall time per pass, the two forms in turn ------------------------------------------------------------------------------
w_dev, w_host = [], []
for r in range(REPEATS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evalvote.evaluate(net, pool, B, N, SEED)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    conf_h, passes_h, t_copy, t_numpy = evaluate_host(net)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    w_dev.append((t1 - t0) * 1e3 / sum(res.passes))
    w_host.append((t2 - t1) * 1e3 / sum(passes_h))
    print("repeat %d: (b) device form %.3f ms per pass (%d passes, mIoU %.4f, complete=%s)   (c) host form %.3f ms per pass (%d passes; "
          "of it copies %.3f ms, numpy %.3f ms per pass); same passes: %s, same confusion matrix: %s"
          % (r, w_dev[-1], sum(res.passes), res.miou, res.complete, w_host[-1], sum(passes_h), t_copy * 1e3 / sum(passes_h),
             t_numpy * 1e3 / sum(passes_h), res.passes == passes_h, bool(np.array_equal(res.confusion, conf_h))))
print("(b) device form: median %.3f ms per pass   (c) host form: median %.3f ms per pass   host / device = %.2f"
      % (med(w_dev), med(w_host), med(w_host) / med(w_dev)))
