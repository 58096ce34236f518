"""The ScanNet input side on the device against its numpy statement on the host, at 16 x 8192 from a pool that is
larger than the L2 (default: 512 blocks of 8 192 - 16 384 rows, about 200 MB); every timed call takes other blocks of the pool.

  * feed.assemble (the S3DIS recipe), for comparison;
  * the one-view training launch: scannet.assemble under train_recipe;
  * the three-view launch under EVAL_VIEWS against three one-view launches with the same masks;
  * one evaluation draw: ScanNetVoter.run_batch with a trivial model_fn (a [6, C] matrix on the points) — one assemble, three
    products, three votes and the loop's one host synchronisation — wall time per draw;
  * scannet.assemble_reference + apply_reference on the host for one batch of three views.
Device times are HIP events around `reps` calls, in microseconds per call.

    python tools/exp_scannet.py [--reps 200] [--blocks 512]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--num-point", type=int, default=8192)
    ap.add_argument("--draws", type=int, default=20)
    args = ap.parse_args()
    import torch
    from sph3d_gcn_amd.harness import feed, scannet
    dev = torch.device("cuda:0")
    B, N, C, V = args.batch, args.num_point, scannet.NUM_CLASSES, len(scannet.EVAL_VIEWS)
    rng = np.random.RandomState(0)
    sizes = rng.randint(N, 2 * N + 1, args.blocks)
    blocks = []
    for n in sizes:
        blk = rng.rand(n, 8).astype(np.float32)
        blk[:, 6], blk[:, 7] = rng.randint(0, C, n), rng.rand(n) < 0.7
        blocks.append(blk)
    pool = feed.BlockPool(blocks, dev)
    out = {"batch": B, "num_point": N, "blocks": int(args.blocks), "pool_mb": float(pool.rows.numel() * 4 / 2 ** 20), "reps": args.reps}
    table = torch.from_numpy(np.stack([rng.permutation(args.blocks)[:B] for _ in range(args.reps + 10)]).astype(np.int32)).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        for k in range(10):
            call(args.reps + k)
        torch.cuda.synchronize()
        e0.record()
        for k in range(args.reps):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    one = (torch.empty((B, N, 6), device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
           torch.empty((B, N), dtype=torch.int32, device=dev))
    three = (torch.empty((V, B, N, 6), device=dev),) + one[1:]
    train_dev = torch.from_numpy(scannet.train_recipe(B)).to(dev)
    views_host = scannet.eval_recipes(scannet.EVAL_VIEWS, B)
    views_dev = torch.from_numpy(views_host).to(dev)
    out["s3dis_feed_us"] = timed(lambda k: feed.assemble(pool.rows, pool.offsets, table[k], N, 1, k, True, out=one))
    out["train_one_view_us"] = timed(lambda k: scannet.assemble(pool.rows, pool.offsets, table[k], N, 1, k, train_dev, out=one))
    out["eval_three_views_us"] = timed(lambda k: scannet.assemble(pool.rows, pool.offsets, table[k], N, 1, k, views_dev, out=three))

    def three_launches(k):
        for v in range(V):
            scannet.assemble(pool.rows, pool.offsets, table[k], N, 1, k, views_dev[v], out=one)
    out["three_one_view_launches_us"] = timed(three_launches)

    # ---- one evaluation draw
    w = torch.from_numpy(rng.randn(6, C).astype(np.float32)).to(dev)
    model_fn = lambda points, label, inner: points @ w
    ids = np.arange(B, dtype=np.int32)
    voter = scannet.ScanNetVoter(pool, B, N, C, int(pool.host_offsets[B]))
    voter.run_batch(model_fn, ids, 0, 0, max_passes=3)                       # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = voter.run_batch(model_fn, ids, 0, 0, max_passes=args.draws)
    torch.cuda.synchronize()
    out.update(eval_draws=int(got.passes), eval_wall_us_per_draw=(time.perf_counter() - t0) * 1e6 / max(1, got.passes))

    # ---- the statement on the host
    host_ids = table[0].cpu().numpy()
    t0 = time.perf_counter()
    ref = scannet.assemble_reference(pool.sizes, host_ids, N, 1, 0, views_host)
    scannet.apply_reference(blocks, host_ids, ref)
    out["numpy_statement_ms_per_batch"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
