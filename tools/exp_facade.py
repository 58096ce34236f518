"""RueMonge2014 facade input and evaluation pass on the device against the S3DIS feed and the numpy statement.

  * the feed: facadefeed.assemble at 16 x 8192 (train_recipe(16)) from a pool of about 30 facade splits of 100 000 - 400 000 rows,
    device microseconds per call (HIP events around `reps` calls after a warm-up), with the bytes per point it reads (48) and
    writes (40, 44 with the index);
  * feed.assemble at 16 x 8192 on an S3DIS-sized pool (blocks of 8 000 - 20 000 rows) in the same run, for comparison;
  * the host time of facadefeed.assemble_reference + apply_reference for the same batch;
  * one evaluation pass at that size: facadefeed.assemble (EVAL_AUGMENT, with the index) + sph3d_vote_accumulate (7 classes,
    min_votes 11) on fixed logits, device microseconds per pass.

    python tools/exp_facade.py [--reps 200] [--facades 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(call, reps, warm=20):
    import torch
    for k in range(warm):
        call(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in range(reps):
        call(warm + k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--facades", type=int, default=30)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--num-point", type=int, default=8192)
    args = ap.parse_args()
    import torch
    from sph3d_gcn_amd import _lib
    from sph3d_gcn_amd.harness import evalvote, facadeeval, facadefeed, feed
    dev = torch.device("cuda:0")
    B, N, C = args.batch, args.num_point, facadeeval.NUM_CLASSES
    rng = np.random.RandomState(0)
    sizes = rng.randint(100000, 400001, args.facades)
    blocks, normals = [], []
    for n in sizes:
        rows, nrm = np.zeros((n, 8), np.float32), np.zeros((n, 4), np.float32)
        rows[:, 0:3] = (rng.rand(n, 3) - [0.5, 0.5, 0.0]) * [12.0, 3.0, 9.0]
        rows[:, 3:6] = rng.rand(n, 3) * 2 - 1
        rows[:, 6], rows[:, 7] = rng.randint(0, C, n), 1.0
        v = rng.randn(n, 3)
        nrm[:, 0:3] = v / np.linalg.norm(v, axis=1, keepdims=True)
        blocks.append(rows)
        normals.append(nrm)
    pool = facadefeed.FacadePool(blocks, normals, device=dev)
    out = {"batch": B, "num_point": N, "facades": int(args.facades), "pool_rows": int(sizes.sum()),
           "bytes_read_per_point": 48, "bytes_written_per_point": 40, "bytes_written_per_point_with_index": 44}

    # ---- the facade feed
    ids = np.arange(B, dtype=np.int32) % len(pool)
    ids_dev = torch.from_numpy(ids).to(dev)
    recipe = facadefeed.train_recipe(B)
    recipe_dev = torch.from_numpy(recipe).to(dev)
    bufs = (torch.empty((B, N, 9), device=dev), torch.empty((B, N), dtype=torch.int32, device=dev))
    out["facadefeed_device_us_per_call"] = _timed(
        lambda k: facadefeed.assemble(pool.rows, pool.normals, pool.offsets, ids_dev, N, 1, k, recipe_dev, out=bufs), args.reps)
    t0 = time.perf_counter()
    for step in range(3):
        ref = facadefeed.assemble_reference(pool.sizes, ids, N, 1, step, recipe)
        facadefeed.apply_reference(blocks, normals, ids, ref)
    out["facadefeed_numpy_statement_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / 3

    # ---- the S3DIS feed on an S3DIS-sized pool, same run
    s_sizes = rng.randint(8000, 20001, 512)
    s_blocks = []
    for n in s_sizes:
        b = rng.rand(n, 8).astype(np.float32)
        b[:, 6], b[:, 7] = rng.randint(0, 13, n), rng.randint(0, 2, n)
        s_blocks.append(b)
    s_pool = feed.BlockPool(s_blocks, dev)
    s_ids = torch.from_numpy(rng.permutation(len(s_pool))[:B].astype(np.int32)).to(dev)
    s_bufs = (torch.empty((B, N, 6), device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
              torch.empty((B, N), dtype=torch.int32, device=dev))
    out["s3dis_feed_device_us_per_call"] = _timed(
        lambda k: feed.assemble(s_pool.rows, s_pool.offsets, s_ids, N, 1, k, True, out=s_bufs), args.reps)
    out["facadefeed_over_s3dis_feed"] = out["facadefeed_device_us_per_call"] / out["s3dis_feed_device_us_per_call"]

    # ---- one evaluation pass: the augmented draw with its index + the vote of fixed logits
    eval_ids = evalvote.batch_blocks(len(pool), B, 0)
    base, cap = int(pool.host_offsets[eval_ids[0]]), int(pool.host_offsets[eval_ids[-1] + 1] - pool.host_offsets[eval_ids[0]])
    voter = facadeeval.FacadeVoter(pool, B, N, C, cap)
    eids = torch.from_numpy(eval_ids).to(dev)
    logits = torch.from_numpy(rng.randn(B, N, C).astype(np.float32)).to(dev)
    l = _lib.lib()
    common = (len(pool), int(pool.rows.shape[0]), _lib.ptr(pool.rows), _lib.ptr(pool.offsets), _lib.ptr(eids), base, cap)
    vbufs = (_lib.ptr(voter.votes), _lib.ptr(voter.count), _lib.ptr(voter.covered), _lib.ptr(voter.inner_size),
             _lib.ptr(voter.remaining), _lib.ptr(voter.ws), voter.ws_bytes)
    _lib.check(l.sph3d_vote_begin(B, C, *common, *vbufs, _lib.stream_ptr()))

    def one_pass(k):
        _p, _l, index = facadefeed.assemble(pool.rows, pool.normals, pool.offsets, eids, N, 0, evalvote.pass_step(0, k), voter.recipe,
                                            out=voter.out, want_index=True)
        _lib.check(l.sph3d_vote_accumulate(B, N, C, *common, k, _lib.ptr(index), _lib.ptr(logits), voter.min_votes, *vbufs,
                                           _lib.stream_ptr()))
    out["eval_pass_device_us"] = _timed(one_pass, args.reps)
    out["eval_rows"] = cap
    print(json.dumps(out))


if __name__ == "__main__":
    main()
