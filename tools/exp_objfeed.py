"""Object-dataset input and evaluation on the device against their numpy statements on the host.

  * the feed: objfeed.assemble at 32 x 2048 (train_recipe "shapenet") from a pool of ShapeNet-sized shapes (2 000 - 3 000 rows),
    device microseconds per call (HIP events around `reps` calls) against the host time of objfeed.assemble_reference +
    apply_reference for the same batch;
  * one evaluation batch: shapeeval.ShapeVoter.run_batch with a trivial model_fn (a [3, C] matrix on the points), wall time per
    batch and per draw (it synchronises once per draw), and sph3d_shape_iou alone in device microseconds, against
    shapeeval.shape_vote_reference on the host replaying the same logits.

    python tools/exp_objfeed.py [--reps 200] [--shapes 256]
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
    ap.add_argument("--shapes", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-point", type=int, default=2048)
    ap.add_argument("--num-cls", type=int, default=50)
    args = ap.parse_args()
    import torch
    from sph3d_gcn_amd import _lib
    from sph3d_gcn_amd.harness import evalvote, objfeed, shapeeval
    dev = torch.device("cuda:0")
    B, N, C = args.batch, args.num_point, args.num_cls
    rng = np.random.RandomState(0)
    sizes = rng.randint(2000, 3001, args.shapes)
    shapes = [objfeed.shape_blocks((rng.rand(n, 3) * 2 - 1).astype(np.float32), rng.randint(0, 4, n)) for n in sizes]
    pool = objfeed.ShapePool(shapes, np.zeros(len(shapes), np.int32), [0], [4], device=dev)
    out = {"batch": B, "num_point": N, "num_cls": C, "shapes": int(args.shapes)}

    # ---- the feed
    ids = rng.permutation(len(shapes))[:B].astype(np.int32)
    ids_dev = torch.from_numpy(ids).to(dev)
    recipe = objfeed.train_recipe(B, "shapenet")
    recipe_dev = torch.from_numpy(recipe).to(dev)
    bufs = (torch.empty((B, N, 3), device=dev), torch.empty((B, N), dtype=torch.int32, device=dev))
    for step in range(10):
        objfeed.assemble(pool.rows, pool.offsets, ids_dev, N, 1, step, recipe_dev, out=bufs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for step in range(args.reps):
        objfeed.assemble(pool.rows, pool.offsets, ids_dev, N, 1, step, recipe_dev, out=bufs)
    e1.record()
    torch.cuda.synchronize()
    out["feed_device_us_per_call"] = e0.elapsed_time(e1) * 1e3 / args.reps
    t0 = time.perf_counter()
    for step in range(3):
        ref = objfeed.assemble_reference(pool.sizes, ids, N, 1, step, recipe)
        objfeed.apply_reference(shapes, ids, ref)
    out["feed_numpy_statement_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / 3

    # ---- one evaluation batch
    w = torch.from_numpy(rng.randn(3, C).astype(np.float32)).to(dev)
    model_fn = lambda points, label, category: points @ w
    eval_ids = evalvote.batch_blocks(len(pool), B, 0)
    cap = int(pool.host_offsets[eval_ids[-1] + 1] - pool.host_offsets[eval_ids[0]])
    voter = shapeeval.ShapeVoter(pool, B, N, C, cap)
    voter.run_batch(model_fn, eval_ids, 0, 0)                                     # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = []
    got = voter.run_batch(model_fn, eval_ids, 0, 0, on_pass=lambda i, q, index, logits: rec.append(logits.cpu().numpy()))
    torch.cuda.synchronize()
    wall_with_copies = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = voter.run_batch(model_fn, eval_ids, 0, 0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out.update(eval_draws=int(got.passes), eval_device_wall_ms_per_batch=wall * 1e3, eval_device_wall_us_per_draw=wall * 1e6 / max(1, got.passes),
               eval_complete=bool(got.complete), eval_instance_miou=float(np.mean(got.shape_iou)))
    # sph3d_shape_iou alone
    plo, pn = pool.part_range(eval_ids, C)
    rng_dev = torch.from_numpy(np.concatenate([plo, pn])).to(dev)
    eids = torch.from_numpy(eval_ids).to(dev)
    inter, pc, gc = (voter.parts[k * B * C:(k + 1) * B * C] for k in range(3))
    call = lambda: _lib.check(_lib.lib().sph3d_shape_iou(
        B, C, len(pool), int(pool.rows.shape[0]), _lib.ptr(pool.rows), _lib.ptr(pool.offsets), _lib.ptr(eids), 0, cap, _lib.ptr(voter.votes),
        _lib.ptr(rng_dev), _lib.ptr(rng_dev[B:]), _lib.ptr(voter.pred), _lib.ptr(inter), _lib.ptr(pc), _lib.ptr(gc),
        _lib.ptr(voter.parts[3 * B * C:]), _lib.ptr(voter.nonfinite), _lib.stream_ptr()))
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    out["shape_iou_device_us_per_call"] = e0.elapsed_time(e1) * 1e3 / args.reps
    label = np.concatenate([s[:, 6] for s in shapes])
    t0 = time.perf_counter()
    want = shapeeval.shape_vote_reference(pool.sizes, label, eval_ids, plo, pn, N, 0, 0, lambda q, index: rec[q], C)
    host = time.perf_counter() - t0
    out.update(eval_numpy_statement_ms_per_batch=host * 1e3, eval_matches_statement=bool(
        want.passes == got.passes and np.array_equal(want.shape_iou, got.shape_iou) and np.array_equal(want.inter, got.inter)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
