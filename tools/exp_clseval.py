"""The ModelNet40 classification evaluation on the device against its numpy statement and against the host-bound form of the same
loop.  32 x 10 000 from a pool of 256 shapes of 10 000 rows, C = 40, a [3, C] matrix on the per-cloud coordinate
mean as model_fn, 1 and 12 votes.

  * device microseconds per call of sph3d_clsfeed_assemble (plain and augmented), sph3d_cls_vote_accumulate and
    sph3d_cls_vote_finalize: HIP events around `reps` calls, after a warm-up of each;
  * wall time per batch of the device loop (clseval.ClassVoter.run_batch over all 8 batches of the pool, no read inside, one
    synchronise at the end), the loops repeated until the window is at least `--min-seconds`;
  * the wall time of the same loop with a `.cpu()` arg-max per batch — the form this replaces: the same assemble and model_fn,
    a float64 sum in torch, argmax(...).cpu() and the host's counting;
  * host time of the numpy statement for the same work (clseval.assemble_reference + vote_reference, one batch).
The two loops are timed alternately in the same process; each figure is the median of `--rounds` windows, with the spread.

    python tools/exp_clseval.py [--reps 200] [--rounds 5] [--min-seconds 0.5]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--shapes", type=int, default=256)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-cls", type=int, default=40)
    args = ap.parse_args()
    import torch
    from sph3d_gcn_amd import _lib
    from sph3d_gcn_amd.harness import clseval, evalvote, objfeed
    if not torch.cuda.is_available():
        raise SystemExit("exp_clseval: needs the GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    B, N, C, P = args.batch, args.rows, args.num_cls, args.shapes
    rng = np.random.RandomState(0)
    xyz = [(rng.rand(N, 3) * 2 - 1).astype(np.float32) for _ in range(P)]
    category = rng.randint(0, C, P).astype(np.int32)
    pool = objfeed.ShapePool.from_arrays(xyz, list(category), category, device=dev)
    w = torch.from_numpy(rng.randn(3, C).astype(np.float32)).to(dev)
    model_fn = lambda points: points.mean(dim=1) @ w
    out = {"batch": B, "num_point": N, "num_cls": C, "shapes": P}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def device_us(call):
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    # ---- the three entries alone
    l = _lib.lib()
    ids = torch.from_numpy(evalvote.batch_blocks(P, B, 0)).to(dev)
    points = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    recipes = [torch.full((B,), m, dtype=torch.int32, device=dev) for m in (0, clseval.EVAL_AUGMENT)]
    for name, r in zip(("plain", "augmented"), recipes):
        out["assemble_%s_device_us" % name] = device_us(
            lambda: clseval.assemble(pool.rows, pool.offsets, ids, N, 1, 2, r, 1, True, out=points))
    out["assemble_bytes_moved"] = B * N * (32 + 12)                    # a 32-byte row read (one 16-byte load of it), 12 bytes stored
    logits = model_fn(points).contiguous()
    sums = torch.zeros((B, C), dtype=torch.float64, device=dev)
    state = torch.zeros((P + 4 + 2 * C,), dtype=torch.int32, device=dev)
    votes_out = torch.zeros((P, 12, C), dtype=torch.float32, device=dev)
    acc_args = (B, C, _lib.ptr(logits), 1, 12, _lib.ptr(sums), _lib.ptr(ids), _lib.ptr(votes_out), P, _lib.stream_ptr())
    fin_args = (B, C, _lib.ptr(sums), _lib.ptr(ids), _lib.ptr(pool.category_dev), P, _lib.ptr(state), _lib.ptr(state[P:]),
                _lib.ptr(state[P + 4:]), _lib.ptr(state[P + 4 + C:]), _lib.stream_ptr())
    out["accumulate_device_us"] = device_us(lambda: l.sph3d_cls_vote_accumulate(*acc_args))     # (addresses formed once: the
    out["finalize_device_us"] = device_us(lambda: l.sph3d_cls_vote_finalize(*fin_args))         #  window holds only the calls)

    # ---- the loops
    batches = list(range((P + B - 1) // B))

    def device_loop(V):
        voter = clseval.ClassVoter(pool, B, N, C, V, swap_yz=True, seed=1)
        for i in voter.batches:
            voter.run_batch(model_fn, i)
        return voter.result()

    def host_bound_loop(V):
        """the reference's loop shape on the same device work: per batch a float64 sum, then argmax(...).cpu() and the host's counts"""
        seen = correct = 0
        class_seen, class_correct = np.zeros((C,), np.int64), np.zeros((C,), np.int64)
        pred = np.full((P,), -1, np.int32)
        for i in batches:
            s = evalvote.batch_blocks(P, B, i)
            ids_i = torch.from_numpy(s).to(dev)
            total = torch.zeros((len(s), C), dtype=torch.float64, device=dev)
            for v in range(V):
                pts = clseval.assemble(pool.rows, pool.offsets, ids_i, N, 1, evalvote.pass_step(i, v), recipes[min(v, 1)][:len(s)], 1,
                                       True, out=points[:len(s)])
                total += model_fn(pts)
            p = torch.argmax(total, 1).cpu().numpy()
            pred[s] = p
            label = category[s]
            seen += len(s)
            correct += int((p == label).sum())
            np.add.at(class_seen, label, 1)
            np.add.at(class_correct, label[p == label], 1)
        return pred, seen, correct

    def window(fn, V):
        fn(V)                                                          # warm
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            fn(V)                                                      # (both end in a device-to-host read: the work is done)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= args.min_seconds:
                return dt * 1e3 / (n * len(batches))

    for V in (1, 12):
        dev_ms, host_ms = [], []
        for _ in range(args.rounds):                                   # alternating, in one process
            dev_ms.append(window(device_loop, V))
            host_ms.append(window(host_bound_loop, V))
        res, (pred, seen, correct) = device_loop(V), host_bound_loop(V)
        out["votes_%d" % V] = {
            "device_loop_ms_per_batch": float(np.median(dev_ms)), "device_loop_ms_min_max": [min(dev_ms), max(dev_ms)],
            "cpu_argmax_loop_ms_per_batch": float(np.median(host_ms)), "cpu_argmax_loop_ms_min_max": [min(host_ms), max(host_ms)],
            "same_predictions": bool(np.array_equal(res.pred, pred) and res.seen == seen and res.correct == correct),
            "accuracy": res.accuracy}

    # ---- the numpy statement of one batch, 12 votes
    rows_xyz = np.concatenate(xyz)
    s = evalvote.batch_blocks(P, B, 0)
    wh = w.cpu().numpy()
    t0 = time.perf_counter()
    votes = []
    for v in range(12):
        ref = clseval.assemble_reference(pool.sizes, rows_xyz, s, N, 1, evalvote.pass_step(0, v), clseval.vote_recipe(v), 1, 1)
        votes.append((ref.points.mean(axis=1) @ wh).astype(np.float32))
    clseval.vote_reference(votes, category[s], C)
    out["numpy_statement_ms_per_batch_12_votes"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
