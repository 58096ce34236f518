"""Isolated timing of the exact k-nearest-neighbour search (tf_nnquery.build_nearest_neighbor; csrc/knn.hip) in both forced launch
forms, beside the sphere search at the same shapes and torch.cdist + topk as the framework baseline, in one run; a sweep over N for
the scan / grid crossover of AUTO; and the GraphPlan build with config.unpool_k = 3 against the same build without it, alternating.
A measurement, not a test (tests/test_gpu_knn.py holds the outputs to the statement).  Device us per call from events around 10
calls after 3 warm-up calls; the plan builds as wall-clock ms with a synchronize, median of 9 alternating pairs.
usage: python tools/exp_knn.py [--skip-plans]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sph3d_gcn_amd import tf_nnquery  # noqa: E402
from sph3d_gcn_amd.harness import s3dis_net, synth  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def cdist_topk(db, q, k):
    return torch.topk(torch.cdist(q, db), min(k, db.shape[1]), dim=2, largest=False)


def row(tag, db, q, k, radius, nnsample, baseline=True):
    scan = timed(lambda: tf_nnquery.build_nearest_neighbor(db, q, k, mode=tf_nnquery.KNN_SCAN))
    grid = timed(lambda: tf_nnquery.build_nearest_neighbor(db, q, k, mode=tf_nnquery.KNN_GRID))
    sphere = timed(lambda: tf_nnquery.build_sphere_neighbor(db, q, radius, None, nnsample)) if radius else float("nan")
    base = float("nan")
    if baseline:
        try:
            base = timed(lambda: cdist_topk(db, q, k), reps=5, warm=2)
        except RuntimeError as e:          # (the [M, N] distance matrix did not fit)
            print("cdist + topk at %s: %s" % (tag, str(e).splitlines()[0]))
    print("%-34s k=%2d  scan %9.1f  grid %9.1f  sphere(r=%.2f, K=%d) %9.1f  cdist+topk %9.1f   us" %
          (tag, k, scan, grid, radius or 0, nnsample, sphere, base), flush=True)


def main():
    xyz, _, _ = synth.s3dis_batch(1000, 16, 8192)
    pts = torch.from_numpy(xyz[:, :, :3]).to(dev).contiguous()
    print("== decoder shapes (B = 16, k = 3; the sphere search with the S3DIS plan's radius and 64 slots)")
    for (n, m), radius in zip(((2048, 8192), (768, 2048), (384, 768), (128, 384)), (0.1, 0.2, 0.4, 0.8)):
        row("16 x %d -> %d" % (n, m), pts[:, :n].contiguous(), pts[:, :m].contiguous(), 3, radius, 64)
    print("== search shapes")
    for k in (16, 64):
        row("16 x 8192 -> 8192", pts, pts, k, 0.1, 64)
    big = torch.from_numpy(synth.s3dis_batch(1001, 1, 65536)[0][:, :, :3]).to(dev).contiguous()
    row("1 x 65536 -> 65536", big, big, 16, 0.05, 16)
    print("== crossover sweep (B = 16, M = N and M = 4 N)")
    for n in (256, 512, 1024, 1536, 2048, 4096):
        for m in (n, min(4 * n, 8192)):
            for k in (3, 16):
                row("16 x %d -> %d" % (n, m), pts[:, :n].contiguous(), pts[:, :m].contiguous(), k, None, 0, baseline=False)
    if "--skip-plans" in sys.argv:
        return
    print("== GraphPlan build, ms (median of 9 alternating pairs): sphere un-pooling graphs | unpool_k = 3")
    for name, cfg, batch in (("small_config 2 x 1024", s3dis_net.small_config(1024), synth.s3dis_batch(0, 2, 1024)[0]),
                             ("s3dis_config 16 x 8192", s3dis_net.s3dis_config(8192), xyz)):
        p = torch.from_numpy(batch).to(dev)
        cfg_k = s3dis_net.small_config(1024) if "small" in name else s3dis_net.s3dis_config(8192)
        cfg_k.unpool_k = 3
        times = {0: [], 1: []}
        for it in range(11):
            for which, c in ((0, cfg), (1, cfg_k)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s3dis_net.build_graphs(p, c)
                torch.cuda.synchronize()
                if it >= 2:
                    times[which].append((time.perf_counter() - t0) * 1e3)
        print("%-26s %8.3f | %8.3f" % (name, statistics.median(times[0]), statistics.median(times[1])), flush=True)


if __name__ == "__main__":
    main()
