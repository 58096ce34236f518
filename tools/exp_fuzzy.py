"""Isolated timing of the fuzzy spherical kernel (csrc/fuzzy.hip) beside the hard ops in one run: the kernel
builder against spherical_kernel, the fuzzy forward and gradient against depthwise_conv3d and its gradient at the four S3DIS
level shapes (B = 16, the plan's radii, 64 slots, the first layer's C and r = 2 of every level), the GraphPlan build and one
training step with and without config.kernel_fuzzy.
A measurement, not a test (tests/test_gpu_fuzzy.py holds the outputs to the statement).  Device us per call from events around
10 calls after 3 warm-up calls (the transposed graphs are cached: the gradients' times exclude their build, which the plan rows
show); the plan builds and steps as wall-clock ms with a synchronize, median of 9 alternating pairs.
usage: python tools/exp_fuzzy.py [--skip-plans]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sph3d_gcn_amd import tf_buildkernel, tf_conv3d, tf_nnquery  # noqa: E402
from sph3d_gcn_amd.harness import s3dis_net, synth  # noqa: E402

dev = torch.device("cuda:0")
KERNEL = [8, 2, 2]


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


def level(tag, pts, radius, C, r=2):
    idx, cnt, dst = tf_nnquery.build_sphere_neighbor(pts, pts, radius, None, 64)
    hard_k = timed(lambda: tf_buildkernel.spherical_kernel(pts, pts, idx, cnt, dst, radius, kernel=KERNEL))
    fuzzy_k = timed(lambda: tf_buildkernel.fuzzy_spherical_kernel(pts, pts, idx, cnt, dst, radius, kernel=KERNEL))
    bins = tf_buildkernel.spherical_kernel(pts, pts, idx, cnt, dst, radius, kernel=KERNEL)
    fi, fr = tf_buildkernel.fuzzy_spherical_kernel(pts, pts, idx, cnt, dst, radius, kernel=KERNEL)
    B, N = pts.shape[0], pts.shape[1]
    x = torch.randn(B, N, C, device=dev)
    w = torch.randn(33, C, r, device=dev)
    go = torch.randn(B, N, C * r, device=dev)
    hard_f = timed(lambda: tf_conv3d.depthwise_conv3d(x, w, idx, cnt, bins))
    fuzzy_f = timed(lambda: tf_conv3d.fuzzy_depthwise_conv3d(x, w, idx, cnt, fi, fr, kernel=KERNEL))
    hard_g = timed(lambda: tf_conv3d.depthwise_conv3d_grad(x, w, go, idx, cnt, bins))
    fuzzy_g = timed(lambda: tf_conv3d.fuzzy_depthwise_conv3d_grad(x, w, go, idx, cnt, fi, fr, kernel=KERNEL))
    print("%-22s C=%3d r=%d  edges/row %5.1f | builder %7.1f %7.1f | forward %8.1f %8.1f (x%.2f) | gradient %8.1f %8.1f (x%.2f)   us" %
          (tag, C, r, float(cnt.float().mean()), hard_k, fuzzy_k, hard_f, fuzzy_f, fuzzy_f / hard_f, hard_g, fuzzy_g, fuzzy_g / hard_g),
          flush=True)


def step(model, pts, label, inner):
    graphs = s3dis_net.build_graphs(pts, model.config)
    pred, _ = model(pts, is_training=True, graphs=graphs)
    model.loss(pred, label, inner).backward()


def main():
    xyz, label, inner = synth.s3dis_batch(1000, 16, 8192)
    pts = torch.from_numpy(xyz[:, :, :3]).to(dev).contiguous()
    print("== S3DIS level shapes, B = 16: hard | fuzzy")
    for n, radius, C in ((8192, 0.1, 64), (2048, 0.2, 128), (768, 0.4, 256), (384, 0.8, 256)):
        level("16 x %d r=%.1f" % (n, radius), pts[:, :n].contiguous(), radius, C)
    if "--skip-plans" in sys.argv:
        return
    print("== s3dis_config 16 x 8192, ms (median of 9 alternating pairs): hard | config.kernel_fuzzy")
    p = torch.from_numpy(xyz).to(dev)
    lab, inn = torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    cfgs = (s3dis_net.s3dis_config(8192), s3dis_net.s3dis_config(8192))
    cfgs[1].kernel_fuzzy = True
    models = [s3dis_net.SPH3DS3DIS(c, device=dev) for c in cfgs]
    for name, fn in (("GraphPlan build", lambda i: s3dis_net.build_graphs(p, cfgs[i])),
                     ("forward + backward step", lambda i: step(models[i], p, lab, inn))):
        times = {0: [], 1: []}
        for it in range(11):
            for which in (0, 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(which)
                torch.cuda.synchronize()
                if it >= 2:
                    times[which].append((time.perf_counter() - t0) * 1e3)
        print("%-26s %8.3f | %8.3f" % (name, statistics.median(times[0]), statistics.median(times[1])), flush=True)


if __name__ == "__main__":
    main()
