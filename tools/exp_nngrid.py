"""Isolated timing of the fused graph construction (search + bins + transposed counts) on the bench's level shapes.
usage: python tools/exp_nngrid.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sph3d_gcn_amd import _lib, tf_nnquery  # noqa: E402
from sph3d_gcn_amd.harness import synth  # noqa: E402

dev = torch.device("cuda:0")
xyz, _, _ = synth.s3dis_batch(1000, 16, 8192)
pts0 = torch.from_numpy(xyz[:, :, :3]).to(dev).contiguous()
levels = [(8192, 0.1), (2048, 0.2), (768, 0.4), (384, 0.8)]
for n, radius in levels:
    pts = pts0[:, :n].contiguous()
    for _ in range(3):
        r = tf_nnquery.build_sphere_graph(pts, radius, 64, (8, 2, 2), with_transpose=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        r = tf_nnquery.build_sphere_graph(pts, radius, 64, (8, 2, 2), with_transpose=False)
    e1.record()
    torch.cuda.synchronize()
    cnt = r[1].float().mean().item()
    print("N=%5d r=%.1f  %.1f us per call   mean count %.1f  max %d" % (n, radius, e0.elapsed_time(e1) * 100, cnt, int(r[1].max())), flush=True)
    # pooling-style graph: queries = first quarter of the points
    q = pts[:, :n // 4].contiguous()
    for _ in range(3):
        r2 = tf_nnquery.build_sphere_neighbor_counted(pts, q, radius, 64)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
        r2 = tf_nnquery.build_sphere_neighbor_counted(pts, q, radius, 64)
    e1.record()
    torch.cuda.synchronize()
    print("   pooling graph %d -> %d: %.1f us per call (with the transposed graph's finish)  mean count %.1f" % (n, n // 4, e0.elapsed_time(e1) * 100, r2[1].float().mean().item()), flush=True)
