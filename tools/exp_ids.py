"""Keyed inverse-density sampling: device time at the plans' shapes beside farthest-point sampling and the torch one-liner
(tf_sample.inverse_density_sample on precomputed weights), and the whole GraphPlan build (forward only) with 'FPS' and 'IDS'.
Median of 20 calls after 5 warm-up calls, each call timed by device events on the current stream.  DESIGN 4.16 holds the numbers.

    python tools/exp_ids.py [--json FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sph3d_gcn_amd import _lib, tf_nnquery, tf_sample
from sph3d_gcn_amd.harness import modelnet_net, s3dis_net, synth

WARMUP, CALLS = 5, 20


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


def room(N):
    """the synthetic room that holds N distinct 3-cm voxels of surface: bench.py's for the 65 536-point blocks"""
    return (6.0, 6.0, 3.0) if N > 16384 else (2.1, 2.1, 3.0)


def cloud(kind, B, N, dev):
    if kind == "modelnet":
        return torch.from_numpy(synth.modelnet_batch(100, B, N)[:, :, :3].copy()).to(dev)
    return torch.from_numpy(synth.s3dis_batch(1000, B, N, extent=room(N))[0][:, :, :3].copy()).to(dev)


def sampler_rows(dev):
    rows = []
    mn = modelnet_net.modelnet_config()
    s3 = s3dis_net.s3dis_config()
    # (kind, B, N, S, radius, K): the S3DIS plan's levels 0 and 1, the 65 536-point plan's level 0, the ModelNet plan's level 0
    shapes = [("s3dis", 16, 8192, 2048, s3.radius[0], s3.nn_uplimit[0]), ("s3dis-l1", 16, 2048, 768, s3.radius[1], s3.nn_uplimit[1]),
              ("scannet", 16, 65536, 16384, s3.radius[0], s3.nn_uplimit[0]),
              ("modelnet", 32, mn.num_input, mn.num_sample[0], mn.radius[0], mn.nn_uplimit[0])]
    for kind, B, N, S, radius, K in shapes:
        if kind == "s3dis-l1":       # the real level-1 input: samples of level 0
            big = cloud("s3dis", B, 8192, dev)
            idx = tf_sample.farthest_point_sample(N, big).long()
            xyz = torch.gather(big, 1, idx.unsqueeze(2).expand(-1, -1, 3)).contiguous()
        else:
            xyz = cloud("modelnet" if kind == "modelnet" else "s3dis", B, N, dev)
        _, cnt, dst = tf_nnquery.build_sphere_neighbor(xyz, xyz, radius, None, K)
        prob = torch.sum(dst, dim=-1) / cnt.float()
        step = [0]

        def keyed():
            step[0] += 1
            return tf_sample.inverse_density_sample_keyed(S, dst, cnt, 1, step[0], 0)

        # interleaved: each sampler's 25 calls follow the others' in the same process, on the same inputs
        row = dict(kind=kind, B=B, N=N, S=S, K=K,
                   ids_keyed_us=median_us(keyed),
                   ids_torch_us=median_us(lambda: tf_sample.inverse_density_sample(S, prob)),
                   ids_torch_with_weights_us=median_us(lambda: tf_sample.inverse_density_sample(
                       S, torch.sum(dst, dim=-1) / cnt.float())),
                   fps_us=median_us(lambda: tf_sample.farthest_point_sample(S, xyz)),
                   ids_keyed_again_us=median_us(keyed))
        rows.append(row)
        print("%-9s B%3d N%6d -> %5d : keyed %8.1f us (again %8.1f) | torch one-liner %8.1f us (+ weights %8.1f) | FPS %9.1f us"
              % (kind, B, N, S, row["ids_keyed_us"], row["ids_keyed_again_us"], row["ids_torch_us"],
                 row["ids_torch_with_weights_us"], row["fps_us"]), flush=True)
    return rows


def plan_rows(dev):
    rows = []
    for name, cfg, B, N in (("s3dis 16x8192", s3dis_net.s3dis_config(8192), 16, 8192),
                            ("scannet 16x65536", s3dis_net.scannet_config(65536), 16, 65536)):
        pts = torch.from_numpy(synth.s3dis_batch(1000, B, N, extent=room(N))[0]).to(dev)
        row = dict(plan=name)
        for method in ("FPS", "IDS", "FPS", "IDS"):
            c = copy.deepcopy(cfg)
            c.sample = method
            step = [0]

            def build():
                step[0] += 1
                with torch.no_grad():
                    plan = s3dis_net.build_graphs(pts, c, sample_key=(1, step[0]))
                torch.cuda.current_stream().synchronize()      # (build_graphs made the main stream wait for every graph)
                return plan

            row.setdefault(method + "_us", []).append(median_us(build))
        rows.append(row)
        print("%-17s GraphPlan build, forward only: FPS %s us | IDS %s us" % (
            name, ", ".join("%.0f" % t for t in row["FPS_us"]), ", ".join("%.0f" % t for t in row["IDS_us"])), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_ids.py measures on the device: no GPU here")
    dev = torch.device("cuda:0")
    _lib.lib()
    out = dict(samplers=sampler_rows(dev), plans=plan_rows(dev))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
