"""What the float32 matmul precision levels of the pointwise products cost and give.

  products: the 13 S3DIS product shapes x NN / NT / TN x the levels — HIP-event time of single calls, the levels alternating inside one
            process: per group the median of 10 calls, four groups; reported: the median of the group medians and their spread
            (min .. max), the 13-shape sums, and the error / summed term magnitudes each level reaches against float64;
  step    : the Trainer step on s3dis_config(8192), 16 blocks, at the levels: 20 steps per group, alternating, four groups.

usage: python tools/exp_gemm_precision.py [--levels highest,high,medium] [--part products|step|all] [--json FILE]
A tree without the levels (the parent commit, for the A/B of the default path) runs with --levels highest."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sph3d_gcn_amd as pkg  # noqa: E402
from sph3d_gcn_amd import tf_gemm  # noqa: E402

# tests/test_gpu_gemm_split.py: SHAPES[:13]
SHAPES = [(131072, 128, 128), (131072, 256, 128), (32768, 256, 256), (32768, 512, 256), (12288, 512, 256), (6144, 512, 512),
          (6144, 1024, 512), (2048, 1024, 512), (6144, 2048, 256), (12288, 1024, 256), (32768, 1024, 128), (4096, 64, 128),
          (2048, 144, 64)]
GROUPS, CALLS, STEPS = 4, 10, 20


def level_scope(level):
    scope = getattr(pkg, "float32_matmul_precision", None)
    if scope is None:
        assert level == "highest", "this tree has one level"
        return contextlib.nullcontext()
    return scope(level)


def time_calls(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def products(levels, dev):
    out = {"shapes": [], "sum_us": {}, "sum_spread_us": {}}
    sums = {(lv, g): 0.0 for lv in levels for g in range(GROUPS)}
    for R, Ci, Co in SHAPES:
        g = torch.Generator(device=dev).manual_seed(R + Ci)
        x = torch.randn(R, Ci, device=dev, generator=g) * torch.exp2(torch.randint(-6, 6, (R, Ci), device=dev, generator=g).float())
        w = torch.randn(Ci, Co, device=dev, generator=g) / Ci ** 0.5
        dy = torch.randn(R, Co, device=dev, generator=g) * torch.exp2(torch.randint(-6, 6, (R, Co), device=dev, generator=g).float())
        calls = {"NN": lambda: tf_gemm._pointwise_gemm_impl(x, w, False), "NT": lambda: tf_gemm._pointwise_gemm_impl(dy, w, True),
                 "TN": lambda: tf_gemm._pointwise_gemm_tn_impl(x, dy)}
        xd, wd, dyd = x.double(), w.double(), dy.double()
        want = {"NN": (xd @ wd, xd.abs() @ wd.abs()), "NT": (dyd @ wd.t(), dyd.abs() @ wd.abs().t()), "TN": (xd.t() @ dyd, xd.abs().t() @ dyd.abs())}
        del xd, wd, dyd
        row = {"shape": [R, Ci, Co]}
        for name, fn in calls.items():
            err, med = {}, {lv: [] for lv in levels}
            for lv in levels:
                with level_scope(lv):
                    err[lv] = float(((fn().double() - want[name][0]).abs() / want[name][1]).max())
                    fn()
            for grp in range(GROUPS):
                for lv in levels:
                    with level_scope(lv):
                        t = time_calls(fn, CALLS) * 1e3
                    med[lv].append(t)
                    sums[(lv, grp)] += t
            row[name] = {lv: {"us": round(statistics.median(med[lv]), 2), "min_us": round(min(med[lv]), 2), "max_us": round(max(med[lv]), 2),
                              "error_over_mag": err[lv]} for lv in levels}
            print("R%6d %4d->%4d %s  " % (R, Ci, Co, name) + "   ".join(
                "%s %7.1f us (%.1f..%.1f) err %.2e" % (lv, row[name][lv]["us"], row[name][lv]["min_us"], row[name][lv]["max_us"], err[lv])
                for lv in levels), flush=True)
        del want
        out["shapes"].append(row)
    for lv in levels:
        per_group = [sums[(lv, grp)] for grp in range(GROUPS)]
        out["sum_us"][lv] = round(statistics.median(per_group), 1)
        out["sum_spread_us"][lv] = [round(min(per_group), 1), round(max(per_group), 1)]
        for name in ("NN", "NT", "TN"):
            out.setdefault("sum_by_product_us", {}).setdefault(name, {})[lv] = round(sum(r[name][lv]["us"] for r in out["shapes"]), 1)
        print("13 shapes, NN + NT + TN, %s: %.1f us (groups %.1f .. %.1f)" % (lv, out["sum_us"][lv], min(per_group), max(per_group)), flush=True)
    return out


def step(levels, dev):
    from sph3d_gcn_amd.harness import optim, s3dis_net, synth, train
    n_pts, blocks = 8192, 16
    items = []
    for which in range(2):
        xyz, label, inner = synth.s3dis_batch(1000 + which * 64 * blocks, blocks, n_pts)
        items.append((torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev), None))
    model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(n_pts), device=dev)
    tr = train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, blocks), 13,
                       prime=items[0][:3], seed=5, log=lambda s: None)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            tr.train_step(items[i % 2])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    run(25)                                   # one-off host stalls of a fresh process (allocator pools, the first full collection)
    ms = {lv: [] for lv in levels}
    for grp in range(GROUPS):
        for lv in levels:
            with level_scope(lv):
                run(3)
                ms[lv].append(run(STEPS))
    out = {}
    for lv in levels:
        out[lv] = {"ms_per_step": round(statistics.median(ms[lv]), 3), "groups": [round(v, 3) for v in ms[lv]]}
        print("step, %s: %.3f ms (groups %s)" % (lv, out[lv]["ms_per_step"], " ".join("%.3f" % v for v in ms[lv])), flush=True)
    r = tr.metrics.read()
    out["mean_loss"] = r.mean_loss
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="highest,high,medium")
    ap.add_argument("--part", choices=("products", "step", "all"), default="all")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    levels = args.levels.split(",")
    dev = torch.device("cuda:0")
    res = {"levels": levels}
    if args.part in ("products", "all"):
        res["products"] = products(levels, dev)
    if args.part in ("step", "all"):
        res["step"] = step(levels, dev)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
