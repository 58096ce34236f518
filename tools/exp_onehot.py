"""The category-conditioned logits layer of the one-hot ShapeNet model: fused (tf_gemm.linear_concat2_onehot,
csrc/condlogits.hip) against the literal concatenation path of the same commit, at the training shape.

  B = 32 clouds x P = 2048 points, K1 = K2 = 64, N = 50 parts, T = 16 categories, no bias (the reference's config)

Device microseconds per call, HIP events around `reps` calls after `warmup` calls, for
  * forward: s3g_util.pointwise_conv3d_onehot with FUSE_LOGITS_ONEHOT True / False (literal: the one-hot tile, the [R, 144]
    concatenation and sph3d_pointwise_gemm);
  * backward: torch.autograd.grad of that output with respect to both inputs and the weights (literal: the two products on the
    concatenated operand and the slice copies back);
  * step: forward and backward of the layer, one after the other, as a training step runs them;
  * cond_grad: sph3d_pointwise_gemm_cond_grad alone (the literal form has no such call: its category rows come out of the
    weight-gradient product).
The two forms alternate in `rounds` rounds inside one process; the median over the rounds and the spread (min .. max) are
reported, and the two forms' outputs are compared first.  One JSON line.

    python tools/exp_onehot.py [--reps 200] [--warmup 20] [--rounds 5] [--bias]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-point", type=int, default=2048)
    ap.add_argument("--mlp", type=int, default=64)
    ap.add_argument("--num-cls", type=int, default=50)
    ap.add_argument("--categories", type=int, default=16)
    ap.add_argument("--bias", action="store_true")
    args = ap.parse_args()
    if args.reps < 100:
        raise SystemExit("at least 100 timed calls")
    import torch
    from sph3d_gcn_amd import _lib, tf_gemm
    from sph3d_gcn_amd import sph3gcn_util as s3g_util
    if not torch.cuda.is_available():
        raise SystemExit("exp_onehot.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, P, K, N, T = args.batch, args.num_point, args.mlp, args.num_cls, args.categories
    if not tf_gemm.cond_supported(B, P, K, K, N, T):
        raise SystemExit("the kernel does not cover this shape")
    rng = np.random.RandomState(0)
    a = torch.from_numpy(rng.randn(B, P, K).astype(np.float32)).to(dev).requires_grad_(True)
    b = torch.from_numpy(rng.randn(B, P, K).astype(np.float32)).to(dev).requires_grad_(True)
    cat = torch.from_numpy(rng.randint(0, T, B).astype(np.int32)).to(dev)
    dy = torch.from_numpy(rng.randn(B, P, N).astype(np.float32)).to(dev)
    store = s3g_util.VariableStore(device=dev, seed=1)

    def layer(fused):
        s3g_util.FUSE_LOGITS_ONEHOT = fused
        with s3g_util.variable_store(store):
            return s3g_util.pointwise_conv3d_onehot(a, b, cat, T, N, 'logits', activation_fn=None, with_bn=False, with_bias=args.bias)

    layer(True)
    wrt = [a, b] + [p for p in store.parameters()]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    # the two forms compute the same thing (fp32 sums in another order)
    yf, yl = layer(True), layer(False)
    gf, gl = torch.autograd.grad(yf, wrt, dy), torch.autograd.grad(yl, wrt, dy)
    out = {"B": B, "P": P, "K1": K, "K2": K, "N": N, "T": T, "bias": bool(args.bias), "reps": args.reps, "warmup": args.warmup,
           "rounds": args.rounds,
           "max_abs_diff_forward": float((yf - yl).abs().max()),
           "max_rel_diff_grads": max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(gf, gl))}

    l = _lib.lib()
    wsb = l.sph3d_pointwise_gemm_cond_grad_workspace(B, P, N, T)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    dt = torch.empty((T, N), device=dev)
    dy2 = dy.reshape(B * P, N)
    cond_grad = lambda: _lib.check(l.sph3d_pointwise_gemm_cond_grad(B, P, N, T, _lib.ptr(dy2), _lib.ptr(cat), _lib.ptr(dt), None,
                                                                    _lib.ptr(ws), wsb, _lib.stream_ptr()))
    samples = {"forward_fused": [], "forward_literal": [], "backward_fused": [], "backward_literal": [], "step_fused": [],
               "step_literal": [], "cond_grad": []}
    for _ in range(args.rounds):
        for fused, tag in ((True, "fused"), (False, "literal")):
            samples["forward_" + tag].append(timed(lambda: layer(fused)))
            y = layer(fused)
            samples["backward_" + tag].append(timed(lambda: torch.autograd.grad(y, wrt, dy, retain_graph=True)))
            del y
            samples["step_" + tag].append(timed(lambda: torch.autograd.grad(layer(fused), wrt, dy)))
        samples["cond_grad"].append(timed(cond_grad))
    for k, v in samples.items():
        out[k + "_us"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    # where a form's time goes: device time of every C-ABI call of one forward + backward (warm; the literal form's torch
    # copies — the tile, the concatenations, the slices back — are what its total has beyond its calls)
    for fused, tag in ((True, "fused"), (False, "literal")):
        _lib.timing_start()
        torch.autograd.grad(layer(fused), wrt, dy)
        events = _lib.timing_stop()
        torch.cuda.synchronize()
        out["calls_" + tag + "_us"] = [[name, list(dims), round(e0_.elapsed_time(e1_) * 1e3, 1)] for name, dims, e0_, e1_ in events]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
