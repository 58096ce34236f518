"""Isolated timing of the Lovasz-softmax loss (csrc/lovasz.hip) beside the torch statement and the masked
cross-entropy in one run, at 16 x 8192 x 13 (S3DIS) and 16 x 8192 x 21 (ScanNet's classes at the S3DIS block size), and a Trainer
step on s3dis_config with model.loss and with lovasz.with_xent(model.loss).
A measurement, not a test (tests/test_gpu_lovasz.py holds the outputs to the statement).  Device us per call from events around
20 calls after 3 warm-up calls, the candidates alternating, median of 5 rounds; the steps as wall-clock ms with a synchronize,
median of 9 alternating pairs.  The three launches' own times are a kernel trace's business:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_lovasz.py --op-only
runs the op alone (forward + backward, 20 calls per shape after 3) for that.
--large measures the global-memory sort (tf_loss.lovasz_softmax_large) against lovasz_torch at 16 x 65536 x 21 (block scope) and at
the batch reductions of 32 x 2048 x 50, 16 x 8192 x 13 and 16 x 8192 x 7, and against the LDS sort at 16 x 16384 x 13, the same way
with 3 rounds.
usage: python tools/exp_lovasz.py [--op-only] [--skip-steps] [--large]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sph3d_gcn_amd import tf_loss  # noqa: E402
from sph3d_gcn_amd.harness import lovasz, optim, s3dis_net, synth, train  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = ((16, 8192, 13), (16, 8192, 21))


def timed(fn, reps=20, warm=3):
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


def inputs(B, N, C):
    g = torch.Generator(device="cpu").manual_seed(B * N + C)
    pred = (3.0 * torch.randn(B, N, C, generator=g)).to(dev)
    label = torch.randint(0, C, (B, N), generator=g).to(dev)
    inner = (torch.rand(B, N, generator=g) < 0.7).float().to(dev)
    return pred, label, inner


def fwd_bwd(loss_of, pred, label, inner):
    p = pred.detach().requires_grad_(True)
    loss_of(p, label, inner).sum().backward()


def fwd(loss_of, pred, label, inner):
    with torch.no_grad():
        loss_of(pred, label, inner)


def op_only():
    for B, N, C in SHAPES:
        pred, label, inner = inputs(B, N, C)
        t = timed(lambda: fwd_bwd(tf_loss.lovasz_softmax, pred, label, inner))
        print("%d x %d x %d  kernels, forward + backward: %.1f us" % (B, N, C, t), flush=True)


def ops():
    print("== device us per call (median of 5 alternating rounds): forward | forward + backward")
    for B, N, C in SHAPES:
        pred, label, inner = inputs(B, N, C)
        cands = (("lovasz kernels", tf_loss.lovasz_softmax), ("lovasz_torch", lovasz.lovasz_torch),
                 ("masked_softmax_xent", lambda p, l, i: tf_loss.masked_softmax_xent(p, l, i)))
        times = {name: ([], []) for name, _ in cands}
        for _ in range(5):
            for name, fn in cands:
                times[name][0].append(timed(lambda: fwd(fn, pred, label, inner)))
                times[name][1].append(timed(lambda: fwd_bwd(fn, pred, label, inner)))
        for name, _ in cands:
            print("%d x %d x %d  %-22s %9.1f | %9.1f" % (B, N, C, name, statistics.median(times[name][0]),
                                                        statistics.median(times[name][1])), flush=True)


def steps():
    print("== Trainer.train_step, s3dis_config 16 x 8192, ms (median of 9 alternating pairs): model.loss | with_xent(model.loss, 1.0)")
    xyz, label, inner = synth.s3dis_batch(1000, 16, 8192)
    item = (torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev), None)
    trainers = []
    for wrap in (lambda m: m.loss, lambda m: lovasz.with_xent(m.loss, 1.0)):
        model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(8192), device=dev)
        trainers.append(train.Trainer(model, wrap(model), lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, 16),
                                      13, prime=item[:3], log=lambda s: None))
    times = {0: [], 1: []}
    for it in range(11):
        for which in (0, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[which].train_step(item)
            torch.cuda.synchronize()
            if it >= 2:
                times[which].append((time.perf_counter() - t0) * 1e3)
    print("train_step %8.3f | %8.3f" % (statistics.median(times[0]), statistics.median(times[1])), flush=True)


def large():
    """the global-memory sort (tf_loss.lovasz_softmax_large) against lovasz_torch where the LDS sort does not reach, and against the
    LDS sort at its own largest shape (the price of the global path)"""
    from sph3d_gcn_amd import _lib
    print("== large entry, device us per call (median of 3 alternating rounds): forward | forward + backward; workspace bytes")
    cases = (((16, 65536, 21), "block"), ((32, 2048, 50), "batch"), ((16, 8192, 13), "batch"), ((16, 8192, 7), "batch"),
             ((16, 16384, 13), "block"))
    for (B, N, C), scope in cases:
        pred, label, inner = inputs(B, N, C)
        cands = [("lovasz large", lambda p, l, i, s=scope: tf_loss.lovasz_softmax_large(p, l, i, scope=s))]
        if tf_loss.supported(N, C) and scope == "block":
            cands.append(("lovasz kernels (LDS)", tf_loss.lovasz_softmax))
        cands.append(("lovasz_torch", lambda p, l, i, s=scope: lovasz.lovasz_torch(p, l, i, scope=s)))
        times = {name: ([], []) for name, _ in cands}
        for _ in range(3):
            for name, fn in cands:
                times[name][0].append(timed(lambda: fwd(fn, pred, label, inner)))
                times[name][1].append(timed(lambda: fwd_bwd(fn, pred, label, inner)))
        b, n = (1, B * N) if scope == "batch" else (B, N)
        ws = _lib.lib().sph3d_lovasz_softmax_large_workspace(b, n, C)
        for name, _ in cands:
            print("%d x %d x %d %-5s  %-22s %9.1f | %9.1f   workspace %d" % (B, N, C, scope, name, statistics.median(times[name][0]),
                                                                            statistics.median(times[name][1]), ws), flush=True)


if __name__ == "__main__":
    if "--large" in sys.argv:
        large()
    elif "--op-only" in sys.argv:
        op_only()
    else:
        ops()
        if "--skip-steps" not in sys.argv:
            steps()
