"""Isolated timing of the cross-entropy with class weights, label smoothing and an ignore label (csrc/xent.hip):
  (a) at 16 x 8192 x 13 (S3DIS) and 16 x 8192 x 21 (ScanNet's classes at the S3DIS block size): the new op with every option at its
      default, the new op with every option on, and the existing sph3d_masked_softmax_xent, in one run;
  (b) the new op with every option on beside the torch statement (harness/xent.py: xent_torch), at the same shapes and at batch
      scope, 1 x 65 536 x 50 and 1 x 131 072 x 7;
  (c) a Trainer step on s3dis_config with model.loss and with make_loss("s3dis", weights, smoothing, ignore);
  (d) what every workgroup does before its rows (it adds the S slices' counts of its block and one thread forms D in float64 in
      ascending c), at the widest C the op takes: every row masked out and no gradient wanted, so the two launches do nothing else.
A measurement, not a test (tests/test_gpu_xent_ex.py holds the outputs to the statement).  Device us per call from events around 20
calls after 3 warm-up calls, the candidates alternating, median of 5 rounds; the steps as wall-clock ms with a synchronize, median
of 9 alternating pairs.  The events see the host's gaps between launches as well; the kernels' own times are a kernel trace's business:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_xent.py --op-only defaults|options|existing
runs one configuration alone (forward + backward, 20 calls per shape of (a) after 3) for that.
usage: python tools/exp_xent.py [--op-only CONFIG] [--skip-steps] [--prologue-only]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sph3d_gcn_amd import tf_loss  # noqa: E402
from sph3d_gcn_amd.harness import optim, s3dis_net, synth, train, xent  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = ((16, 8192, 13), (16, 8192, 21))
BATCH_SHAPES = ((1, 65536, 50), (1, 131072, 7))


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
    weight = (0.25 + 3.0 * torch.rand(C, generator=g)).to(dev)
    return pred, label, inner, weight


def options(weight):
    return dict(class_weight=weight, label_smoothing=0.1, ignore=0, normalize="weight")


def fwd_bwd(loss_of, pred, label, inner):
    p = pred.detach().requires_grad_(True)
    loss_of(p, label, inner).sum().backward()


def fwd(loss_of, pred, label, inner):
    with torch.no_grad():
        loss_of(pred, label, inner)


def compare(title, shapes, candidates_of):
    print("== %s: device us per call (median of 5 alternating rounds): forward | forward + backward" % title)
    for B, N, C in shapes:
        pred, label, inner, weight = inputs(B, N, C)
        cands = candidates_of(weight)
        times = {name: ([], []) for name, _ in cands}
        for _ in range(5):
            for name, fn in cands:
                times[name][0].append(timed(lambda: fwd(fn, pred, label, inner)))
                times[name][1].append(timed(lambda: fwd_bwd(fn, pred, label, inner)))
        for name, _ in cands:
            print("%d x %d x %d  %-28s %9.1f | %9.1f" % (B, N, C, name, statistics.median(times[name][0]),
                                                        statistics.median(times[name][1])), flush=True)


def op_only(config):
    for B, N, C in SHAPES:
        pred, label, inner, weight = inputs(B, N, C)
        fn = {"defaults": lambda p, l, i: tf_loss.softmax_xent(p, l, i),
              "options": lambda p, l, i: tf_loss.softmax_xent(p, l, i, **options(weight)),
              "existing": lambda p, l, i: tf_loss.masked_softmax_xent(p, l, i)}[config]
        t = timed(lambda: fwd_bwd(fn, pred, label, inner))
        print("%d x %d x %d  %s, forward + backward: %.1f us" % (B, N, C, config, t), flush=True)


def ops():
    compare("(a) the new op beside the existing op", SHAPES, lambda w: (
        ("softmax_xent, defaults", lambda p, l, i: tf_loss.softmax_xent(p, l, i)),
        ("softmax_xent, options on", lambda p, l, i: tf_loss.softmax_xent(p, l, i, **options(w))),
        ("masked_softmax_xent", lambda p, l, i: tf_loss.masked_softmax_xent(p, l, i))))
    compare("(b) the new op beside the torch statement, block scope", SHAPES, lambda w: (
        ("softmax_xent, options on", lambda p, l, i: tf_loss.softmax_xent(p, l, i, **options(w))),
        ("xent_torch, options on", lambda p, l, i: xent.xent_torch(p, l, i, **options(w)))))
    compare("(b) the new op beside the torch statement, batch scope, no mask", BATCH_SHAPES, lambda w: (
        ("softmax_xent, options on", lambda p, l, i: tf_loss.softmax_xent(p, l, None, scope="batch", **options(w))),
        ("xent_torch, options on", lambda p, l, i: xent.xent_torch(p, l, None, scope="batch", **options(w)))))


def prologue():
    print("== (d) count launch + the workgroups' prologue, no counted row, losses only: device us per call (median of 5 rounds)")
    for B, N, C in ((16, 8192, 13), (16, 8192, 4096), (1, 262144, 13), (1, 262144, 4096)):
        pred = torch.zeros(B, N, C, device=dev)
        label = torch.zeros(B, N, dtype=torch.int32, device=dev)
        inner = torch.zeros(B, N, device=dev)
        weight = torch.ones(C, device=dev)
        t = [timed(lambda: fwd(lambda p, l, i: tf_loss.softmax_xent(p, l, i, **options(weight)), pred, label, inner)) for _ in range(5)]
        print("%d x %d x %d  S = %3d  %9.1f" % (B, N, C, min(256, (N + 1023) // 1024), statistics.median(t)), flush=True)
        del pred


def steps():
    print("== (c) Trainer.train_step, s3dis_config 16 x 8192, ms (median of 9 alternating pairs): model.loss | make_loss, options on")
    xyz, label, inner = synth.s3dis_batch(1000, 16, 8192)
    item = (torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev), None)
    weight = xent.class_weights(xent.class_counts(item[1], 13), "median")
    trainers = []
    for loss_of in (lambda m: m.loss, lambda m: xent.make_loss("s3dis", class_weight=weight, label_smoothing=0.1, ignore=0)):
        model = s3dis_net.SPH3DS3DIS(s3dis_net.s3dis_config(8192), device=dev)
        trainers.append(train.Trainer(model, loss_of(model), lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, 16),
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


if __name__ == "__main__":
    if "--op-only" in sys.argv:
        op_only(sys.argv[sys.argv.index("--op-only") + 1])
    elif "--prologue-only" in sys.argv:
        prologue()
    else:
        ops()
        prologue()
        if "--skip-steps" not in sys.argv:
            steps()
