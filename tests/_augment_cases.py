"""The batches tests/test_gpu_augment.py runs on the device; tests/test_augment.py checks on the CPU that the statement alone
decides every elastic skip among them with a margin of a whole node, so that fp32 cell indices cannot change a decision."""
import numpy as np

from sph3d_gcn_amd.harness import augment

LDS_NODES = 8192          # csrc/augment.hip: kAugLdsNodes — the lattice lives in LDS up to this many raw nodes


def options(layout, max_nodes=32768, **prob):
    """default_options with single probabilities replaced, e.g. mix=1.0"""
    names = ("mix", "flipx", "flipy", "ascale", "elastic", "autocontrast", "ctranslate", "cjitter", "cdrop")
    o = augment.default_options(layout, max_nodes=max_nodes)
    return o._replace(prob=tuple(prob.get(n, p) for n, p in zip(names, o.prob)))


def batch_a(C=6):
    """B = 5, N = 777 (odd B, odd N, 777 = 12 * 64 + 9: every cloud boundary falls inside a wave).  Cloud 0 straddles the origin
    (negative node indices: floor, not truncation); cloud 1 is one point repeated (max == min in every channel, a one-node box);
    cloud 2 holds a point exactly on a lattice node of both passes and fills a box too large for LDS; cloud 3 is too wide for
    max_nodes in both passes; cloud 4 has one coordinate beyond the +-500-node range of both passes."""
    rng = np.random.RandomState(7)
    B, N = 5, 777
    p = np.empty((B, N, C), dtype=np.float32)
    p[..., 3:] = rng.rand(B, N, C - 3) * 2 - 1
    p[0, :, 0:3] = rng.rand(N, 3) * np.array([1.4, 1.4, 1.5]) + np.array([-0.7, -0.7, -0.5])
    p[1] = np.array([0.3, -0.7, 1.1, 0.25, -0.5, 0.75] + [0.1] * (C - 6), dtype=np.float32)
    p[2, :, 0:3] = rng.rand(N, 3) * np.array([3.0, 3.0, 3.6])
    p[2, 0, 0:3] = (0.8, 1.6, 2.4)                      # a node of g = 0.2 and of g = 0.8 (before scaling)
    p[2, 1, 0:3] = (2.999, 2.999, 3.599)                # the top cell of the box
    p[2, 2, 0:3] = (0.0, 0.0, 0.0)
    p[3, :, 0:3] = rng.rand(N, 3) * np.array([28.0, 28.0, 28.0]) + np.array([-14.0, -14.0, 0.0])
    p[4, :, 0:3] = rng.rand(N, 3) * np.array([1.4, 1.4, 2.5])
    p[4, 5, 0] = 450.0
    label = rng.randint(0, 13, (B, N)).astype(np.int32)
    inner = rng.randint(0, 2, (B, N)).astype(np.int32)
    return p, label, inner


def batch_e():
    """B = 4, N = 300, C = 9: the facade layout xyz, unit normal, rgb"""
    rng = np.random.RandomState(9)
    B, N = 4, 300
    p = np.empty((B, N, 9), dtype=np.float32)
    p[..., 0:3] = rng.rand(B, N, 3) * np.array([2.0, 1.0, 2.5]) - np.array([1.0, 0.5, 0.0])
    n = rng.randn(B, N, 3)
    p[..., 3:6] = n / np.sqrt((n * n).sum(axis=2, keepdims=True))
    p[..., 6:9] = rng.rand(B, N, 3) * 2 - 1
    return p, rng.randint(0, 8, (B, N)).astype(np.int32), None


def small(B, N, C, seed):
    rng = np.random.RandomState(seed)
    p = (rng.rand(B, N, C) * 2 - 1).astype(np.float32)
    return p, rng.randint(0, 13, (B, N)).astype(np.int32), rng.randint(0, 2, (B, N)).astype(np.int32)


SKIP_OPTS = options("s3dis", max_nodes=16384, elastic=1.0)._replace(enable=augment.GEOMETRIC & ~augment.MIX | augment.COLOUR)

# name -> (batch, options, [(seed, step)])
CASES = {
    "a": (batch_a(), options("s3dis"), [(1, 0), (2, 12345678901), (0xfedcba9876543210, 3)]),
    "a_skip": (batch_a(), SKIP_OPTS, [(5, 1)]),
    "b": (small(1, 64, 6, 1), options("s3dis", mix=1.0), [(3, 4)]),
    "c": (small(2, 1, 6, 2), options("s3dis", mix=1.0), [(3, 5), (4, 5)]),
    "d": (small(2, 2, 6, 3), options("s3dis", mix=1.0), [(3, 6), (4, 6)]),
    "e": (batch_e(), options("facade"), [(1, 0), (2, 1), (3, 2), (4, 3)]),
    "xyz": (small(3, 130, 3, 4), options("object"), [(8, 8), (9, 9)]),
}


def margins(report, max_nodes):
    """every elastic decision of `report` again with the cell box grown (a pass that ran) or shrunk (a pass that was skipped) by
    a whole node per side -> [(b, pass, ran, still)]: `still` says the decision survives"""
    out = []
    for b, which, cmin, cmax in report.boxes:
        ran = augment.box_ok(cmin, cmax, max_nodes)
        still = augment.box_ok(cmin - 1, cmax + 1, max_nodes) if ran else not augment.box_ok(cmin + 1, np.maximum(cmax - 1, cmin + 1), max_nodes)
        out.append((b, which, ran, still))
    return out
