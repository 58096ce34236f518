"""Shared inputs of the keyed inverse-density sampler's tests (tests/test_idsample.py, tests/test_gpu_idsample.py)."""
import copy
import functools

import numpy as np
import torch

from oracle import torch_ops
from sph3d_gcn_amd.harness import s3dis_net, synth


def graph_inputs(B, N, K, seed, nan_tail):
    """nn_dist [B, N, K] float32, nn_count [B, N] int32 as an intra graph gives them, with the cases the statement names:
    counts uniform in 0..K (at least 10 % zeros for K <= 9, 1 / (K + 1) of them otherwise plus the zeroed cloud), a few rows
    with inf or all-zero distances, one cloud with all counts 0 (the last, when B > 1), and (nan_tail) NaN in the slots >=
    count, which are not read"""
    rng = np.random.RandomState(seed)
    d = (rng.rand(B, N, K).astype(np.float32) * np.float32(0.3)) ** 2
    c = rng.randint(0, K + 1, size=(B, N)).astype(np.int32)
    zeros = rng.rand(B, N) < 0.1
    c[zeros] = 0
    for r in rng.randint(0, N, size=min(N, 5)):
        d[0, r, :] = 0.0
        c[0, r] = max(c[0, r], 1)
    for r in rng.randint(0, N, size=min(N, 5)):
        d[0, r, 0] = np.inf
        c[0, r] = max(c[0, r], 1)
    if B > 1:
        c[B - 1] = 0
    slot = np.arange(K)[None, None, :]
    d = np.where(slot < c[:, :, None], d, np.float32(np.nan) if nan_tail else np.float32(0)).astype(np.float32)
    return d, c


def ids_config(num_input=1024):
    cfg = copy.deepcopy(s3dis_net.small_config(num_input))
    cfg.sample = 'IDS'
    return cfg


def plan_batch():
    """the batch the plan tests share: -> xyz+features [2, 1024, 9] float32, label, inner"""
    return synth.s3dis_batch(0, 2, 1024, extent=(1.0, 1.0, 1.5))


@functools.lru_cache(maxsize=4)
def cpu_plan(key=(5, 3), decoder=True):
    """the CPU plan (oracle ops, numpy statement of the sampler) of small_config(1024) with sample = 'IDS', every graph built;
    computed once per key and left unchanged"""
    cfg = ids_config()
    pts = torch.from_numpy(plan_batch()[0])
    with torch_ops.patched_util():
        plan = s3dis_net.GraphPlan(pts, cfg, sample_key=key, decoder=decoder)
        for l in range(len(cfg.radius)):
            plan.enc(l)
            plan.pool(l)
        if decoder:
            for l in range(len(cfg.radius)):
                plan.dec(l)
    return plan
