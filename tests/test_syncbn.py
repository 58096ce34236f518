"""Batch-norm statistics over all ranks' rows (tf_norm.set_sync / tf_norm.sync), on the CPU: the torch statement of
s3g_util.batch_normalization under a stand-in reducer, and the whole model on two gloo ranks against the whole batch."""
import os
import subprocess
import sys

import torch

from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd import tf_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R_SHARDS, C = (700, 300), 35


def _data():
    g = torch.Generator(device="cpu").manual_seed(35)
    R = sum(R_SHARDS)
    x = torch.randn(R, C, generator=g) * 2 - 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    dout = torch.randn(R, C, generator=g)
    return x, gamma, beta, dout


def _store(gamma, beta):
    """a fresh variable store whose 'bn' layer has the given gamma / beta and moving statistics 0.1 / 0.7"""
    store = s3g_util.VariableStore()
    g, b, mm, mv = s3g_util._bn_variables(store, 'bn', C)
    with torch.no_grad():
        g.copy_(gamma); b.copy_(beta); mm.fill_(0.1); mv.fill_(0.7)
    return store, g, b, mm, mv


def _run(x, gamma, beta, dout, is_training=True):
    """s3g_util.batch_normalization on x with a fresh store -> out, dx, dgamma, dbeta, moving_mean, moving_var"""
    store, g, b, mm, mv = _store(gamma, beta)
    xr = x.clone().requires_grad_(True)
    with s3g_util.variable_store(store):
        out = s3g_util.batch_normalization(xr, is_training, 'bn')
    out.backward(dout)
    return out.detach(), xr.grad, g.grad, b.grad, mm, mv


class _OtherShards:
    """the reducer of one shard: adds the other shards' float64 sums, known beforehand as plain torch expressions"""

    def __init__(self, fwd_other, bwd_other):
        self.other = {2 * C + 1: fwd_other, 2 * C: bwd_other}
        self.calls = []

    def __call__(self, buf):
        assert buf.dtype == torch.float64 and buf.dim() == 1
        self.calls.append(buf.numel())
        buf.add_(self.other[buf.numel()])


def _sums(x, dout):
    """per shard: the float64 forward sums [2C + 1] and backward sums [2C], with xhat over ALL rows"""
    xd = x.double()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    xhat = (xd - mean) / torch.sqrt(var + 1e-3)
    fwd, bwd, r0 = [], [], 0
    for r in R_SHARDS:
        xs, gs, hs = xd[r0:r0 + r], dout.double()[r0:r0 + r], xhat[r0:r0 + r]
        fwd.append(torch.cat((xs.sum(0), (xs * xs).sum(0), torch.tensor([float(r)], dtype=torch.float64))))
        bwd.append(torch.cat((gs.sum(0), (gs * hs).sum(0))))
        r0 += r
    return fwd, bwd


def test_sharded_batch_norm_equals_whole_batch():
    x, gamma, beta, dout = _data()
    whole = _run(x, gamma, beta, dout)
    assert tf_norm.sync_reducer() is None
    fwd, bwd = _sums(x, dout)
    shards, r0 = [], 0
    for k, r in enumerate(R_SHARDS):
        red = _OtherShards(sum(f for j, f in enumerate(fwd) if j != k), sum(b for j, b in enumerate(bwd) if j != k))
        with tf_norm.sync(red):
            assert tf_norm.sync_reducer() is red
            shards.append(_run(x[r0:r0 + r], gamma, beta, dout[r0:r0 + r]))
        assert tf_norm.sync_reducer() is None
        assert red.calls == [2 * C + 1, 2 * C]          # exactly one call per direction
        r0 += r
    out = torch.cat([s[0] for s in shards])
    dx = torch.cat([s[1] for s in shards])
    dgamma = sum(s[2] for s in shards)
    dbeta = sum(s[3] for s in shards)
    torch.testing.assert_close(out, whole[0], rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(dx, whole[1], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(dgamma, whole[2], rtol=1e-4, atol=1e-4 * max(1.0, float(whole[2].abs().max())))
    torch.testing.assert_close(dbeta, whole[3], rtol=1e-4, atol=1e-4 * max(1.0, float(whole[3].abs().max())))
    # the float64 statement over all rows
    xd = x.double()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    ref = ((xd - mean) / torch.sqrt(var + 1e-3) * gamma.double() + beta.double())
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=2e-5)
    for s in shards:
        # the moving statistics of every shard are the whole batch's (biased variance), and equal from shard to shard
        torch.testing.assert_close(s[4], (0.99 * 0.1 + 0.01 * mean).float(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s[5], (0.99 * 0.7 + 0.01 * var).float(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s[4], whole[4], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s[5], whole[5], rtol=1e-5, atol=1e-6)
        assert torch.equal(s[4], shards[0][4]) and torch.equal(s[5], shards[0][5])


def test_inference_mode_makes_no_reducer_call_and_switch_restores():
    x, gamma, beta, dout = _data()
    before = _run(x, gamma, beta, dout)
    before_eval = _run(x, gamma, beta, dout, is_training=False)
    calls = []
    prev = tf_norm.set_sync(lambda buf: calls.append(buf.numel()))
    try:
        assert prev is None
        under = _run(x, gamma, beta, dout, is_training=False)
        assert calls == []
        for a, b in zip(under, before_eval):
            assert torch.equal(a, b)
        _run(x, gamma, beta, dout)                      # (the identity reducer: one rank)
        assert calls == [2 * C + 1, 2 * C]
    finally:
        assert tf_norm.set_sync(prev) is not None
    assert tf_norm.sync_reducer() is None
    del calls[:]
    after = _run(x, gamma, beta, dout)
    assert calls == []
    for a, b in zip(after, before):
        assert torch.equal(a, b)


def test_gloo_world2_sync_bn_equals_whole_batch():
    """two gloo ranks, 2 + 2 clouds, training-mode batch norm under tf_norm.sync(hdist.stat_all_reduce): gradient, logits and
    moving statistics of the whole batch; without the switch the gradient is far off (the worker checks both)"""
    script = os.path.join(ROOT, "tests", "_syncbn_gloo_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", OMP_NUM_THREADS="2")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29541", script],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "SYNCBN_GLOO_OK" in p.stdout
