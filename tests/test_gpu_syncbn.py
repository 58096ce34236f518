"""Batch-norm statistics over all ranks' rows on the GPU (tf_norm.set_sync; csrc/norm.hip: sph3d_elu_bn_{forward,backward}_{sums,
apply}): shards of one tensor as virtual ranks on one GPU against the float64 statement over ALL rows, the identity reducer
against the plain ops bit for bit, the GEMM-epilogue route, the layer functions, the registered ops, and one rank over RCCL."""
import os
import subprocess
import sys

import pytest
import torch

from sph3d_gcn_amd import _lib, tf_norm
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-5, atol=1e-5)          # the project's tolerance for activations (tests/test_gpu_parity.py)

CASES = [(4, (1, 5)), (64, (700, 300)), (192, (777, 1223, 3)), (1024, (33, 31)), (128, (40000, 1000))]
IDS = ["C%d-%s" % (c, "+".join(str(r) for r in rows)) for c, rows in CASES]


class _AllReduce:
    """stand-in reducer of virtual rank k: the sum over the ranks in rank order, as an all-reduce gives every rank the same bits —
    the rank's own term is the live buffer, the others' are what the public *_sums ops gave for their shards"""

    def __init__(self, k, fwd, bwd):
        self.k, self.sums, self.calls = k, {fwd[0].numel(): fwd, bwd[0].numel(): bwd}, []

    def __call__(self, buf):
        assert buf.dtype == torch.float64 and buf.dim() == 1 and buf.is_cuda
        self.calls.append(buf.numel())
        terms = [buf.clone() if j == self.k else s for j, s in enumerate(self.sums[buf.numel()])]
        total = terms[0].clone()
        for t in terms[1:]:
            total += t
        buf.copy_(total)


def _case(C, rows, dev):
    g = torch.Generator(device="cpu").manual_seed(sum(rows) + C)
    R = sum(rows)
    y = (torch.randn(R, C, generator=g) * 2 - 0.3).to(dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = torch.randn(C, generator=g).to(dev)
    dout = torch.randn(R, C, generator=g).to(dev)
    return y, gamma, beta, dout


def _statement(y, gamma, beta, dout):
    """float64 ELU -> batch norm over all rows -> out, dy, dgamma, dbeta, moving_mean, moving_var (from 0.1 / 0.7, biased variance)"""
    yd = y.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = torch.nn.functional.elu(yd)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    out = (z - mean) / torch.sqrt(var + 1e-3) * gd + bd
    out.backward(dout.double())
    return (out.detach(), yd.grad, gd.grad, bd.grad, 0.99 * 0.1 + 0.01 * mean.detach(), 0.99 * 0.7 + 0.01 * var.detach(),
            mean.detach(), torch.rsqrt(var.detach() + 1e-3))


def _check_against_statement(got, want):
    """got: out, dy, sum dgamma, sum dbeta, moving_mean, moving_var — at the tolerances of test_gpu_parity.py::test_fused_elu_batch_norm"""
    out, dy, dgamma, dbeta, mm, mv = got
    torch.testing.assert_close(out.double(), want[0], rtol=1e-5, atol=2e-5)
    if dy is not None:
        torch.testing.assert_close(dy.double(), want[1], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(dgamma.double(), want[2], rtol=1e-4, atol=1e-4 * max(1.0, float(want[2].abs().max())))
    torch.testing.assert_close(dbeta.double(), want[3], rtol=1e-4, atol=1e-4 * max(1.0, float(want[3].abs().max())))
    torch.testing.assert_close(mm.double(), want[4], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(mv.double(), want[5], rtol=1e-5, atol=1e-6)


def _buffers(C, dev):
    return torch.zeros(C, device=dev) + 0.1, torch.ones(C, device=dev) * 0.7


@pytest.mark.parametrize("C,rows", CASES, ids=IDS)
def test_virtual_ranks_equal_the_statement_over_all_rows(dev, C, rows):
    y, gamma, beta, dout = _case(C, rows, dev)
    want = _statement(y, gamma, beta, dout)
    ys, ds = torch.split(y, rows), torch.split(dout, rows)
    # the cut, with the public ops: every shard's sums, the statistics from their total on every shard
    fwd = [tf_norm.elu_bn_forward_sums(s) for s in ys]
    for f, r in zip(fwd, rows):
        assert f.shape == (2 * C + 1,) and f.dtype == torch.float64 and float(f[2 * C]) == r
    total = fwd[0].clone()
    for f in fwd[1:]:
        total += f
    stats = []
    for s in ys:
        mm, mv = _buffers(C, dev)
        _out, sm, sr, count = tf_norm.elu_bn_forward_apply(s, total.clone(), gamma, beta, mm, mv)
        assert count.dtype == torch.float64 and float(count) == sum(rows)
        stats.append((sm, sr))
    for sm, sr in stats[1:]:                               # the statistics do not depend on the shard
        assert torch.equal(sm, stats[0][0]) and torch.equal(sr, stats[0][1])
    torch.testing.assert_close(stats[0][0].double(), want[6], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[0][1].double(), want[7], rtol=1e-5, atol=1e-6)
    bwd = [tf_norm.elu_bn_backward_sums(s, d, stats[0][0], stats[0][1])[2] for s, d in zip(ys, ds)]
    # every shard as one rank through the autograd function
    outs, dys, dgs, dbs, moving = [], [], [], [], []
    for k, (s, d) in enumerate(zip(ys, ds)):
        red = _AllReduce(k, fwd, bwd)
        y1, g1, b1 = s.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        mm, mv = _buffers(C, dev)
        with tf_norm.sync(red):
            out = tf_norm.elu_batch_norm(y1, g1, b1, mm, mv, True)
            out.backward(d)
        assert red.calls == [2 * C + 1, 2 * C]
        outs.append(out.detach()); dys.append(y1.grad); dgs.append(g1.grad); dbs.append(b1.grad); moving.append((mm, mv))
    for mm, mv in moving[1:]:
        assert torch.equal(mm, moving[0][0]) and torch.equal(mv, moving[0][1])
    _check_against_statement((torch.cat(outs), torch.cat(dys), sum(dgs), sum(dbs), moving[0][0], moving[0][1]), want)


@pytest.mark.parametrize("C,rows", CASES, ids=IDS)
def test_identity_reducer_is_the_plain_op_bit_for_bit(dev, C, rows):
    y, gamma, beta, dout = _case(C, rows, dev)

    def run(reducer):
        y1, g1, b1 = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        mm, mv = _buffers(C, dev)
        with tf_norm.sync(reducer):
            out = tf_norm.elu_batch_norm(y1, g1, b1, mm, mv, True)
            out.backward(dout)
        return out.detach(), mm, mv, y1.grad, g1.grad, b1.grad

    calls = []
    for a, b in zip(run(lambda buf: calls.append(buf.numel())), run(None)):
        assert torch.equal(a, b)
    assert calls == [2 * C + 1, 2 * C]
    # save_mean / save_rstd: the ops themselves
    mm, mv = _buffers(C, dev)
    _o, sm, sr = tf_norm._fwd_impl(y, gamma, beta, mm, mv, True)
    mm2, mv2 = _buffers(C, dev)
    o2, sm2, sr2, count = tf_norm.elu_bn_forward_apply(y, tf_norm.elu_bn_forward_sums(y), gamma, beta, mm2, mv2)
    assert torch.equal(sm, sm2) and torch.equal(sr, sr2) and torch.equal(_o, o2) and torch.equal(mm, mm2) and torch.equal(mv, mv2)
    dy, dg, db = tf_norm._bwd_impl(y, dout, gamma, sm, sr, True)
    dg2, db2, sums = tf_norm.elu_bn_backward_sums(y, dout, sm2, sr2)
    dy2 = tf_norm.elu_bn_backward_apply(y, dout, gamma, sm2, sr2, sums, count)
    assert torch.equal(dy, dy2) and torch.equal(dg, dg2) and torch.equal(db, db2)


def test_inference_mode_and_no_reducer_run_no_new_kernel(dev):
    y, gamma, beta, dout = _case(64, (700, 300), dev)
    calls = []
    mm, mv = _buffers(64, dev)
    _lib.timing_start()
    with tf_norm.sync(lambda buf: calls.append(buf.numel())):
        tf_norm.elu_batch_norm(y, gamma, beta, mm, mv, False)
    y1 = y.clone().requires_grad_(True)
    tf_norm.elu_batch_norm(y1, gamma, beta, mm, mv, True).backward(dout)
    names = [n for n, *_ in _lib.timing_stop()]
    assert calls == [] and names == ["sph3d_elu_bn_forward", "sph3d_elu_bn_forward", "sph3d_elu_bn_backward"]


# ---- statistics from the GEMM's epilogue -----------------------------------------------------------------------------------------
def test_gemm_epilogue_route_under_virtual_ranks(dev):
    rows, Cin, Cout = (4096, 4096), 64, 128
    assert tf_norm.gemm_bn_blocks(rows[0], Cin, Cout) > 0 and tf_norm.gemm_bn_blocks(sum(rows), Cin, Cout) > 0
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(sum(rows), Cin, generator=g).to(dev)
    w = (torch.randn(Cin, Cout, generator=g) / Cin ** 0.5).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(Cout, generator=g)).to(dev)
    beta = (0.1 * torch.randn(Cout, generator=g)).to(dev)
    dout = torch.randn(sum(rows), Cout, generator=g).to(dev)

    def run(xk, dk, reducer):
        xs, ws, gs, bs = (t.clone().requires_grad_(True) for t in (xk, w, gamma, beta))
        mm, mv = _buffers(Cout, dev)
        _lib.timing_start()
        with tf_norm.sync(reducer):
            out = tf_norm.gemm_elu_batch_norm(xs, ws, gs, bs, mm, mv)
            out.backward(dk)
        names = [n for n, *_ in _lib.timing_stop()]
        assert "sph3d_pointwise_gemm_bnstats" in names
        assert ("sph3d_elu_bn_forward_sums" in names) == (reducer is not None)
        return [out.detach(), xs.grad, ws.grad, gs.grad, bs.grad, mm, mv]

    # the float64 statement: product -> ELU -> batch norm over all rows
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yd = xd @ wd
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = torch.nn.functional.elu(yd)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    ref = (z - mean) / torch.sqrt(var + 1e-3) * gd + bd
    ref.backward(dout.double())

    # the shards' sums with the public ops: forward from the GEMM's partials, backward from the global statistics
    xs_, ds_ = torch.split(x, rows), torch.split(dout, rows)
    prods = [tf_norm._gemm_bnstats_impl(s, w, None) for s in xs_]
    fwd = [tf_norm.elu_bn_forward_sums(yk, pk) for yk, pk in prods]
    mm, mv = _buffers(Cout, dev)
    _o, sm, sr, _c = tf_norm.elu_bn_forward_apply(prods[0][0], fwd[0] + fwd[1], gamma, beta, mm, mv)
    bwd = [tf_norm.elu_bn_backward_sums(yk, dk, sm, sr)[2] for (yk, _p), dk in zip(prods, ds_)]
    got = [run(xk, dk, _AllReduce(k, fwd, bwd)) for k, (xk, dk) in enumerate(zip(xs_, ds_))]
    assert torch.equal(got[0][5], got[1][5]) and torch.equal(got[0][6], got[1][6])
    _check_against_statement((torch.cat([r[0] for r in got]), None, got[0][3] + got[1][3], got[0][4] + got[1][4], got[0][5], got[0][6]),
                             (ref.detach(), None, gd.grad, bd.grad, 0.99 * 0.1 + 0.01 * mean.detach(), 0.99 * 0.7 + 0.01 * var.detach()))
    # dy leaves the function only through the product's gradients: dx per shard, dw summed over the shards (rtol 1e-4 like the
    # other gradients)
    dx, dw = torch.cat([r[1] for r in got]), got[0][2] + got[1][2]
    torch.testing.assert_close(dx.double(), xd.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(xd.grad.abs().max())))
    torch.testing.assert_close(dw.double(), wd.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(wd.grad.abs().max())))
    # identity reducer on the whole tensor: the plain call bit for bit
    for a, b in zip(run(x, dout, lambda buf: None), run(x, dout, None)):
        assert torch.equal(a, b)


# ---- layer functions: each cloud of a two-cloud batch as one virtual rank ---------------------------------------------------------
class _Lockstep:
    """reducer of one virtual rank over several passes: call i adds what the OTHER rank's call i held in the previous pass (its own
    sums: they do not depend on the reducer for the forward call of one layer, and for the backward call once the forward is right)"""

    def __init__(self, other_prev):
        self.other_prev, self.own = other_prev, []

    def __call__(self, buf):
        i = len(self.own)
        self.own.append(buf.clone())
        if i < len(self.other_prev):
            buf.add_(self.other_prev[i])


def _layer_virtual_ranks(layer, inputs, dev):
    """layer(store, x, k) -> out for cloud k (k None: the whole batch).  -> per rank (out, dx, grads, buffers) after three passes:
    forward sums known, then backward sums known, then both"""
    prev = [[], []]
    for _ in range(3):
        res, own = [], []
        for k in range(2):
            store = s3g_util.VariableStore(device=dev, seed=11)
            x = inputs[k:k + 1].clone().requires_grad_(True)
            red = _Lockstep(prev[1 - k])
            with tf_norm.sync(red), s3g_util.variable_store(store):
                out = layer(x, k)
                (out * _gout(out, k)).sum().backward()
            assert len(red.own) == 2
            own.append(red.own)
            res.append((out.detach(), x.grad, {n: p.grad.clone() for n, p in store.params.items()},
                        {n: b.clone() for n, b in store.named_buffers()}))
        prev = own
    return res


def _gout(out, k):
    g = torch.Generator(device="cpu").manual_seed(4)
    full = torch.randn((2,) + tuple(out.shape[1:]), generator=g).to(out.device)
    return full if k is None else full[k:k + 1]


def _layer_whole(layer, inputs, dev):
    store = s3g_util.VariableStore(device=dev, seed=11)
    x = inputs.clone().requires_grad_(True)
    with s3g_util.variable_store(store):
        out = layer(x, None)
        (out * _gout(out, None)).sum().backward()
    return out.detach(), x.grad, {n: p.grad.clone() for n, p in store.params.items()}, {n: b.clone() for n, b in store.named_buffers()}


def _compare_layer(ranks, whole):
    torch.testing.assert_close(torch.cat([r[0] for r in ranks]), whole[0], **TOL)
    torch.testing.assert_close(torch.cat([r[1] for r in ranks]), whole[1], rtol=1e-4, atol=1e-4 * max(1.0, float(whole[1].abs().max())))
    assert set(ranks[0][2]) == set(whole[2])
    for n, gw in whole[2].items():
        torch.testing.assert_close(ranks[0][2][n] + ranks[1][2][n], gw, rtol=1e-4, atol=1e-4 * max(1.0, float(gw.abs().max())), msg=n)
    for n, bw in whole[3].items():
        torch.testing.assert_close(ranks[0][3][n], bw, rtol=1e-5, atol=1e-6)
        assert torch.equal(ranks[0][3][n], ranks[1][3][n])


def test_pointwise_layer_virtual_ranks(dev):
    feat = torch.randn(2, 512, 32, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    feat[1] = feat[1] * 1.5 + 0.4                    # the two clouds' statistics differ

    def layer(x, k):
        return s3g_util.pointwise_conv3d(x, 64, 'p1', with_bn=True, is_training=True)

    _compare_layer(_layer_virtual_ranks(layer, feat, dev), _layer_whole(layer, feat, dev))


@pytest.mark.parametrize("fuse", [False, True], ids=["layer-by-layer", "one-kernel"])
def test_separable_layer_virtual_ranks(dev, fuse):
    xyz = torch.from_numpy(synth.s3dis_batch(3, 2, 512, extent=(0.8, 0.8, 1.0))[0][:, :, :3].copy()).to(dev)
    idx, cnt, dst, filt = s3g_util.build_intra_graph(xyz, 0.2, 32, [8, 2, 2])
    feat = torch.randn(2, 512, 32, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)
    feat[1] = feat[1] * 1.5 + 0.4

    def layer(x, k):
        s = slice(None) if k is None else slice(k, k + 1)
        return s3g_util.separable_conv3d(x, 64, 33, 2, 'c1', idx[s], cnt[s], filt[s], with_bn=True, is_training=True)

    old = s3g_util.FUSE_SEPARABLE_TRAINING
    s3g_util.FUSE_SEPARABLE_TRAINING = fuse
    try:
        _lib.timing_start()
        ranks = _layer_virtual_ranks(layer, feat, dev)
        names = [n for n, *_ in _lib.timing_stop()]
        whole = _layer_whole(layer, feat, dev)
    finally:
        s3g_util.FUSE_SEPARABLE_TRAINING = old
    assert ("sph3d_separable_conv3d_train" in names) == fuse
    assert names.count("sph3d_elu_bn_forward_sums") == 6 and names.count("sph3d_elu_bn_backward_apply") == 6
    _compare_layer(ranks, whole)


# ---- the three tails, each plain and under a one-rank reducer ---------------------------------------------------------------------
def _tail_elu_batch_norm(dev):
    C = 12
    y, gamma, beta, dout = _case(C, (33,), dev)

    def run():
        y1, g1, b1 = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
        mm, mv = _buffers(C, dev)
        out = tf_norm.elu_batch_norm(y1, g1, b1, mm, mv, True)
        out.backward(dout)
        return [out.detach(), mm, mv, y1.grad, g1.grad, b1.grad]

    return C, run


def _tail_gemm_elu_batch_norm(dev):
    R, Cin, C = 1024, 64, 128                                 # tests/test_gpu_round3.py: test_gemm_bnstats_ops_registered
    g = torch.Generator(device="cpu").manual_seed(R + Cin)
    x = (torch.randn(R, Cin, generator=g) * 0.5).to(dev)
    w = (torch.randn(Cin, C, generator=g) / Cin ** 0.5).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    dout = torch.randn(R, C, generator=g).to(dev)

    def run():
        xs, ws, gs, bs = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
        mm, mv = _buffers(C, dev)
        out = tf_norm.gemm_elu_batch_norm(xs, ws, gs, bs, mm, mv)
        out.backward(dout)
        return [out.detach(), mm, mv, xs.grad, ws.grad, gs.grad, bs.grad]

    return C, run


def _tail_separable(dev):
    from sph3d_gcn_amd import tf_buildkernel, tf_conv3d, tf_nnquery
    kind, B, N, M, radius, K, kernel, Cin, r, C = ("uniform", 1, 64, 40, 0.3, 16, [8, 2, 2], 128, 2, 128)      # tests/test_gpu_sepring.py
    xyz = torch.from_numpy(synth.uniform_cloud(7, B, N, 1.0).copy()).to(dev)
    q = xyz[:, :M].contiguous()
    idx, cnt, dst = tf_nnquery.build_sphere_neighbor(xyz, q, radius, None, K)
    filt = tf_buildkernel.spherical_kernel(xyz, q, idx, cnt, dst, radius, kernel)
    F = kernel[0] * kernel[1] * kernel[2] + 1
    g = torch.Generator(device="cpu").manual_seed(Cin * 7 + C)
    x = torch.randn(B, N, Cin, generator=g).to(dev)
    dwf = torch.randn(F, Cin, r, generator=g).to(dev)
    w = (torch.randn(Cin * r, C, generator=g) / (Cin * r) ** 0.5).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    dout = torch.randn(B, M, C, generator=g).to(dev)
    assert tf_conv3d.separable_train_supported(x, dwf, idx, C)

    def run():
        xs, fs, ws, cs, gs, bs = (t.clone().requires_grad_(True) for t in (x, dwf, w, bias, gamma, beta))
        mm, mv = _buffers(C, dev)
        out = tf_conv3d.separable_conv3d_elu_bn_train(xs, fs, ws, gs, bs, mm, mv, idx, cnt, filt, bias=cs)
        out.backward(dout)
        torch.cuda.synchronize()
        assert _lib.lib().sph3d_separable_conv3d_ring_failures() == 0
        return [out.detach(), mm, mv, xs.grad, fs.grad, ws.grad, cs.grad, gs.grad, bs.grad]

    return C, run


@pytest.mark.parametrize("tail", [_tail_elu_batch_norm, _tail_gemm_elu_batch_norm, _tail_separable],
                         ids=["elu_batch_norm", "gemm_elu_batch_norm", "separable_conv3d_elu_bn_train"])
def test_every_tail_under_a_one_rank_reducer_is_the_plain_tail_bit_for_bit(dev, tail):
    """the reducer of one rank leaves the buffer as it is: it is called once per forward pass with 2C + 1 values and once per backward
    pass with 2C, and out, both moving statistics and every gradient carry the bits of the call without a reducer"""
    C, run = tail(dev)
    calls = []

    def one_rank(buf):
        assert buf.dtype == torch.float64 and buf.dim() == 1 and buf.is_cuda
        calls.append(buf.numel())

    plain = run()
    assert calls == []
    with tf_norm.sync(one_rank):
        synced = run()
    assert calls == [2 * C + 1, 2 * C]
    assert len(plain) == len(synced) >= 6                      # out, two moving statistics, at least three gradients
    for i, (a, b) in enumerate(zip(plain, synced)):
        assert a is not None and torch.equal(a, b), "result %d differs" % i


# ---- the registered ops ----------------------------------------------------------------------------------------------------------
def test_sync_ops_registered(dev):
    checks = ("test_schema", "test_faketensor")
    y, gamma, beta, dout = _case(16, (200,), dev)
    mm, mv = _buffers(16, dev)
    sums = torch.ops.sph3d.elu_bn_forward_sums(y, None)
    torch.library.opcheck(torch.ops.sph3d.elu_bn_forward_sums, (y, None), test_utils=checks)
    part = torch.rand(3, 2, 16, device=dev)
    torch.library.opcheck(torch.ops.sph3d.elu_bn_forward_sums, (y, part), test_utils=checks)
    out, sm, sr, count = torch.ops.sph3d.elu_bn_forward_apply(y, sums, gamma, beta, mm, mv)
    torch.library.opcheck(torch.ops.sph3d.elu_bn_forward_apply, (y, sums, gamma, beta, mm.clone(), mv.clone()), test_utils=checks)
    dg, db, bsums = torch.ops.sph3d.elu_bn_backward_sums(y, dout, sm, sr)
    torch.library.opcheck(torch.ops.sph3d.elu_bn_backward_sums, (y, dout, sm, sr), test_utils=checks)
    torch.library.opcheck(torch.ops.sph3d.elu_bn_backward_apply, (y, dout, gamma, sm, sr, bsums, count), test_utils=checks)
    with pytest.raises(ValueError):
        tf_norm.elu_bn_forward_apply(y, sums[:-1].contiguous(), gamma, beta, mm, mv)
    with pytest.raises(ValueError):
        tf_norm.elu_bn_backward_apply(y, dout, gamma, sm, sr, bsums.float(), count)
    with pytest.raises(ValueError):
        tf_norm.elu_bn_forward_sums(torch.randn(8, 6, device=dev))           # C % 4 != 0


# ---- RCCL ------------------------------------------------------------------------------------------------------------------------
def _torchrun(nproc, port, script, *args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["SPH3D_FORCE_COLLECTIVES"] = "1"
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", script)] + list(args),
                          env=env, capture_output=True, text=True, timeout=600)


def test_trainer_sync_bn_one_rank_over_rccl():
    """Trainer(sync_bn=True) as one rank with SPH3D_FORCE_COLLECTIVES=1: every statistics all-reduce really goes through RCCL, and
    at world size 1 the sum is the identity, so the steps are those of sync_bn=False (the worker checks)"""
    p = _torchrun(1, 29543, "_syncbn_rccl_worker.py")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "SYNCBN_RCCL_OK" in p.stdout


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_ranks_over_rccl_equal_the_whole_batch():
    p = _torchrun(2, 29545, "_syncbn_gloo_worker.py", "cuda")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "SYNCBN_GLOO_OK" in p.stdout
