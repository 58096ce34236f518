"""harness/ruemonge_net.py on the device: the nine-channel input with xy centred on the mean, the K = 9 product of mlp1 through the
ragged pointwise path, the reduced plan against the oracle-backed CPU run, one training step that consumes a FacadeFeed item
through `points_ready`, the real network through facadeeval.evaluate, and the mean cross-entropy.  Every launch here is an
ordinary one."""
import contextlib

import numpy as np
import pytest
import torch

from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import facadeeval, facadefeed, ruemonge_net, synth

pytestmark = pytest.mark.gpu


def _cloud9(first, B, N, seed):
    """[B, N, 9] float32: an S3DIS-like slab's xyz, unit normals, rgb in [-1, 1]; labels [B, N] in 0..6"""
    rng = np.random.RandomState(seed)
    xyz = synth.s3dis_batch(first, B, N, extent=(1.0, 1.0, 1.5))[0]
    normal = rng.randn(B, N, 3)
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    rgb = rng.rand(B, N, 3) * 2 - 1
    return np.concatenate((xyz, normal, rgb), axis=2).astype(np.float32), rng.randint(0, 7, (B, N)).astype(np.int32)


def test_net_input_centres_xy_on_the_mean_and_copies_the_rest(dev):
    """xy within 1e-5 * max|xy| of the float64 statement; z and channels 3:9 bit-equal"""
    pts, _ = _cloud9(0, 3, 1000, 1)
    pts[:, :, 0:2] += np.array([30.0, -12.0], dtype=np.float32)            # (a mean far from the origin)
    cfg = ruemonge_net.small_config(1000)
    got = ruemonge_net.net_input(torch.from_numpy(pts).to(dev), cfg).cpu().numpy()
    p64 = pts.astype(np.float64)
    want_xy = p64[:, :, 0:2] - p64[:, :, 0:2].mean(axis=1, keepdims=True)
    assert got.shape == (3, 1000, 9) and got.dtype == np.float32
    err = np.abs(got[:, :, 0:2].astype(np.float64) - want_xy).max()
    bound = 1e-5 * np.abs(p64[:, :, 0:2]).max()
    print("net_input: xy error %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert np.array_equal(got[:, :, 2:].view(np.int32), pts[:, :, 2:].view(np.int32))
    # not the S3DIS centring (the bounding box's centre), and the plan prepares the same tensor on its sampling stream
    from sph3d_gcn_amd.harness import s3dis_net
    assert not np.array_equal(got[:, :, 0:2], s3dis_net.normalize_xyz(torch.from_numpy(pts[:, :, 0:3]).to(dev)).cpu().numpy()[:, :, 0:2])
    t = torch.from_numpy(pts[:, :, :]).to(dev)
    plan = ruemonge_net.GraphPlan(t, cfg, net_input=ruemonge_net.net_input, need_backward=False)
    assert torch.equal(plan.input(t), ruemonge_net.net_input(t, cfg)) and plan.input(t).shape[-1] == 9
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,cout", [(1024, 16), (8192, 64)])
def test_the_nine_channel_product_of_mlp1(dev, n, cout):
    """pointwise_conv3d without batch norm on a [2, n, 9] input: the forward result, the input gradient and the weight gradient
    each within 1e-5 of the sum of their term magnitudes against float64 (the ragged path that serves ModelNet's K = 3).
    Worst error / bound on the MI355X (the test prints it per tensor): 0.021 forward, 0.028 input gradient, 0.0035 weight
    gradient."""
    g = torch.Generator().manual_seed(n + cout)
    x = torch.randn(2, n, 9, generator=g)
    dout = torch.randn(2, n, cout, generator=g)
    store = s3g_util.VariableStore(device=dev, seed=5)
    xs = x.to(dev).requires_grad_(True)
    with s3g_util.variable_store(store):
        out = s3g_util.pointwise_conv3d(xs, cout, 'mlp1', with_bn=False, with_bias=False, activation_fn=None, is_training=True)
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    (name, w), = store.params.items()
    assert tuple(w.shape) == (9, cout) and tuple(out.shape) == (2, n, cout)
    x64, w64, d64 = x.double().reshape(-1, 9), w.detach().cpu().double(), dout.double().reshape(-1, cout)
    checks = (("out", out.detach().cpu().reshape(-1, cout), x64 @ w64, x64.abs() @ w64.abs()),
              ("dx", xs.grad.cpu().reshape(-1, 9), d64 @ w64.t(), d64.abs() @ w64.abs().t()),
              ("dw", w.grad.cpu(), x64.t() @ d64, x64.abs().t() @ d64.abs()))
    worst = {}
    for nm, got, want, terms in checks:
        assert got.shape == want.shape
        worst[nm] = float(((got.double() - want).abs() / (1e-5 * terms)).max())
    print("K=9 product R=2x%d -> %d: worst error / bound %s" % (n, cout, worst))
    for nm, v in worst.items():
        assert v <= 1.0, (nm, v)


def _run_net(device):
    """one forward + backward of the reduced plan with seed-7 weights: on the CPU through the oracle ops, on the GPU through the
    HIP ops -> (logits, loss, {name: grad})"""
    from oracle import torch_ops
    cpu = device.type == "cpu"
    with (torch_ops.patched_util() if cpu else contextlib.nullcontext()):
        pts, label = _cloud9(0, 2, 1024, 3)
        model = ruemonge_net.SPH3DRueMonge(ruemonge_net.small_config(1024), device=device)
        pred, _ = model(torch.from_numpy(pts).to(device), is_training=True)
        loss = model.loss(pred, torch.from_numpy(label).to(device))
        loss.backward()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters()}
    return pred.detach().cpu().numpy(), float(loss.detach()), grads


def test_model_end_to_end_vs_oracle(dev):
    """models/SPH3D_ruemonge2014.py, reduced plan, same seed-7 weights: HIP ops on the GPU against the oracle ops on the CPU —
    logits, loss and every parameter gradient, with test_model_graphs_end_to_end_vs_oracle's tolerances"""
    pred_o, loss_o, grads_o = _run_net(torch.device("cpu"))
    pred, loss, grads = _run_net(dev)
    assert pred.shape == pred_o.shape == (2, 1024, 7)
    s = max(1.0, float(np.abs(pred_o).max()))
    print("logits: max error / scale %.3e; loss %r vs %r" % (float(np.abs(pred - pred_o).max()) / s, loss, loss_o))
    np.testing.assert_allclose(pred / s, pred_o / s, rtol=0, atol=2e-3)
    assert abs(loss - loss_o) <= 2e-3 * max(1.0, abs(loss_o))
    assert grads.keys() == grads_o.keys() and any("mlp1" in n and grads[n].shape[0] == 9 for n in grads)
    for n in grads_o:
        s = max(1e-3, float(np.abs(grads_o[n]).max()))
        np.testing.assert_allclose(grads[n] / s, grads_o[n] / s, rtol=0, atol=5e-3, err_msg=n)


def _facade_pool(dev, sizes=(1500, 1024, 900, 2000)):
    blocks, normals = [], []
    for k, n in enumerate(sizes):
        pts, label = _cloud9(40 + k, 1, n, 10 + k)
        rows, nrm = facadefeed.facade_blocks(pts[0, :, 0:3], pts[0, :, 3:6], pts[0, :, 6:9], label[0])
        blocks.append(rows)
        normals.append(nrm)
    return blocks, facadefeed.FacadePool(blocks, normals, device=dev)


def test_a_training_step_consumes_the_feed_through_points_ready(dev):
    """one reduced-plan training step (forward, backward) on a FacadeFeed item handed over as `points_ready`, issued without a
    host synchronisation: the loss and every gradient are finite, and the item is the batch of its plan entry"""
    N, B, seed = 1024, 3, 21
    _blocks, p = _facade_pool(dev)
    model = ruemonge_net.SPH3DRueMonge(ruemonge_net.small_config(N), device=dev, seed=3)
    f = facadefeed.FacadeFeed(p, B, N, seed=seed, repeat=2)
    pts, label, ready = next(iter(f))
    pred, _ = model(pts, is_training=True, points_ready=ready)
    torch.cuda.current_stream().wait_event(ready)          # (the loss reads label on the main stream)
    loss = model.loss(pred, label)
    f.done(ready)
    loss.backward()
    fed = loss.detach().clone()
    torch.cuda.synchronize()
    assert pred.shape == (B, N, 7) and np.isfinite(float(fed))
    grads = [q.grad for q in model.parameters() if q.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    step, ids = facadefeed.epoch_plan(len(p), B, seed, 0, repeat=2)[0]
    pts2, label2 = facadefeed.assemble(p.rows, p.normals, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step,
                                       facadefeed.train_recipe(B))
    torch.cuda.synchronize()
    assert torch.equal(pts2.view(torch.int32), pts.view(torch.int32)) and torch.equal(label2, label)
    assert facadefeed.train_recipe(B).tolist() == [31, 28, 0] and len(f) == 3
    print("loss %r" % float(fed))


def test_the_real_network_is_evaluated(dev):
    """SPH3DRueMonge (reduced plan) in inference mode through facadeeval.evaluate: every row is counted once, the evaluation
    completes with 11 votes per row, and two runs give identical results"""
    N, seed = 1024, 9
    blocks, p = _facade_pool(dev)
    model = ruemonge_net.SPH3DRueMonge(ruemonge_net.small_config(N), device=dev, seed=3)

    def run():
        res = facadeeval.evaluate(lambda pts, l: model(pts, is_training=False)[0], p, 2, N, seed, keep_votes=True)
        torch.cuda.synchronize()
        return res
    a, b = run(), run()
    print("passes %s miou %.4f overall %.4f" % (a.passes, a.miou, a.overall_acc))
    assert a.complete and a.batches == [0, 1] and a.nonfinite_rows == 0
    assert a.confusion.shape == (7, 7) and a.confusion.sum() == sum(len(x) for x in blocks)
    assert all(c.min() >= 11 for i in a.batches for c in a.votes[i].count)
    assert a.passes == b.passes and np.array_equal(a.confusion, b.confusion) and a.miou == b.miou
    for i in a.batches:
        for x, y in zip(a.votes[i].votes + a.votes[i].count + a.votes[i].pred, b.votes[i].votes + b.votes[i].count + b.votes[i].pred):
            assert x.tobytes() == y.tobytes()


def test_the_loss_is_the_mean_cross_entropy(dev):
    """model.loss against float64 F.cross_entropy over all B * N points, within 1e-5; its gradient likewise"""
    g = torch.Generator().manual_seed(4)
    B, N, C = 3, 1000, 7
    pred = (torch.randn(B, N, C, generator=g) * 3).to(dev).requires_grad_(True)
    label = torch.randint(0, C, (B, N), generator=g).int().to(dev)
    model = ruemonge_net.SPH3DRueMonge(ruemonge_net.small_config(N), device=dev)
    loss = model.loss(pred, label)
    loss.backward()
    p64 = pred.detach().cpu().double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(p64.reshape(-1, C), label.cpu().long().reshape(-1))
    want.backward()
    want = want.detach()
    err = abs(float(loss.detach()) - float(want))
    print("loss %r, float64 %r, error %.3e" % (float(loss.detach()), float(want), err))
    assert err <= 1e-5 * max(1.0, abs(float(want)))
    gerr = float((pred.grad.cpu().double() - p64.grad).abs().max())
    assert gerr <= 1e-5 * float(p64.grad.abs().max()), gerr
    # the CPU form is the same number
    cpu = ruemonge_net.get_loss(pred.detach().cpu(), label.cpu())
    assert abs(float(cpu) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
