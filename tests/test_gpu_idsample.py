"""Keyed inverse-density sampling on the device (csrc/idsample.hip): the op equals the numpy statement bit for bit at every
launch form, it is a pure function of its key, it is registered, and GraphPlan / SPH3DS3DIS run with config.sample == 'IDS'."""
import numpy as np
import pytest
import torch

import _ids_cases
from sph3d_gcn_amd import _lib, tf_sample
from sph3d_gcn_amd.harness import idsample, s3dis_net

pytestmark = pytest.mark.gpu


def _chunk():
    return _lib.lib().sph3d_ids_sample_chunk()


def _cases():
    C = _chunk()
    return [(3, 1, 1, 1), (2, 63, 4, 63), (4, 600, 16, 100), (2, 1024, 8, 256), (1, 65536, 1, 16384),
            (2, C - 1, 2, C // 4), (2, C, 2, C // 4), (2, C + 1, 2, C + 1), (1, 2 * C + 1, 3, C // 2 + 7)]


# (seed 0, step 337, level 0, cloud 0): point 46575 draws u = 1, so E = +0 and t = +0 — the smallest key there is
_U1_KEY, _U1_POINT = (0, 337, 0), 46575


@pytest.mark.parametrize("case", range(9))
def test_op_equals_the_statement(dev, case):
    B, N, K, S = _cases()[case]
    d, c = _ids_cases.graph_inputs(B, N, K, seed=100 + case, nan_tail=case % 2 == 1)
    seed, step, level = (7 + case, 1000 * case + 3, case % 8)
    if N == 65536:
        seed, step, level = _U1_KEY
        d[0, _U1_POINT, 0], c[0, _U1_POINT] = 0.25, 1
    want = idsample.ids_reference(d, c, S, seed, step, level)
    got = tf_sample.inverse_density_sample_keyed(S, torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev), seed, step, level)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, S)
    assert np.array_equal(got.cpu().numpy(), want)
    if N == 65536:
        assert want[0, 0] == _U1_POINT
    if B > 1:
        assert np.array_equal(want[B - 1], np.arange(S))          # the cloud with all counts 0


def test_seeds_beyond_63_bits_and_unaligned_rows(dev):
    """the key is 64 unsigned bits; K % 4 != 0 and a view that is not 16-byte aligned take the scalar loads"""
    d, c = _ids_cases.graph_inputs(2, 300, 8, seed=5, nan_tail=True)
    seed, step = 0xfedcba9876543210, 0x8000000000000001
    want = idsample.ids_reference(d, c, 50, seed, step, 7)
    dd, cc = torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)
    assert np.array_equal(tf_sample.inverse_density_sample_keyed(50, dd, cc, seed, step, 7).cpu().numpy(), want)
    flat = torch.empty(d.size + 1, dtype=torch.float32, device=dev)
    shifted = flat[1:].view(2, 300, 8)
    shifted.copy_(dd)
    assert shifted.data_ptr() % 16 == 4
    l = _lib.lib()
    out = torch.empty((2, 50), dtype=torch.int32, device=dev)
    _lib.check(l.sph3d_ids_sample(2, 300, 8, 50, shifted.data_ptr(), cc.data_ptr(), seed, step, 7, out.data_ptr(), None, 0,
                                  _lib.stream_ptr()))
    assert np.array_equal(out.cpu().numpy(), want)


def test_sample_is_a_pure_function_of_its_key(dev):
    B, N, K, S = 4, 3000, 8, 500
    d, c = _ids_cases.graph_inputs(B, N, K, seed=42, nan_tail=False)
    c[B - 1] = np.maximum(c[0], 1)                                   # (no empty cloud here: every cloud's sample depends on the key)
    d[B - 1] = d[0] + np.float32(0.01)
    dd, cc = torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)
    base = tf_sample.inverse_density_sample_keyed(S, dd, cc, 9, 21, 3)
    assert torch.equal(tf_sample.inverse_density_sample_keyed(S, dd, cc, 9, 21, 3), base)
    for key in ((10, 21, 3), (9, 22, 3), (9, 21, 4)):
        other = tf_sample.inverse_density_sample_keyed(S, dd, cc, *key)
        assert all(not torch.equal(other[b], base[b]) for b in range(B)), key
    # cloud 1 of a B = 4 call equals cloud 1 of a B = 2 call on the same rows
    two = tf_sample.inverse_density_sample_keyed(S, dd[:2].contiguous(), cc[:2].contiguous(), 9, 21, 3)
    assert torch.equal(two, base[:2])
    # a non-default stream
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = tf_sample.inverse_density_sample_keyed(S, dd, cc, 9, 21, 3)
    side.synchronize()
    assert torch.equal(on_side, base)
    # the multi-chunk form as well (workspace from the stream's scratch)
    N2 = 2 * _chunk() + 5
    d2, c2 = _ids_cases.graph_inputs(2, N2, 2, seed=43, nan_tail=False)
    dd2, cc2 = torch.from_numpy(d2).to(dev), torch.from_numpy(c2).to(dev)
    b2 = tf_sample.inverse_density_sample_keyed(777, dd2, cc2, 1, 2, 0)
    with torch.cuda.stream(side):
        s2 = tf_sample.inverse_density_sample_keyed(777, dd2, cc2, 1, 2, 0)
    side.synchronize()
    assert torch.equal(s2, b2) and np.array_equal(b2.cpu().numpy(), idsample.ids_reference(d2, c2, 777, 1, 2, 0))


def test_registration(dev):
    d, c = _ids_cases.graph_inputs(2, 200, 4, seed=3, nan_tail=False)
    dd, cc = torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)
    out = torch.ops.sph3d.inverse_density_sample(dd, cc, 40, 5, 6, 1)
    assert torch.equal(out, tf_sample.inverse_density_sample_keyed(40, dd, cc, 5, 6, 1))
    torch.library.opcheck(torch.ops.sph3d.inverse_density_sample, (dd, cc, 40, 5, 6, 1), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        tf_sample.inverse_density_sample_keyed(201, dd, cc, 5, 6)
    with pytest.raises(ValueError):
        tf_sample.inverse_density_sample_keyed(40, dd, cc, 5, 6, level=8)


def _same(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _check_encoder(plan, ref, L):
    for l in range(L):
        g, r = plan.enc(l), ref.enc(l)
        for name in ("intra_idx", "intra_cnt", "filt_idx"):
            assert _same(g[name], r[name]), (l, name)
        assert np.array_equal(g["intra_dst"].cpu().numpy().view(np.int32), r["intra_dst"].numpy().view(np.int32)), l
        g, r = plan.pool(l), ref.pool(l)
        assert _same(g["inter_idx"], r["inter_idx"]) and _same(g["inter_cnt"], r["inter_cnt"]), l
        assert _same(plan.indices[l], ref.indices[l]), l
        assert _same(plan.xyz_layers[l + 1], ref.xyz_layers[l + 1]), l


@pytest.mark.parametrize("overlap", [True, False])
def test_device_plan_equals_the_cpu_plan(dev, overlap):
    key = (5, 3)
    cfg = _ids_cases.ids_config()
    L = len(cfg.radius)
    ref = _ids_cases.cpu_plan(key)
    pts = torch.from_numpy(_ids_cases.plan_batch()[0]).to(dev)
    plan = s3dis_net.build_graphs(pts, cfg, overlap=overlap, sample_key=key)
    torch.cuda.synchronize()
    assert plan.use_side == overlap
    _check_encoder(plan, ref, L)
    for l in range(L):
        g, r = plan.dec(l), ref.dec(l)
        for name in ("intra_idx", "intra_cnt", "filt_idx", "inter_idx", "inter_cnt"):
            assert _same(g[name], r[name]), (l, name)
    # the encoder-only form of the classification net: no decoder, the global graph behind the last sample
    xyz = pts[:, :, 0:3].contiguous()
    query = torch.from_numpy(_ids_cases.plan_batch()[0][:, :, 0:3].mean(axis=1, keepdims=True)).to(dev)
    enc = s3dis_net.GraphPlan(xyz, cfg, overlap=overlap, decoder=False, global_kernel=[8, 2, 1], global_query=query,
                              prepare_input=False, sample_key=key)
    glob = enc.glob()
    torch.cuda.synchronize()
    _check_encoder(enc, ref, L)
    assert not enc._dec and int(glob["nn_cnt"].min()) == cfg.num_sample[-1] == int(glob["nn_cnt"].max())
    # another key: another plan
    other = s3dis_net.GraphPlan(pts, cfg, overlap=overlap, sample_key=(5, 4))
    other.pool(0)
    torch.cuda.synchronize()
    assert not _same(other.indices[0], ref.indices[0])


def test_model_forward_backward_with_inverse_density_sampling(dev):
    cfg = _ids_cases.ids_config()
    xyz, label, inner = _ids_cases.plan_batch()
    pts, label, inner = torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    model = s3dis_net.SPH3DS3DIS(cfg, device=dev)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        plan = s3dis_net.GraphPlan(pts, cfg, sample_key=(11, 4))
        pred, _ = model(pts, is_training=True, graphs=plan)
        loss = model.loss(pred, label, inner)
        loss.backward()
        torch.cuda.synchronize()
        assert tuple(pred.shape) == (2, 1024, 13) and torch.isfinite(pred).all() and torch.isfinite(loss)
        grads = [p.grad for p in model.parameters() if p.requires_grad]
        assert all(g is not None and torch.isfinite(g).all() for g in grads)
        runs.append((plan, pred.detach().clone(), loss.detach().clone()))
    (p0, y0, l0), (p1, y1, l1) = runs
    for l in range(len(cfg.radius)):
        assert torch.equal(p0.indices[l], p1.indices[l]) and torch.equal(p0.xyz_layers[l + 1], p1.xyz_layers[l + 1])
    # one key, one graph: the two forwards differ at most by the feature path's own run-to-run arithmetic (the batch-norm
    # running statistics moved between them do not enter a training-mode forward) — the project's 1e-5 activation bound
    print("max |pred0 - pred1| = %.3g" % float((y0 - y1).abs().max()))
    assert torch.allclose(y0, y1, rtol=1e-5, atol=1e-5) and torch.allclose(l0, l1, rtol=1e-5, atol=1e-5)
    # through forward(sample_key=...) the model builds the same plan itself
    pred2, _ = model(pts, is_training=True, sample_key=(11, 4))
    torch.cuda.synchronize()
    assert torch.allclose(pred2.detach(), y0, rtol=1e-5, atol=1e-5)


def test_classification_net_plans_with_inverse_density_sampling(dev):
    """modelnet_net builds its plan for 'IDS' as for 'FPS': the encoder-only plan with the global graph, from the key"""
    import copy
    from sph3d_gcn_amd.harness import modelnet_net, synth
    cfg = copy.deepcopy(modelnet_net.small_config(1024))
    cfg.sample = 'IDS'
    pts = torch.from_numpy(synth.modelnet_batch(0, 2, 1024)).to(dev)
    model = modelnet_net.SPH3DModelNet(cfg, device=dev)
    with torch.no_grad():
        a = model(pts, is_training=False, sample_key=(2, 7))[0]
        b = model(pts, is_training=False, sample_key=(2, 7))[0]
        c = model(pts, is_training=False, sample_key=(2, 8))[0]
    torch.cuda.synchronize()
    assert tuple(a.shape) == (2, 40) and torch.isfinite(a).all()
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)          # one key, one graph (bound: as in the segmentation test above)
    assert not torch.equal(a, c)
    pred, _ = model(pts, is_training=True, sample_key=(2, 9), dropout_generator=torch.Generator().manual_seed(5))
    model.loss(pred, torch.tensor([3, 17], device=dev)).backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters() if p.requires_grad)
