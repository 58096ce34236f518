"""The fuzzy spherical kernel on the device (csrc/fuzzy.hip) against its numpy statement
(sph3d_gcn_amd/harness/fuzzy.py): the builder bit for bit, the convolution and both gradients per element within the bounds
tests/_fuzzy_ref.py derives, at every template instantiation and launch shape the launchers can reach; deterministic mode;
autograd through the layer; a reduced S3DIS plan with config.kernel_fuzzy; and the hard plan unchanged without the flag."""
import numpy as np
import pytest
import torch

import _fuzzy_ref as R
from _conv_ref import make_values
from _pool_ref import make_graph
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph, tf_buildkernel, tf_conv3d, tf_nnquery
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import fuzzy, s3dis_net, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    pkg.set_deterministic(False)
    _tgraph.clear()
    yield
    pkg.set_deterministic(False)
    _tgraph.clear()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


# ---- the kernel builder ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def searched(dev):
    """the planted cloud of the CPU test (B = 2, N = M = 256) and its sphere-search graph, K = 32"""
    xyz = R.planted_cloud(3)
    pts = _t(xyz, dev)
    idx, cnt, dst = tf_nnquery.build_sphere_neighbor(pts, pts, 0.2, None, 32)
    return xyz, pts, idx, cnt, dst


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("radius", [0.2, 0.12])                     # the smaller one: neighbours with dist > radius
def test_builder_equals_the_statement_bit_for_bit(searched, kernel, radius):
    xyz, pts, idx, cnt, dst = searched
    fi, fr = tf_buildkernel.fuzzy_spherical_kernel(pts, pts, idx, cnt, dst, radius, kernel=kernel)
    ri, rf = fuzzy.fuzzy_kernel_reference(xyz, xyz, _n(idx), _n(cnt), _n(dst), radius, kernel)
    assert fi.dtype == torch.int32 and fr.dtype == torch.int32 and tuple(fi.shape) == (2, 256, 32)
    assert np.array_equal(_n(fi), ri)
    assert np.array_equal(_n(fr), rf)
    live = np.arange(32)[None, None, :] < _n(cnt)[:, :, None]
    assert (ri[live] == 0).sum() >= 2 * 256 and (rf[live] != 0).sum() > 1000 and (ri[~live] == 0).all()
    if radius < 0.2:
        assert (live & (_n(dst) > radius)).sum() >= 100


# ---- forward and both gradients ----------------------------------------------------------------------------------------------------
def _problem(seed, B, N, M, K, C, r, kernel):
    rng = np.random.RandomState(seed)
    F = R.num_bins(kernel)
    idx, cnt = make_graph(rng, B, N, M, K)                               # rows of count 0, 1, 2, K - 1, K in every cloud
    fi, fr = R.random_words(rng, cnt, K, kernel)
    x, w, go = make_values(rng, (B, N, C)), make_values(rng, (F, C, r)), make_values(rng, (B, M, C * r))
    return idx, cnt, fi, fr, x, w, go


def _check(dev, seed, B, N, M, K, C, r, kernel, what):
    idx, cnt, fi, fr, x, w, go = _problem(seed, B, N, M, K, C, r, kernel)
    d = [_t(a, dev) for a in (x, w, idx, cnt, fi, fr, go)]
    out = tf_conv3d.fuzzy_depthwise_conv3d(d[0], d[1], d[2], d[3], d[4], d[5], kernel=kernel)
    gi, gf = tf_conv3d.fuzzy_depthwise_conv3d_grad(d[0], d[1], d[6], d[2], d[3], d[4], d[5], kernel=kernel)
    ref, mag, terms = fuzzy.fuzzy_conv_reference(x, w, idx, cnt, fi, fr, kernel)
    g = fuzzy.fuzzy_conv_grad_reference(x, w, go, idx, cnt, fi, fr, kernel)
    assert (_n(out)[cnt == 0] == 0).all()
    used = (R.assert_conv(_n(out), ref, mag, R.fwd_terms(terms), what + " forward"),
            R.assert_conv(_n(gi), g.gi, g.gi_mag, R.gi_terms(g.deg, r), what + " grad_input"),
            R.assert_conv(_n(gf), g.gf, g.gf_mag, R.gf_terms(g.gf_terms), what + " grad_filter"))
    return used


# The launchers pick <columns per lane, wave per row> by the slice's width (fuzzy_shape): <1, no> up to 32 columns (C r for the
# forward and grad_filter, C for grad_input), <1, yes> up to 64, <2, yes> up to 128, <4, yes> above.  C r of the grid: 3 .. 32,
# 64, 67 .. 128, 134 .. 384 reach all four of the first two kernels; C = 3, 4, 32 | 67, 128 three of grad_input's, the cases
# behind the grid the others (C = 48: <1, yes>; C = 300: <4, yes>)
@pytest.mark.parametrize("K", [9, 64])
@pytest.mark.parametrize("C", [3, 4, 32, 67, 128])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_conv_and_gradients_per_element(dev, K, C, r):
    kernel = R.KERNELS[(C + r + K) % 3]
    _check(dev, 1000 + 10 * C + r + K, 2, 70, 37, K, C, r, kernel, "K=%d C=%d r=%d %s" % (K, C, r, kernel))


@pytest.mark.parametrize("C,r", [(48, 1), (48, 2), (300, 1)])          # (r = 2 is a path of its own in grad_input)
def test_grad_input_channel_widths_outside_the_grid(dev, C, r):
    _check(dev, 7, 2, 70, 37, 9, C, r, R.KERNELS[0], "C=%d r=%d" % (C, r))


def test_column_sliced_table(dev):
    """F = 33, C r = 1024: the table is 135 KB, the launch runs three column slices (448, 448, 128; grad_input: 224 channels each)"""
    _check(dev, 8, 1, 40, 24, 8, 512, 2, R.KERNELS[0], "sliced C=512 r=2")


def test_widest_kernel(dev):
    """F = 257: 60 table columns per slice"""
    _check(dev, 9, 2, 30, 17, 9, 40, 2, [16, 4, 4], "F=257")


def test_gradients_repeat_bit_for_bit_in_deterministic_mode(dev):
    idx, cnt, fi, fr, x, w, go = _problem(21, 2, 70, 300, 64, 32, 2, R.KERNELS[0])       # sources with hundreds of in-edges
    runs = []
    with pkg.deterministic():
        for _ in range(2):
            _tgraph.clear()                                   # the edge lists are rebuilt: another arrival order, sorted again
            d = [_t(a, dev) for a in (x, w, go, idx, cnt, fi, fr)]
            gi, gf = tf_conv3d.fuzzy_depthwise_conv3d_grad(*d, kernel=R.KERNELS[0])
            off, ent = _tgraph.transpose_edges(d[3], d[4], 70)
            off, ent = _n(off), _n(ent).copy()
            for b in range(2):                                # (the slab's tail, the slots k >= nn_count, is not written)
                ent[off[b * 71 + 70]:(b + 1) * 300 * 64] = -1
            runs.append((_n(gi).view(np.int32), _n(gf).view(np.int32), off, ent))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # the lists are in canonical order: ascending edge id, and they name exactly the source's in-edges
    off, ent = runs[0][2].reshape(2, 71), runs[0][3]
    for b in range(2):
        for n in range(70):
            e = ent[off[b, n]:off[b, n + 1]].astype(np.int64)
            assert (np.diff(e) > 0).all()
            m, k = e // 64, e % 64
            assert (idx[b, m, k] == n).all() and (k < cnt[b, m]).all()
        assert off[b, 70] - off[b, 0] == np.minimum(cnt[b], 64).sum()


def test_autograd_through_separable_conv3d_with_a_pair(dev):
    kernel = R.KERNELS[0]
    idx, cnt, fi, fr, x, w, go = _problem(31, 2, 70, 37, 9, 8, 2, kernel)
    d_idx, d_cnt, d_fi, d_fr = (_t(a, dev) for a in (idx, cnt, fi, fr))
    xa = _t(x[:, :, :5], dev).requires_grad_(True)
    xb = _t(x[:, :, 5:], dev).requires_grad_(True)
    store = s3g_util.VariableStore(device=dev, seed=3)
    with s3g_util.variable_store(store):
        out = s3g_util.separable_conv3d((xa, xb), 12, R.num_bins(kernel), 2, "layer", d_idx, d_cnt, (d_fi, d_fr, kernel),
                                        with_bn=False, with_bias=True, is_training=True)
    names = [n for n, _ in store.named_parameters()]
    assert len(names) == 3 and "depthwise" in names[0]                  # depthwise weights, weights, biases: the hard layer's order
    params = dict(store.named_parameters())
    dw = [p for n, p in params.items() if "depthwise" in n][0]
    pw = [p for n, p in params.items() if "depthwise" not in n and p.dim() == 2][0]
    bias = [p for n, p in params.items() if p.dim() == 1][0]
    seed = torch.randn_like(out)
    grads = torch.autograd.grad(out, [xa, xb, dw, pw], seed)
    # the composed ops
    xc = torch.cat((xa, xb), dim=2).detach().requires_grad_(True)
    dw2, pw2 = dw.detach().clone().requires_grad_(True), pw.detach().clone().requires_grad_(True)
    mid = tf_conv3d.fuzzy_depthwise_conv3d(xc, dw2, d_idx, d_cnt, d_fi, d_fr, kernel=kernel)
    out2 = torch.nn.functional.elu(torch.matmul(mid.reshape(-1, 16), pw2) + bias.detach()).reshape(2, 37, 12)
    np.testing.assert_allclose(_n(out), _n(out2), rtol=1e-5, atol=1e-6)
    g2 = torch.autograd.grad(out2, [xc, dw2, pw2], seed)
    np.testing.assert_allclose(_n(torch.cat(grads[:2], dim=2)), _n(g2[0]), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_n(grads[2]), _n(g2[1]), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_n(grads[3]), _n(g2[2]), rtol=1e-4, atol=1e-5)
    # and the registered custom op: same bits as the eager function, a fake for tracing
    reg = torch.ops.sph3d.fuzzy_depthwise_conv3d(xc.detach(), dw2.detach(), d_idx, d_cnt, d_fi, d_fr, *kernel)
    assert torch.equal(reg, mid.detach())
    with pytest.raises(ValueError):
        tf_conv3d.fuzzy_depthwise_conv3d(xc, dw2, d_idx, d_cnt, d_fi, d_fr, kernel=[4, 2, 2])


# ---- the model plans ---------------------------------------------------------------------------------------------------------------
def _batch(dev):
    xyz, label, inner = synth.s3dis_batch(0, 2, 1024, extent=(1.0, 1.0, 1.5))
    return _t(xyz, dev), _t(label, dev), _t(inner, dev)


def test_reduced_s3dis_plan_with_kernel_fuzzy_trains(dev):
    pts, label, inner = _batch(dev)
    cfg = s3dis_net.small_config(1024)
    cfg.kernel_fuzzy = True
    model = s3dis_net.SPH3DS3DIS(cfg, device=dev)
    graphs = s3dis_net.build_graphs(pts, model.config)
    g0 = graphs.enc(0)
    assert isinstance(g0["filt_idx"], tuple) and len(g0["filt_idx"]) == 2
    ri, rf = fuzzy.fuzzy_kernel_reference(_n(graphs.xyz_layers[0]), _n(graphs.xyz_layers[0]), _n(g0["intra_idx"]), _n(g0["intra_cnt"]),
                                          _n(tf_nnquery.build_sphere_neighbor(graphs.xyz_layers[0], graphs.xyz_layers[0], cfg.radius[0],
                                                                              None, cfg.nn_uplimit[0])[2]), cfg.radius[0], cfg.kernel)
    assert np.array_equal(_n(g0["filt_idx"][0]), ri) and np.array_equal(_n(g0["filt_idx"][1]), rf)
    # the plan prebuilt the edge-id transpose, not the binned one
    keys = list(_tgraph._cache.keys())
    assert any(k[0] == "edges" for k in keys) and not any(k[0] != "edges" and k[5] == cfg.binSize for k in keys)
    pred, _ = model(pts, is_training=True, graphs=graphs)
    loss = model.loss(pred, label, inner)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(pred).all()
    filters = [(n, p) for n, p in model.named_parameters() if "depthwise_weights" in n]
    assert len(filters) >= 4
    for n, p in filters:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    before = [p.detach().clone() for _, p in filters]
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, (_, p) in zip(before, filters))


def test_hard_plan_is_unchanged_without_the_flag(dev):
    """flag absent or False: the plan's tensors and the model's output are those of the hard ops called directly"""
    pts, label, inner = _batch(dev)
    outs = []
    for flag in (None, False):
        _tgraph.clear()
        cfg = s3dis_net.small_config(1024)
        if flag is not None:
            cfg.kernel_fuzzy = flag
        model = s3dis_net.SPH3DS3DIS(cfg, device=dev)
        graphs = s3dis_net.build_graphs(pts, model.config)
        for l in range(2):
            g = graphs.enc(l)
            xyz = graphs.xyz_layers[l]
            idx, cnt, dst = tf_nnquery.build_sphere_neighbor(xyz, xyz, cfg.radius[l], None, cfg.nn_uplimit[l])
            filt = tf_buildkernel.spherical_kernel(xyz, xyz, idx, cnt, dst, cfg.radius[l], kernel=cfg.kernel)
            assert torch.is_tensor(g["filt_idx"]) and torch.equal(g["filt_idx"], filt)
            assert torch.equal(g["intra_idx"], idx) and torch.equal(g["intra_cnt"], cnt)
        keys = list(_tgraph._cache.keys())
        assert not any(k[0] == "edges" for k in keys) and any(k[5] == cfg.binSize for k in keys)
        pred, _ = model(pts, is_training=True, graphs=graphs)
        loss = model.loss(pred, label, inner)
        loss.backward()
        grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        outs.append((pred.detach().clone(), loss.detach().clone(), grads))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # first-layer activation: the depthwise op on the plan's tensors equals the op on directly computed bins
    g = graphs.enc(0)
    x = torch.randn(2, 1024, 16, device=dev)
    w = torch.randn(cfg.binSize, 16, 2, device=dev)
    xyz = graphs.xyz_layers[0]
    idx, cnt, dst = tf_nnquery.build_sphere_neighbor(xyz, xyz, cfg.radius[0], None, cfg.nn_uplimit[0])
    filt = tf_buildkernel.spherical_kernel(xyz, xyz, idx, cnt, dst, cfg.radius[0], kernel=cfg.kernel)
    assert torch.equal(tf_conv3d.depthwise_conv3d(x, w, g["intra_idx"], g["intra_cnt"], g["filt_idx"]),
                       tf_conv3d.depthwise_conv3d(x, w, idx, cnt, filt))
