"""The last un-pooling behind the logits product (s3g_util.unpool_logits): interp(x) @ W == interp(x @ W).

The product runs on the coarse points and the interpolation moves num_cls-wide rows (sph3d_interpolate_narrow, 16 lanes per
row).  Checked against cat(interp(net), skip) @ W + b in float64, forward and all four gradients, with the error of the
unfused path (FUSE_UNPOOL_LOGITS = False) against the same reference as the yardstick: only the order of summation differs."""
import numpy as np
import pytest
import torch

from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd import tf_unpool3d
from sph3d_gcn_amd.harness import s3dis_net, synth

pytestmark = pytest.mark.gpu

K_SMALL = 8
C_COARSE = 20
EPS = 2.0 ** -23
# B, Nf, Mc, K.  "wide": more than one 16-id chunk per row (the headline plan has 64 slots): counts 17, 33 and 40 among the rows
GRAPH_DIMS = {"small": (2, 96, 24, K_SMALL), "hub": (2, 300, 3, K_SMALL), "wide": (2, 80, 48, 40)}
NUM_CLS = [1, 13, 16]


def _graph(kind, seed):
    """-> nn_index [B, Nf, K] i32, nn_count [B, Nf] i32, nn_dist [B, Nf, K] f32, Mc.  The last coarse point has no in-edge;
    slots past a row's count name that point (a valid id nobody may read)."""
    rng = np.random.RandomState(seed)
    B, Nf, Mc, K = GRAPH_DIMS[kind]
    idx = np.full((B, Nf, K), Mc - 1, np.int32)
    cnt = np.zeros((B, Nf), np.int32)
    top = min(K, Mc - 1)
    first = (0, 1, top, 17, 33, 16, 32) if kind == "wide" else (0, 1, top)
    for b in range(B):
        for n in range(Nf):
            c = first[n] if n < len(first) else int(rng.randint(0, top + 1))
            cnt[b, n] = c
            idx[b, n, :c] = rng.permutation(Mc - 1)[:c]
    dist = (rng.rand(B, Nf, K) * 0.1 + 0.01).astype(np.float32)
    if kind == "small":
        assert {0, 1, K} <= set(cnt.ravel().tolist())
    elif kind == "wide":
        assert {0, 1, 17, 33, 40} <= set(cnt.ravel().tolist())
    else:       # a hub: one coarse point collects more than 64 fine points of a cloud
        live = np.arange(K)[None, :] < cnt[0][:, None]
        assert int((idx[0][live] == 0).sum()) > 64
    return idx, cnt, dist, Mc


def _weights(method, cnt, dist32):
    """[B, Nf, K] float64 factors of the interpolation (zero past the count); dist32: the fp32 weights both paths compute"""
    Kk = dist32.shape[-1]
    mask = (torch.arange(Kk, device=cnt.device)[None, None, :] < cnt[:, :, None]).double()
    if method == "mean":
        return mask / cnt.clamp(min=1)[:, :, None].double()
    w32 = (dist32 + 1e-7) / (torch.sum(dist32, dim=-1, keepdim=True) + 1e-7)       # s3g_util.unpool3d, in fp32 like both paths
    return w32.double() * mask


def _reference(net, skip, W, b, idx, fac, dL):
    """cat(interp(net), skip) @ W + b in float64 -> (out, d net, d skip, dW, db)"""
    net, W, b = (t.clone().requires_grad_(True) for t in (net, W, b))
    skip = None if skip is None else skip.clone().requires_grad_(True)
    B = net.shape[0]
    rows = net[torch.arange(B, device=net.device)[:, None, None], idx.long()]            # [B, Nf, K, C]
    feat = (rows * fac[..., None]).sum(2)
    if skip is not None:
        feat = torch.cat((feat, skip), dim=2)
    out = feat @ W + b
    out.backward(dL)
    return [out.detach(), net.grad, None if skip is None else skip.grad, W.grad, b.grad]


def _run(fused, method, net, skip, W, b, idx, cnt, dist, dL):
    dev = net.device
    saved = s3g_util.FUSE_UNPOOL_LOGITS
    s3g_util.FUSE_UNPOOL_LOGITS = fused
    try:
        store = s3g_util.VariableStore(device=dev, seed=1)
        net = net.clone().requires_grad_(True)
        skip = None if skip is None else skip.clone().requires_grad_(True)
        with s3g_util.variable_store(store):
            def layer():
                return s3g_util.unpool_logits(net, idx, cnt, dist, skip, W.shape[1], 'logits', method, with_bn=False, with_bias=True,
                                              activation_fn=None, is_training=True)
            layer()                                             # creates the variables
            names = [n for n, _ in store.named_parameters()]
            assert names == ['params.logits/weights', 'params.logits/biases']
            with torch.no_grad():
                store.params['logits/weights'].copy_(W)
                store.params['logits/biases'].copy_(b)
            out = layer()
        out.backward(dL)
        torch.cuda.synchronize()
        return [out.detach(), net.grad, None if skip is None else skip.grad, store.params['logits/weights'].grad,
                store.params['logits/biases'].grad]
    finally:
        s3g_util.FUSE_UNPOOL_LOGITS = saved


def _rel_err(got, ref, terms):
    """max |got - ref| / sum |terms| over the elements (an element without terms must be exact)"""
    err = (got.double() - ref).abs()
    assert bool((err[terms == 0] == 0).all())
    return float((err / terms.clamp(min=1e-300)).max())


def _check_against_float64(dev, kind, method, c_coarse, c_skip, num_cls):
    idx_n, cnt_n, dist_n, Mc = _graph(kind, 11)
    B, Nf = cnt_n.shape
    g = torch.Generator().manual_seed(num_cls * 100 + c_skip)
    net = torch.randn(B, Mc, c_coarse, generator=g).to(dev)
    skip = torch.randn(B, Nf, c_skip, generator=g).to(dev) if c_skip else None
    W = torch.randn(c_coarse + c_skip, num_cls, generator=g).to(dev)
    b = torch.randn(num_cls, generator=g).to(dev)
    dL = torch.randn(B, Nf, num_cls, generator=g).to(dev)
    idx, cnt, dist = (torch.from_numpy(a).to(dev) for a in (idx_n, cnt_n, dist_n))
    fac = _weights(method, cnt, dist)
    d = lambda t: None if t is None else t.double()
    ref = _reference(d(net), d(skip), d(W), d(b), idx, fac, d(dL))
    terms = _reference(d(net).abs(), None if skip is None else d(skip).abs(), d(W).abs(), d(b).abs(), idx, fac, d(dL).abs())
    new = _run(True, method, net, skip, W, b, idx, cnt, dist, dL)
    old = _run(False, method, net, skip, W, b, idx, cnt, dist, dL)
    for name, n_, o_, r_, t_ in zip(("logits", "d_net", "d_skip", "dW", "db"), new, old, ref, terms):
        if r_ is None:
            assert n_ is None and o_ is None
            continue
        assert n_.shape == r_.shape and n_.dtype == torch.float32
        e_new, e_old = _rel_err(n_, r_, t_), _rel_err(o_, r_, t_)
        print("%s %s skip=%d cls=%d %-6s fused %.3e unfused %.3e" % (kind, method, c_skip, num_cls, name, e_new, e_old))
        assert e_new <= 2.0 * e_old + EPS, name
    # the coarse point without in-edges receives no gradient
    assert bool((new[1][:, Mc - 1] == 0).all())


@pytest.mark.parametrize("num_cls", NUM_CLS)
@pytest.mark.parametrize("c_skip", [0, 12])
@pytest.mark.parametrize("method", ["mean", "weighted"])
@pytest.mark.parametrize("kind", ["small", "hub"])
def test_unpool_logits_against_float64(dev, kind, method, c_skip, num_cls):
    """forward and the four gradients: error of the fused path <= 2 x error of the unfused path + 2^-23, both measured here
    against float64 as max |err| / sum |terms|"""
    _check_against_float64(dev, kind, method, C_COARSE, c_skip, num_cls)


@pytest.mark.parametrize("chans", [(32, 16), (32, 0), (20, 12)], ids=lambda c: "C%d-S%d" % c)
@pytest.mark.parametrize("method", ["mean", "weighted"])
@pytest.mark.parametrize("kind", ["small", "wide"])
def test_unpool_logits_against_float64_hot_path_shapes(dev, kind, method, chans):
    """the same bound where the run takes the paths of the headline plan: rows of more than 16 neighbours (several chunks of
    ids per row, odd and even tails) and channel counts the few-output product kernels cover (multiples of 16), whose weight
    gradients are written into the two row ranges of one tensor"""
    from sph3d_gcn_amd import tf_gemm
    Nf = {"small": 96, "wide": 80}[kind]
    if chans[0] % 16 == 0:
        assert tf_gemm.skinny_supported(2 * Nf, chans[0], chans[1], 13) and tf_gemm.skinny_supported(2 * Nf, chans[0], 0, 13)
    _check_against_float64(dev, kind, method, chans[0], chans[1], 13)


@pytest.mark.parametrize("chans", [(C_COARSE, 0), (C_COARSE, 12), (32, 16)], ids=lambda c: "C%d-S%d" % c)
@pytest.mark.parametrize("method", ["mean", "weighted"])
@pytest.mark.parametrize("kind", ["small", "hub", "wide"])
def test_selecting_projection_is_exact_and_empty_rows_keep_base(dev, kind, method, chans):
    """a W whose columns each select one channel and unit weights: the fused forward equals the separate ops bit for bit; rows
    without neighbours equal the skip half's product (with bias) bit for bit"""
    c_coarse, c_skip = chans
    idx_n, cnt_n, _dist, Mc = _graph(kind, 5)
    B, Nf = cnt_n.shape
    K = idx_n.shape[2]
    num_cls = 13
    g = torch.Generator().manual_seed(3 + c_skip)
    net = torch.randn(B, Mc, c_coarse, generator=g).to(dev)
    skip = torch.randn(B, Nf, c_skip, generator=g).to(dev) if c_skip else None
    b = torch.randn(num_cls, generator=g).to(dev)
    sel = torch.randperm(c_coarse + c_skip, generator=g)[:num_cls]
    W = torch.zeros(c_coarse + c_skip, num_cls)
    W[sel, torch.arange(num_cls)] = 1.0
    W = W.to(dev)
    idx, cnt = torch.from_numpy(idx_n).to(dev), torch.from_numpy(cnt_n).to(dev)
    ones = torch.ones(B, Nf, K, device=dev) if method == "weighted" else None
    fused = tf_unpool3d.interpolate_linear(net, skip, W, b, idx, cnt, weight=ones)
    feat = tf_unpool3d.mean_interpolate(net, idx, cnt) if ones is None else tf_unpool3d.weighted_interpolate(net, ones, idx, cnt)
    saved = s3g_util.FUSE_UNPOOL_LOGITS
    s3g_util.FUSE_UNPOOL_LOGITS = False
    try:
        store = s3g_util.VariableStore(device=dev, seed=1)
        with s3g_util.variable_store(store), torch.no_grad():
            def layer():
                if skip is None:
                    return s3g_util.pointwise_conv3d(feat, num_cls, 'logits', with_bn=False, with_bias=True, activation_fn=None)
                return s3g_util.pointwise_conv3d_concat(feat, skip, num_cls, 'logits', with_bn=False, with_bias=True, activation_fn=None)
            layer()
            store.params['logits/weights'].copy_(W)
            store.params['logits/biases'].copy_(b)
            separate = layer()
    finally:
        s3g_util.FUSE_UNPOOL_LOGITS = saved
    assert torch.equal(fused, separate)
    # rows without neighbours: the base row, bit for bit (also under a random projection)
    W2 = torch.randn(c_coarse + c_skip, num_cls, generator=g).to(dev)
    out = tf_unpool3d.interpolate_linear(net, skip, W2, b, idx, cnt, weight=ones)
    if skip is None:
        base = b.expand(B, Nf, num_cls)
    else:
        base = tf_unpool3d._product(skip.reshape(B * Nf, c_skip), W2[c_coarse:], b).reshape(B, Nf, num_cls)
    empty = cnt == 0
    assert int(empty.sum()) >= B
    assert torch.equal(out[empty].view(torch.int32), base[empty].contiguous().view(torch.int32))


def test_s3dis_reduced_plan_fused_tail_equals_unfused(dev):
    """the reduced S3DIS plan with the fused logits tail against the plan without it: same variables in the same order, loss and
    flat gradient within the tolerance tests/test_gpu_parity.py uses for this plan (2e-3 / 5e-3 of the scale)"""
    cfg = s3dis_net.small_config(1024)
    xyz, label, inner = synth.s3dis_batch(0, 2, 1024, extent=(1.0, 1.0, 1.5))
    pts, label, inner = (torch.from_numpy(a).to(dev) for a in (xyz, label, inner))

    def run(fused):
        s3g_util.FUSE_UNPOOL_LOGITS = fused
        model = s3dis_net.SPH3DS3DIS(cfg, device=dev)
        pred, end = model(pts, is_training=True)
        loss = model.loss(pred, label, inner)
        loss.backward()
        names = [n for n, _ in model.named_parameters()]
        flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
        return pred.detach(), float(loss.detach()), names, flat, end['feats'].detach()

    try:
        pf, lf, nf, gf, ff = run(True)
        pu, lu, nu, gu, fu = run(False)
    finally:
        s3g_util.FUSE_UNPOOL_LOGITS = True
    assert nf == nu
    assert ff.shape == fu.shape == (2, 1024, 2 * cfg.channels[0][0]) and torch.equal(ff, fu)     # end_points['feats'] stays available
    s = max(1.0, float(pu.abs().max()))
    assert float((pf - pu).abs().max()) / s <= 2e-3
    assert abs(lf - lu) <= 2e-3 * max(1.0, abs(lu))
    s = max(1e-3, float(gu.abs().max()))
    print("loss fused %.7f unfused %.7f; flat gradient max |diff| / scale %.3e" % (lf, lu, float((gf - gu).abs().max()) / s))
    assert float((gf - gu).abs().max()) / s <= 5e-3


def plan_cases():
    """-> [(B, Nf, Mc, C, K)] of the narrow interpolation (mean and weighted) and its gradient behind the fused tails above"""
    cases = [(kind, C) for kind in ("small", "hub") for C in NUM_CLS] + [(kind, 13) for kind in GRAPH_DIMS]
    return [GRAPH_DIMS[kind][:3] + (C, GRAPH_DIMS[kind][3]) for kind, C in cases]
