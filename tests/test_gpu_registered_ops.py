"""The ``torch.ops.sph3d.*`` registrations: every op is callable through the dispatcher, agrees with the public function of
the mirrored module (which takes an eager fast path around the dispatcher), has a consistent schema / fake kernel /
autograd registration (``torch.library.opcheck``), and its registered gradient equals the fast path's: both come from one
statement (``_op.differentiable``), and the comparison runs over ``_op.WIRED``, the list of ops wired that way.  Plus the two
RNG samplers of tf_sample.py and the 'IDS' / 'random' branches of build_graph."""
import numpy as np
import pytest
import torch

import oracle
from sph3d_gcn_amd import (_op, _tgraph, tf_nnquery, tf_buildkernel, tf_conv3d, tf_pool3d, tf_unpool3d, tf_sample, tf_gemm, tf_norm,
                           sph3gcn_util as s3g_util)
from sph3d_gcn_amd.harness import synth

pytestmark = pytest.mark.gpu
CHECKS = ("test_schema", "test_faketensor", "test_autograd_registration")


def _graph(dev, B=2, N=120, M=50, K=12, r=0.3):
    db = torch.from_numpy(synth.uniform_cloud(3, B, N)).to(dev)
    q = db[:, :M].contiguous()
    idx, cnt, dst = tf_nnquery.build_sphere_neighbor(db, q, r, None, K)
    filt = tf_buildkernel.spherical_kernel(db, q, idx, cnt, dst, r, [8, 2, 2])
    return db, q, idx, cnt, dst, filt


def test_graph_ops_through_the_dispatcher(dev):
    db, q, idx, cnt, dst, filt = _graph(dev)
    i2, c2, d2 = torch.ops.sph3d.build_sphere_neighbor(db, q, 0.3, 12)
    assert torch.equal(i2, idx) and torch.equal(c2, cnt) and torch.equal(d2, dst)
    f2 = torch.ops.sph3d.spherical_kernel(db, q, idx, cnt, dst, 0.3, 8, 2, 2)
    assert torch.equal(f2, filt)
    ci, cc = torch.ops.sph3d.build_cube_neighbor(db, q, 0.3, 12, 3)
    ri, rc = tf_nnquery.build_cube_neighbor(db, q, 0.3, None, 12, 3)
    assert torch.equal(ci, ri) and torch.equal(cc, rc)
    s = torch.ops.sph3d.farthest_point_sample(db, 17)
    assert torch.equal(s, tf_sample.farthest_point_sample(17, db))
    for op, args in ((torch.ops.sph3d.build_sphere_neighbor, (db, q, 0.3, 12)),
                     (torch.ops.sph3d.spherical_kernel, (db, q, idx, cnt, dst, 0.3, 8, 2, 2)),
                     (torch.ops.sph3d.build_cube_neighbor, (db, q, 0.3, 12, 3)),
                     (torch.ops.sph3d.farthest_point_sample, (db, 17))):
        torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))


def _grads(fn, inputs, go):
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    out = out[0] if isinstance(out, tuple) else out
    out.backward(go)
    return out.detach(), [t.grad for t in leaves]


def _feature_cases(dev):
    """registered op's name -> (through the dispatcher, the public function, differentiable inputs, output shape), on _graph's shapes"""
    db, q, idx, cnt, dst, filt = _graph(dev)
    fi, ff = tf_buildkernel.fuzzy_spherical_kernel(db, q, idx, cnt, dst, 0.3, kernel=[8, 2, 2])
    B, N, M, K, C, r = 2, 120, 50, 12, 8, 2
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(B, N, C, generator=g).to(dev)
    w = torch.randn(33, C, r, generator=g).to(dev)
    wt = torch.rand(B, M, K, generator=g).to(dev)
    x2, w2 = torch.randn(300, 20, generator=g).to(dev), torch.randn(20, 12, generator=g).to(dev)
    ops = torch.ops.sph3d
    cases = {
        "sph3d::depthwise_conv3d": (lambda a, b: ops.depthwise_conv3d(a, b, idx, cnt, filt),
                                    lambda a, b: tf_conv3d.depthwise_conv3d(a, b, idx, cnt, filt), (x, w), (B, M, C * r)),
        "sph3d::fuzzy_depthwise_conv3d": (lambda a, b: ops.fuzzy_depthwise_conv3d(a, b, idx, cnt, fi, ff, 8, 2, 2),
                                          lambda a, b: tf_conv3d.fuzzy_depthwise_conv3d(a, b, idx, cnt, fi, ff, kernel=[8, 2, 2]),
                                          (x, w), (B, M, C * r)),
        "sph3d::max_pool3d": (lambda a: ops.max_pool3d(a, idx, cnt), lambda a: tf_pool3d.max_pool3d(a, idx, cnt), (x,), (B, M, C)),
        "sph3d::avg_pool3d": (lambda a: ops.avg_pool3d(a, idx, cnt), lambda a: tf_pool3d.avg_pool3d(a, idx, cnt), (x,), (B, M, C)),
        "sph3d::mean_interpolate": (lambda a: ops.mean_interpolate(a, idx, cnt), lambda a: tf_unpool3d.mean_interpolate(a, idx, cnt),
                                    (x,), (B, M, C)),
        "sph3d::weighted_interpolate": (lambda a: ops.weighted_interpolate(a, wt, idx, cnt),
                                        lambda a: tf_unpool3d.weighted_interpolate(a, wt, idx, cnt), (x,), (B, M, C)),
        "sph3d::pointwise_gemm": (lambda a, b: ops.pointwise_gemm(a, b, False), tf_gemm.matmul, (x2, w2), (300, 12)),
    }
    return cases, (idx, cnt, filt, fi, ff, x, w, wt, g)


def test_every_wired_op_has_a_case(dev):
    cases, _ = _feature_cases(dev)
    assert len(_op.WIRED) == 7 and sorted(op._qualname for op, _ in _op.WIRED) == sorted(cases)


def test_feature_ops_registered_gradients_equal_fast_path(dev):
    B, N, M, K, C, r = 2, 120, 50, 12, 8, 2
    cases, (idx, cnt, filt, fi, ff, x, w, wt, g) = _feature_cases(dev)
    for op, _apply in _op.WIRED:                     # every op wired through _op.differentiable: an eighth cannot go uncompared
        name = op._qualname
        reg, fast, inputs, oshape = cases[name]
        go = torch.randn(*oshape, generator=g).to(dev)
        o1, g1 = _grads(reg, inputs, go)
        o2, g2 = _grads(fast, inputs, go)
        torch.testing.assert_close(o1, o2, rtol=0, atol=0)
        assert len(g1) == len(g2) == len(inputs)
        for a, b in zip(g1, g2):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=lambda m: "%s: %s" % (name, m))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    torch.library.opcheck(torch.ops.sph3d.depthwise_conv3d, (xr, wr, idx, cnt, filt), test_utils=CHECKS)
    torch.library.opcheck(torch.ops.sph3d.max_pool3d, (xr, idx, cnt), test_utils=CHECKS)
    torch.library.opcheck(torch.ops.sph3d.avg_pool3d, (xr, idx, cnt), test_utils=CHECKS)
    torch.library.opcheck(torch.ops.sph3d.mean_interpolate, (xr, idx, cnt), test_utils=CHECKS)
    torch.library.opcheck(torch.ops.sph3d.weighted_interpolate, (xr, wt, idx, cnt), test_utils=CHECKS)
    go = torch.randn(B, M, C * r, generator=g).to(dev)
    torch.library.opcheck(torch.ops.sph3d.depthwise_conv3d_grad, (x, w, go, idx, cnt, filt), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.sph3d.fuzzy_depthwise_conv3d, (xr, wr, idx, cnt, fi, ff, 8, 2, 2), test_utils=CHECKS)


def test_registered_max_pool_takes_the_gather_where_the_public_function_does(dev):
    """with a transposed pooling graph whose builder promised unique rows, both paths run the atomics-free gather: the same bits"""
    db, q, idx, cnt, dst, filt = _graph(dev)
    B, N, M, C = 2, 120, 50, 8
    g = torch.Generator(device="cpu").manual_seed(2)
    x = torch.randn(B, N, C, generator=g).to(dev)
    go = torch.randn(B, M, C, generator=g).to(dev)
    _tgraph.transpose(idx, cnt, N, unique_rows=True)
    assert tf_pool3d._gather_form(x, idx, cnt)[0] == "t"
    o1, (g1,) = _grads(lambda a: torch.ops.sph3d.max_pool3d(a, idx, cnt), (x,), go)
    o2, (g2,) = _grads(lambda a: tf_pool3d.max_pool3d(a, idx, cnt), (x,), go)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    # (and it is the pooling gradient: every output's gradient lands on its winner)
    want = torch.zeros(B, N, C, dtype=torch.float64, device=dev)
    _, arg = tf_pool3d.max_pool3d(x, idx, cnt)
    want.scatter_add_(1, arg.long(), go.double())
    torch.testing.assert_close(g1.double(), want, rtol=1e-6, atol=1e-6)


def test_registered_max_pool_follows_deterministic_mode(dev):
    """deterministic mode, no transposed pooling graph with unique rows and no row link: backward refuses on the host, through the
    dispatcher as through the public function, before anything is launched for the gradient"""
    with _tgraph.deterministic():
        db, q, idx, cnt, dst, filt = _graph(dev)
        x = torch.randn(2, 120, 8, device=dev)
        assert tf_pool3d._gather_form(x, idx, cnt) is None
        for fn in (torch.ops.sph3d.max_pool3d, tf_pool3d.max_pool3d):
            out, _ = fn(x.clone().requires_grad_(True), idx, cnt)
            with pytest.raises(RuntimeError, match="deterministic mode is on"):
                out.backward(torch.ones_like(out))


def test_gemm_and_elu_bn_registered(dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(300, 20, generator=g).to(dev)
    w = torch.randn(20, 12, generator=g).to(dev)
    go = torch.randn(300, 12, generator=g).to(dev)
    o1, g1 = _grads(lambda a, b: torch.ops.sph3d.pointwise_gemm(a, b, False), (x, w), go)
    o2, g2 = _grads(tf_gemm.matmul, (x, w), go)
    torch.testing.assert_close(o1, o2, rtol=0, atol=0)
    for a, b in zip(g1, g2):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    torch.testing.assert_close(o1, x.double().matmul(w.double()).float(), rtol=1e-5, atol=1e-5)
    torch.library.opcheck(torch.ops.sph3d.pointwise_gemm, (x.clone().requires_grad_(True), w.clone().requires_grad_(True), False),
                          test_utils=CHECKS)
    torch.library.opcheck(torch.ops.sph3d.pointwise_gemm_tn, (x, go), test_utils=("test_schema", "test_faketensor"))
    # fused ELU + batch norm
    C = 16
    y = torch.randn(4, 50, C, generator=g).to(dev)
    gamma, beta = torch.rand(C, generator=g).to(dev) + 0.5, torch.randn(C, generator=g).to(dev)
    dout = torch.randn(4, 50, C, generator=g).to(dev)

    mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    out_r, sm, sr = torch.ops.sph3d.elu_bn(y, gamma, beta, mm, mv, True)              # forward through the dispatcher
    dy_r, dg_r, db_r = torch.ops.sph3d.elu_bn_grad(y, dout, gamma, sm, sr, True)       # its (functional) gradient op
    mm2, mv2 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    leaves = [t.detach().clone().requires_grad_(True) for t in (y, gamma, beta)]
    out_f = tf_norm.elu_batch_norm(leaves[0], leaves[1], leaves[2], mm2, mv2, True)  # public fast path
    out_f.backward(dout)
    torch.testing.assert_close(out_r, out_f.detach(), rtol=0, atol=0)
    for p_, q_ in zip((dy_r, dg_r, db_r), (t.grad for t in leaves)):
        torch.testing.assert_close(p_, q_, rtol=0, atol=0)
    torch.testing.assert_close(mm, mm2, rtol=0, atol=0)
    torch.testing.assert_close(mv, mv2, rtol=0, atol=0)
    torch.library.opcheck(torch.ops.sph3d.elu_bn_grad, (y, dout, gamma, sm, sr, True), test_utils=("test_schema", "test_faketensor"))
    a = (out_r,)
    ref = torch.nn.functional.batch_norm(torch.nn.functional.elu(y).reshape(-1, C), None, None, gamma, beta, True, 0.01, 1e-3)
    torch.testing.assert_close(a[0].reshape(-1, C), ref, rtol=1e-5, atol=1e-5)


def test_random_samplers_and_build_graph_branches(dev):
    """a14: inverse_density_sample (Gumbel top-k: distinct ids, favours large weights), random_sample (uniform with
    replacement), and build_graph's 'IDS' probability = sum of the neighbours' sqrt-distances / neighbour count."""
    B, N, K, S = 4, 600, 16, 100
    xyz = torch.from_numpy(synth.uniform_cloud(9, B, N)).to(dev)
    torch.manual_seed(0)
    prob = torch.rand(B, N, device=dev) + 1e-3
    prob[:, :50] = 0.0                                            # zero weight: never drawn
    prob[0, 50] = float("nan")                                    # 0/0 of an empty row: treated as zero weight
    idx = tf_sample.inverse_density_sample(S, prob)
    assert idx.dtype == torch.int32 and idx.shape == (B, S)
    for b in range(B):
        ids = idx[b].tolist()
        assert len(set(ids)) == S and min(ids) >= 50 and max(ids) < N
    assert 50 not in idx[0].tolist()
    heavy = torch.full((1, N), 1e-6, device=dev)
    heavy[0, 100:110] = 1.0                                       # ten dominant points are (almost) always among the first draws
    hits = sum(len(set(tf_sample.inverse_density_sample(10, heavy)[0].tolist()) & set(range(100, 110))) for _ in range(20))
    assert hits >= 190
    r = tf_sample.random_sample(5000, xyz)
    assert r.dtype == torch.int32 and r.shape == (B, 5000) and int(r.min()) >= 0 and int(r.max()) < N
    counts = torch.bincount(r[0].long(), minlength=N).float()
    assert counts.std() < 3 * (5000 / N) ** 0.5 and counts.max() < 40          # uniform: Poisson(8.3) per point
    # build_graph branches
    i_f, c_f, d_f, ind_f = s3g_util.build_graph(xyz, 0.15, K, S, sample_method='FPS')
    i_i, c_i, d_i, ind_i = s3g_util.build_graph(xyz, 0.15, K, S, sample_method='IDS')
    i_r, c_r, d_r, ind_r = s3g_util.build_graph(xyz, 0.15, K, S, sample_method='random')
    assert torch.equal(i_f, i_i) and torch.equal(i_f, i_r)
    for ind in (ind_f, ind_i, ind_r):
        assert ind.shape == (B, S, 2) and ind.dtype == torch.int32
        assert torch.equal(ind[:, :, 0], torch.arange(B, device=dev, dtype=torch.int32).view(B, 1).expand(B, S))
        assert int(ind[:, :, 1].min()) >= 0 and int(ind[:, :, 1].max()) < N
    for b in range(B):
        assert len(set(ind_i[b, :, 1].tolist())) == S
    io, co, do = oracle.build_sphere_neighbor(xyz.cpu().numpy(), xyz.cpu().numpy(), 0.15, None, K)
    prob_o = do.sum(-1) / co                                       # utils/sph3gcn_util.py:38
    torch.testing.assert_close((d_i.sum(-1) / c_i.float()).cpu(), torch.from_numpy(prob_o.astype(np.float32)), rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        s3g_util.build_graph(xyz, 0.15, K, S, sample_method='nope')
    none = s3g_util.build_graph(xyz, 0.15, K, None)
    assert none[3] is None
