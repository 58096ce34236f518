"""The category-conditioned logits layer without a GPU: the float64 statement (tests/_cond_ref.py) against the autograd gradient of
the literal-concatenation path, the host-side validation of the new entry points (no launch), the one-hot ShapeNet model on the
oracle-backed stand-ins, and the category table."""
import os

import numpy as np
import pytest
import torch

import _cond_ref as cr
from oracle import torch_ops
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import objfeed, shapenet_net, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_INFO = os.path.join(ROOT, "tests", "golden", "shapenet_class_info.txt")


def test_statement_by_hand():
    """two clouds of two rows, K1 = 1, no second half, T = 2: every figure written out"""
    a1 = np.array([[1.0], [2.0], [3.0], [-4.0]], np.float32)
    w = np.array([[10.0, -1.0], [100.0, 200.0], [300.0, 400.0]], np.float32)            # one operand row, two category rows
    bias = np.array([0.5, -0.5], np.float32)
    dy = np.array([[1, 2], [3, 4], [5, 6], [-7, 8]], np.float32)
    r = cr.cond_reference(a1, None, w, bias, [1, 2], 2, dy)                              # cloud 1's category 2 == T: no row
    assert r.y.tolist() == [[310.5, 398.5], [320.5, 397.5], [30.5, -3.5], [-39.5, 3.5]]
    assert r.y_mag.tolist() == [[310.5, 401.5], [320.5, 402.5], [30.5, 3.5], [40.5, 4.5]]
    assert r.dt.tolist() == [[0, 0], [4, 6]] and r.dt_mag.tolist() == [[0, 0], [4, 6]] and r.dt_terms.tolist() == [0, 2]
    assert r.db.tolist() == [2, 20] and r.db_mag.tolist() == [16, 20]
    assert r.dw.tolist() == [[1 + 6 + 15 + 28, 2 + 8 + 18 - 32]]


@pytest.mark.parametrize("B,P,K1,K2,N,T", [(5, 3, 16, 16, 50, 16), (7, 1, 16, 0, 17, 16), (3, 37, 32, 16, 5, 1)])
def test_literal_path_gradient_is_the_analytic_statement(B, P, K1, K2, N, T):
    """the CPU fallback of s3g_util.pointwise_conv3d_onehot (concatenation with the one-hot tile + pointwise_conv3d): its output
    and its autograd gradients against the statement — dT the per-category sums, absent categories exactly zero rows, categories
    -1 and T without contribution"""
    a1, a2, w, bias, dy = cr.make_operands(3, B, P, K1, K2, N, T)
    if a2 is None:
        a2 = np.zeros((B * P, 0), np.float32)
    cat = cr.make_categories(B, T)
    assert -1 in cat and (T in cat or B < 4) and len(set(cat.tolist())) < B
    ref = cr.cond_reference(a1, a2, w, bias, cat, P, dy)
    store = s3g_util.VariableStore(seed=1)
    ta, tb = (torch.from_numpy(x).reshape(B, P, -1).requires_grad_(True) for x in (a1, a2))
    with torch_ops.patched_util(), s3g_util.variable_store(store):
        call = lambda: s3g_util.pointwise_conv3d_onehot(ta, tb, torch.from_numpy(cat), T, N, 'logits', activation_fn=None,
                                                        with_bn=False, with_bias=True)
        call()                                                                           # creates the variables
        params = dict(store.named_parameters())
        assert sorted(params) == ["params.logits/biases", "params.logits/weights"]
        assert tuple(params["params.logits/weights"].shape) == (K1 + K2 + T, N)
        with torch.no_grad():
            params["params.logits/weights"].copy_(torch.from_numpy(w))
            params["params.logits/biases"].copy_(torch.from_numpy(bias))
        y = call()
    assert y.shape == (B, P, N)
    cr.assert_bound(y.detach().numpy().reshape(B * P, N), ref.y, ref.y_mag, K1 + K2 + 2, "literal forward")
    gw, gb, ga, gb2 = torch.autograd.grad(y, [params["params.logits/weights"], params["params.logits/biases"], ta, tb],
                                          torch.from_numpy(dy).reshape(B, P, N))
    K = K1 + K2
    gt = gw[K:].numpy()
    cr.assert_bound(gt, ref.dt, ref.dt_mag, ref.dt_terms[:, None], "literal dT")
    absent = [c for c in range(T) if c not in cat.tolist()]
    assert not gt[absent].any() and (ref.dt_terms[absent] == 0).all()
    live = cat[(cat >= 0) & (cat < T)]
    assert int(ref.dt_terms.sum()) == P * len(live)                                      # -1 and T: counted nowhere
    cr.assert_bound(gb.numpy(), ref.db, ref.db_mag, B * P, "literal dbias")
    cr.assert_bound(gw[:K].numpy(), ref.dw, ref.dw_mag, B * P, "literal dW halves")
    cr.assert_bound(torch.cat((ga, gb2), 2).numpy().reshape(B * P, K), ref.da, ref.da_mag, N, "literal dA")


def test_one_hot_tile_is_tf_one_hot():
    hot = s3g_util.one_hot_tile(torch.tensor([2, -1, 3, 0]), 3, 5)
    assert hot.shape == (4, 5, 3) and hot.dtype == torch.float32
    assert hot[:, 0].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0], [1, 0, 0]] and torch.equal(hot[:, 0], hot[:, 4])


# ---- the entry points on the host ---------------------------------------------------------------------------------------------
PTR = 4096          # a non-NULL, 16-byte aligned address for calls that must answer before they touch anything


def _fwd(l, B, P, K1, K2, N, T, a1=PTR, a2=PTR, w=PTR, bias=None, cat=PTR, y=PTR):
    return l.sph3d_pointwise_gemm_cond(B, P, K1, K2, N, T, a1, a2, w, bias, cat, y, None)


def _grad(l, B, P, N, T, dy=PTR, cat=PTR, dt=PTR, dbias=None, ws=PTR, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = l.sph3d_pointwise_gemm_cond_grad_workspace(B, P, N, T)
    return l.sph3d_pointwise_gemm_cond_grad(B, P, N, T, dy, cat, dt, dbias, ws, ws_bytes, None)


def test_entry_points_validate_on_the_host():
    l = _lib.lib()
    assert l.sph3d_abi_version() == 2
    EINVAL, EUNSUPPORTED = -1, -4
    ok = (32, 2048, 64, 64, 50, 16)
    assert l.sph3d_pointwise_gemm_cond_supported(*ok) == 1
    # dimensions that are not positive, B * P past an int
    for bad in [(-1, 8, 16, 16, 8, 4), (2, 0, 16, 16, 8, 4), (2, 8, -16, 16, 8, 4), (2, 8, 16, -16, 8, 4), (2, 8, 16, 16, 0, 4),
                (2, 8, 16, 16, 8, 0), (2, 8, 16, 16, 8, -3), (65536, 65536, 16, 16, 8, 4), (1 << 30, 2, 16, 16, 8, 4)]:
        assert l.sph3d_pointwise_gemm_cond_supported(*bad) == 0, bad
        assert _fwd(l, *bad) == EINVAL, bad
    assert b"fit an int" in l.sph3d_last_error()
    # shapes outside the kernels' domain
    for bad in [(2, 8, 24, 16, 8, 4), (2, 8, 16, 8, 8, 4), (2, 8, 16, 16, 65, 4), (2, 8, 80, 64, 8, 4), (2, 8, 8, 0, 8, 4),
                (2, 8, 16, 16, 8, 4097)]:
        assert l.sph3d_pointwise_gemm_cond_supported(*bad) == 0, bad
        assert _fwd(l, *bad) == EUNSUPPORTED, bad
    assert b"multiples of 16" in l.sph3d_last_error()
    with pytest.raises(_lib.Sph3dError):
        _lib.check(EUNSUPPORTED)
    # NULL operands (a shape the call accepts gets as far as this check: rc -1 with this message)
    for null in ("a1", "a2", "w", "cat", "y"):
        assert _fwd(l, *ok, **{null: None}) == EINVAL and b"must not be NULL" in l.sph3d_last_error(), null
    assert _fwd(l, 2, 8, 16, 16, 8, 4, a1=PTR + 4) == EINVAL and b"aligned" in l.sph3d_last_error()
    # _supported agrees with what the call accepts: an accepted shape reaches the NULL check, any other is refused before it
    for B, P in [(1, 1), (3, 37), (32, 2048)]:
        for K1 in (0, 8, 16, 24, 64, 128, 144):
            for K2 in (0, 16, 40, 64):
                for N in (1, 50, 64, 65):
                    for T in (1, 16, 4096):
                        rc = _fwd(l, B, P, K1, K2, N, T, a1=None)
                        accepted = rc == EINVAL and b"must not be NULL" in l.sph3d_last_error()
                        assert accepted == bool(l.sph3d_pointwise_gemm_cond_supported(B, P, K1, K2, N, T)), (B, P, K1, K2, N, T, rc)
                        assert rc in (EINVAL, EUNSUPPORTED)
    assert l.sph3d_pointwise_gemm_cond_supported(2, 8, 64, 0, 50, 16) == 1 and _fwd(l, 2, 8, 64, 0, 50, 16, a2=None, y=None) == EINVAL

    # the gradient of the category rows
    for bad in [(0, 8, 8, 4), (2, -8, 8, 4), (2, 8, 0, 4), (2, 8, 8, 0), (65536, 65536, 8, 4)]:
        assert l.sph3d_pointwise_gemm_cond_grad_workspace(*bad) == 0
        assert _grad(l, *bad) == EINVAL, bad
    for bad in [(2, 8, 65, 4), (2, 8, 8, 4097), (65536, 2, 8, 4)]:
        assert _grad(l, *bad) == EUNSUPPORTED, bad
    for null in ("dy", "cat", "dt"):
        assert _grad(l, 32, 2048, 50, 16, **{null: None}) == EINVAL and b"must not be NULL" in l.sph3d_last_error(), null
    need = l.sph3d_pointwise_gemm_cond_grad_workspace(32, 2048, 50, 16)
    assert need >= 32 * 50 * 4 and need % 4 == 0
    assert l.sph3d_pointwise_gemm_cond_grad_workspace(5, 1, 50, 16) == 5 * 50 * 4        # one slice per cloud
    assert _grad(l, 32, 2048, 50, 16, ws_bytes=need - 1) == EINVAL and b"workspace" in l.sph3d_last_error()
    assert _grad(l, 32, 2048, 50, 16, ws=None) == EINVAL and b"workspace" in l.sph3d_last_error()
    with pytest.raises(ValueError):
        _lib.check(EINVAL)


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from sph3d_gcn_amd import tf_gemm
    a = torch.zeros(6, 16)
    with pytest.raises(_lib.Sph3dError):
        tf_gemm.linear_concat2_onehot(a, None, torch.zeros(2, dtype=torch.int32), torch.zeros(16 + 4, 8), None, 3)
    assert tf_gemm.cond_supported(32, 2048, 64, 64, 50, 16) and not tf_gemm.cond_supported(32, 2048, 24, 64, 50, 16)
    assert s3g_util.FUSE_LOGITS_ONEHOT in (True, False)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _variables(model):
    return [(n, tuple(p.shape)) for n, p in model.named_parameters()]


def test_onehot_model_on_oracle_ops():
    cfg = shapenet_net.small_config(512)
    pts = torch.from_numpy(synth.modelnet_batch(20, 2, 512))
    label = torch.randint(0, 50, (2, 512), generator=torch.Generator().manual_seed(1))
    cat = torch.tensor([11, 2], dtype=torch.int32)
    with torch_ops.patched_util():
        model = shapenet_net.SPH3DShapeNetOneHot(50, 16, cfg, device=torch.device("cpu"))
        pred, end = model(pts, cat, is_training=True)
        assert 'feats' not in dict.keys(end)                       # built on first access
        loss = model.loss(pred, label)
        loss.backward()
        plain = shapenet_net.SPH3DShapeNet(3, cfg, device=torch.device("cpu"))
        _, end_plain = plain(pts, is_training=True)
    assert pred.shape == (2, 512, 50) and torch.isfinite(pred).all() and torch.isfinite(loss)
    params = dict(model.named_parameters())
    assert tuple(params["store.params.logits/weights"].shape) == (cfg.mlp + cfg.mlp + 16, 50) == (48, 50)
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    # end_points['feats'] is the literal concatenation: the per-category model's 2 mlp features (same seed, same variables
    # up to the classifier) followed by the one-hot tile; and the logits are its product with the weights
    feats = end['feats']
    assert feats.shape == (2, 512, 48) and 'feats' in dict.keys(end)
    assert torch.equal(feats[:, :, :32], end_plain['feats'])
    want_hot = torch.zeros(2, 512, 16)
    want_hot[0, :, 11] = 1
    want_hot[1, :, 2] = 1
    assert torch.equal(feats[:, :, 32:], want_hot)
    torch.testing.assert_close(pred, feats @ params["store.params.logits/weights"], rtol=1e-5, atol=1e-5)
    # only the two categories' rows of the classifier get a gradient
    g = params["store.params.logits/weights"].grad[32:]
    assert g[[2, 11]].abs().sum() > 0 and not g[[c for c in range(16) if c not in (2, 11)]].any()
    # the full plan's classifier is [64 + 64 + 16, 50]
    full = shapenet_net.shapenet_config()
    assert (full.mlp + full.mlp + shapenet_net.NUM_CATEGORIES, 50) == (144, 50)


def test_per_category_model_creates_the_variables_it_created_before():
    """factoring the shared body out of get_model changes neither the variables, nor their order, nor (same seed) their values"""
    cfg = shapenet_net.small_config(512)
    pts = torch.from_numpy(synth.modelnet_batch(20, 2, 512))
    with torch_ops.patched_util():
        plain = shapenet_net.SPH3DShapeNet(3, cfg, device=torch.device("cpu"))
        plain(pts, is_training=True)
        onehot = shapenet_net.SPH3DShapeNetOneHot(50, 16, cfg, device=torch.device("cpu"))
        onehot(pts, torch.tensor([0, 1]), is_training=True)
    got = _variables(plain)
    want = [("store.params.mlp1/weights", (3, 16)), ("store.params.mlp1/bn/gamma", (16,)), ("store.params.mlp1/bn/beta", (16,))]
    cin = 16
    layers = [("conv1_1", 32, 2), ("conv1_2", 32, 2), ("conv2_1", 64, 2), ("conv2_2", 64, 1),
              ("deconv1_1", 64, 2), ("deconv1_2", 64, 1), ("deconv2_1", 32, 2), ("deconv2_2", 32, 2)]
    for name, cout, r in layers:
        if name == "deconv2_1":
            cin += 64                                               # the skip connection of level 2
        want += [("store.params.%s/depthwise_weights" % name, (33, cin, r)), ("store.params.%s/weights" % name, (cin * r, cout)),
                 ("store.params.%s/bn/gamma" % name, (cout,)), ("store.params.%s/bn/beta" % name, (cout,))]
        cin = cout
    want += [("store.params.mlp2/weights", (32 + 32, 16)), ("store.params.mlp2/bn/gamma", (16,)), ("store.params.mlp2/bn/beta", (16,)),
             ("store.params.logits/weights", (32, 3))]
    assert got == want
    # the one-hot model: the same variables in the same order, the same values up to the classifier
    other = _variables(onehot)
    assert other[:-1] == want[:-1] and other[-1] == ("store.params.logits/weights", (48, 50))
    for (n, p), (_, q) in list(zip(plain.named_parameters(), onehot.named_parameters()))[:-1]:
        assert torch.equal(p, q), n


def test_read_class_info_on_the_fixture():
    names, part_lo, part_n = objfeed.read_class_info(CLASS_INFO)
    assert len(names) == 16 and names[0] == "Airplane" and names[10] == "Motorbike" and names[-1] == "Table"
    assert part_lo.dtype == np.int32 and part_n.dtype == np.int32
    rows = [line.rstrip("\n").split("\t") for line in open(CLASS_INFO)]
    assert part_n.tolist() == [int(r[2]) for r in rows] and part_lo.tolist() == [int(r[3]) for r in rows]
    assert int(part_n.sum()) == 50 and part_lo.tolist() == np.concatenate(([0], np.cumsum(part_n)[:-1])).tolist()
    assert int(part_n[10]) == 6 and int(part_lo[10]) == 30
    # a ShapePool takes the table as it is
    pool = objfeed.ShapePool([objfeed.shape_blocks(np.zeros((4, 3), np.float32), 31)], [10], part_lo, part_n, device=torch.device("cpu"))
    lo, n = pool.part_range([0], 50)
    assert lo.tolist() == [30] and n.tolist() == [6]


def test_the_protocol_case_completes_within_its_cap():
    """the evaluation tests/test_gpu_condlogits.py runs on the device: its draws cover every row within PROTO_MAX_PASSES whatever
    the logits are (the draws do not depend on them), so the GPU test's `complete` cannot hide behind the cap"""
    from sph3d_gcn_amd.harness import shapeeval
    _names, part_lo, part_n = objfeed.read_class_info(CLASS_INFO)
    blocks = cr.proto_shapes(part_lo, part_n)
    assert [len(b) for b in blocks] == cr.PROTO_SIZES
    label = np.concatenate([b[:, 6] for b in blocks])
    for k, c in enumerate(cr.PROTO_CATEGORY):
        assert ((blocks[k][:, 6] >= part_lo[c]) & (blocks[k][:, 6] < part_lo[c] + part_n[c])).all()
    zeros = lambda i, q, index: np.zeros(index.shape + (50,), np.float32)
    res = shapeeval.evaluate_reference(zeros, cr.PROTO_SIZES, label, np.asarray(cr.PROTO_CATEGORY, np.int32), cr.PROTO_BATCH,
                                       cr.PROTO_N, cr.PROTO_SEED, 50, part_lo, part_n, cr.PROTO_MIN_COUNT, cr.PROTO_MAX_PASSES)
    assert res.complete and res.batches == [0, 1] and max(res.passes) < cr.PROTO_MAX_PASSES
    print("draws per batch: %s" % (res.passes,))


def test_read_class_info_refuses_other_tables(tmp_path):
    p = tmp_path / "t.txt"
    p.write_text("A\t1\t2\n")
    with pytest.raises(ValueError):
        objfeed.read_class_info(str(p))
    p.write_text("A\tx\t2\t0\nB\ty\t3\t3\n")                        # the second range does not follow the first
    with pytest.raises(ValueError):
        objfeed.read_class_info(str(p))
