"""csrc/condlogits.hip, tf_gemm.linear_concat2_onehot, s3g_util.pointwise_conv3d_onehot and the one-hot ShapeNet model on the device
against the float64 statement of tests/_cond_ref.py.  Bounds (derived there, not measured): |got - ref| <= (terms + 3) 2^-24 mag
per element — forward: terms = K1 + K2 + 2; dT, dbias: the rows summed; elements without a term exactly 0 — for the fused form AND
for the literal concatenation of the same commit; the dW halves and dA1 / dA2 come from existing kernels and are held by
tests/_errors.assert_per_element at its 1e-5.  Measured on an MI355X (largest used fraction of the bound over the cases below):
    forward: fused 0.17, literal 0.27;  dT: fused 0.17, literal 0.27;  dbias: fused 0.19, literal 0.15;
    the small model's logits: fused 0.07, literal 0.08;  dW halves / dA (of mag): 4.1e-7 / 5.2e-7 in both forms
Every launch here is an ordinary one."""
import os

import numpy as np
import pytest

import _cond_ref as cr
from _errors import assert_per_element

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_INFO = os.path.join(ROOT, "tests", "golden", "shapenet_class_info.txt")

# (B, P, K1, K2, N, T, bias): (5, 1) every row another cloud; (3, 37) tiles and 4-row groups straddling clouds, a ragged last
# tile; (4, 600) several workgroups and several slices per cloud; (2, 16) the aligned case.  Every N of {1, 16, 17, 50, 64} (one to
# four column tiles, full and ragged), every (K1, K2) of {(16, 0), (16, 16), (64, 64)}, T of {1, 16}, with and without bias.
CASES = [
    (5, 1, 64, 64, 50, 16, True),
    (5, 1, 16, 16, 1, 1, False),
    (3, 37, 16, 16, 17, 16, False),
    (3, 37, 16, 0, 1, 16, True),
    (3, 37, 64, 64, 64, 16, True),
    (4, 600, 64, 64, 50, 16, True),
    (4, 600, 16, 16, 64, 1, False),
    (4, 600, 16, 0, 16, 16, True),
    (2, 16, 16, 0, 16, 1, True),
    (2, 16, 64, 64, 50, 16, False),
]


def _called(events):
    return [name for name, _args, _e0, _e1 in events]


def _layer(dev, fused, ops, cat, B, P, T, N, w, bias, dy, monkeypatch):
    """s3g_util.pointwise_conv3d_onehot in one form with the given weights -> (y, [dW, dbias | None, dA1, dA2 | None], C calls)"""
    import torch
    from sph3d_gcn_amd import _lib
    from sph3d_gcn_amd import sph3gcn_util as s3g_util
    a1, a2 = ops
    monkeypatch.setattr(s3g_util, "FUSE_LOGITS_ONEHOT", fused)
    store = s3g_util.VariableStore(device=dev, seed=1)
    ta = torch.from_numpy(a1).to(dev).reshape(B, P, -1).requires_grad_(True)
    tb = torch.zeros((B, P, 0), device=dev) if a2 is None else torch.from_numpy(a2).to(dev).reshape(B, P, -1).requires_grad_(True)
    tcat = torch.from_numpy(cat).to(dev)
    with s3g_util.variable_store(store):
        call = lambda: s3g_util.pointwise_conv3d_onehot(ta, tb, tcat, T, N, 'logits', activation_fn=None, with_bn=False,
                                                        with_bias=bias is not None)
        call()                                                      # creates the variables
        params = dict(store.named_parameters())
        with torch.no_grad():
            params["params.logits/weights"].copy_(torch.from_numpy(w))
            if bias is not None:
                params["params.logits/biases"].copy_(torch.from_numpy(bias))
        _lib.timing_start()
        y = call()
        wrt = [params["params.logits/weights"]] + ([params["params.logits/biases"]] if bias is not None else []) + [ta] \
            + ([tb] if a2 is not None else [])
        grads = list(torch.autograd.grad(y, wrt, torch.from_numpy(dy).to(dev).reshape(B, P, N)))
        calls = _called(_lib.timing_stop())
    torch.cuda.synchronize()
    gw = grads.pop(0)
    gb = grads.pop(0) if bias is not None else None
    ga1 = grads.pop(0)
    ga2 = grads.pop(0) if a2 is not None else None
    return y.detach(), (gw, gb, ga1, ga2), calls


@pytest.mark.parametrize("B,P,K1,K2,N,T,with_bias", CASES)
def test_fused_and_literal_forms_against_the_float64_statement(dev, monkeypatch, B, P, K1, K2, N, T, with_bias):
    import torch
    a1, a2, w, bias, dy = cr.make_operands(11, B, P, K1, K2, N, T, with_bias)
    cat = cr.make_categories(B, T)
    ref = cr.cond_reference(a1, a2, w, bias, cat, P, dy)
    K, R = K1 + K2, B * P
    kept = {}
    for fused in (True, False):
        what = "%s (B=%d P=%d K=%d+%d N=%d T=%d)" % ("fused" if fused else "literal", B, P, K1, K2, N, T)
        y, (gw, gb, ga1, ga2), calls = _layer(dev, fused, (a1, a2), cat, B, P, T, N, w, bias, dy, monkeypatch)
        # the fused form runs the new kernels and no concatenated product; the literal form none of the new kernels
        assert ("sph3d_pointwise_gemm_cond" in calls) == fused and ("sph3d_pointwise_gemm_cond_grad" in calls) == fused, calls
        assert y.shape == (B, P, N) and gw.shape == (K + T, N)
        cr.assert_bound(y.cpu().numpy().reshape(R, N), ref.y, ref.y_mag, K + 2, what + " forward")
        gw = gw.cpu().numpy()
        cr.assert_bound(gw[K:], ref.dt, ref.dt_mag, ref.dt_terms[:, None], what + " dT")
        absent = [c for c in range(T) if c not in cat.tolist()]
        assert not gw[K:][absent].any()                              # exactly 0.0f
        if with_bias:
            cr.assert_bound(gb.cpu().numpy(), ref.db, ref.db_mag, R, what + " dbias")
        assert_per_element(gw[:K], ref.dw, ref.dw_mag, what + " dW halves")
        ga = ga1 if ga2 is None else torch.cat((ga1, ga2), 2)
        assert_per_element(ga.cpu().numpy().reshape(R, K), ref.da, ref.da_mag, what + " dA")
        kept[fused] = (y, gw)
    # determinism: a second run of the fused forward and of the category gradient is bit-equal
    y2, (gw2, _gb, _a, _b), _ = _layer(dev, True, (a1, a2), cat, B, P, T, N, w, bias, dy, monkeypatch)
    assert torch.equal(y2.view(torch.int32), kept[True][0].view(torch.int32))
    assert np.array_equal(cr_bits(gw2.cpu().numpy()), cr_bits(kept[True][1]))


def cr_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_entry_points_directly_and_their_determinism(dev):
    """tf_gemm.linear_concat2_onehot without the layer around it; sph3d_pointwise_gemm_cond_grad with and without dbias: the same
    dT bit for bit, twice; rows of absent categories are overwritten with 0 (the output buffer starts as NaN)"""
    import torch
    from sph3d_gcn_amd import _lib, tf_gemm
    B, P, K1, K2, N, T = 4, 600, 64, 64, 50, 16
    a1, a2, w, bias, dy = cr.make_operands(5, B, P, K1, K2, N, T)
    cat = cr.make_categories(B, T)
    ref = cr.cond_reference(a1, a2, w, bias, cat, P, dy)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    y = tf_gemm.linear_concat2_onehot(t(a1), t(a2), t(cat), t(w), t(bias), P)
    cr.assert_bound(y.cpu().numpy(), ref.y, ref.y_mag, K1 + K2 + 2, "linear_concat2_onehot")
    y_again = tf_gemm.linear_concat2_onehot(t(a1), t(a2), t(cat).long(), t(w), t(bias), P)         # any integer dtype of cat
    assert torch.equal(y.view(torch.int32), y_again.view(torch.int32))
    l = _lib.lib()
    wsb = l.sph3d_pointwise_gemm_cond_grad_workspace(B, P, N, T)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    tdy, tcat = t(dy), t(cat)
    outs = []
    for with_db in (True, False, True):
        dt = torch.full((T, N), float("nan"), device=dev)
        db = torch.full((N,), float("nan"), device=dev)
        _lib.check(l.sph3d_pointwise_gemm_cond_grad(B, P, N, T, _lib.ptr(tdy), _lib.ptr(tcat), _lib.ptr(dt),
                                                    _lib.ptr(db) if with_db else None, _lib.ptr(ws), wsb, _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs.append((dt.cpu().numpy(), db.cpu().numpy()))
        assert np.isnan(outs[-1][1]).all() != with_db
    cr.assert_bound(outs[0][0], ref.dt, ref.dt_mag, ref.dt_terms[:, None], "cond_grad dT")
    cr.assert_bound(outs[0][1], ref.db, ref.db_mag, B * P, "cond_grad dbias")
    assert np.array_equal(cr_bits(outs[0][0]), cr_bits(outs[1][0])) and np.array_equal(cr_bits(outs[0][0]), cr_bits(outs[2][0]))
    assert np.array_equal(cr_bits(outs[0][1]), cr_bits(outs[2][1]))
    # more clouds than the finishing workgroup takes at a time (1024 / N = 16 at N = 64)
    B, P, N = 37, 3, 64
    _a1, _a2, _w, _bias, dy = cr.make_operands(6, B, P, 16, 0, N, T)
    cat = cr.make_categories(B, T)
    ref = cr.cond_reference(_a1, None, _w, None, cat, P, dy)
    dt, db = torch.full((T, N), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
    wsb = l.sph3d_pointwise_gemm_cond_grad_workspace(B, P, N, T)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    tdy, tcat = t(dy), t(cat)
    _lib.check(l.sph3d_pointwise_gemm_cond_grad(B, P, N, T, _lib.ptr(tdy), _lib.ptr(tcat), _lib.ptr(dt), _lib.ptr(db), _lib.ptr(ws), wsb,
                                                _lib.stream_ptr()))
    torch.cuda.synchronize()
    cr.assert_bound(dt.cpu().numpy(), ref.dt, ref.dt_mag, ref.dt_terms[:, None], "cond_grad dT, 37 clouds")
    cr.assert_bound(db.cpu().numpy(), ref.db, ref.db_mag, B * P, "cond_grad dbias, 37 clouds")


@pytest.mark.parametrize("K1,N", [(24, 50), (16, 65)])
def test_an_unsupported_shape_falls_back_or_raises_and_launches_nothing(dev, monkeypatch, K1, N):
    """s3g_util.pointwise_conv3d_onehot takes the literal concatenation (none of the new entry points is called);
    tf_gemm.linear_concat2_onehot raises (SPH3D_EUNSUPPORTED is answered on the host, before any launch)"""
    import torch
    from sph3d_gcn_amd import _lib, tf_gemm
    B, P, K2, T = 3, 37, 16, 16
    assert not tf_gemm.cond_supported(B, P, K1, K2, N, T)
    a1, a2, w, bias, dy = cr.make_operands(2, B, P, K1, K2, N, T)
    cat = cr.make_categories(B, T)
    ref = cr.cond_reference(a1, a2, w, bias, cat, P, dy)
    y, (gw, gb, ga1, ga2), calls = _layer(dev, True, (a1, a2), cat, B, P, T, N, w, bias, dy, monkeypatch)
    assert not [c for c in calls if "_cond" in c], calls
    assert_per_element(y.cpu().numpy().reshape(B * P, N), ref.y, ref.y_mag, "fallback forward")
    assert_per_element(gw.cpu().numpy()[K1 + K2:], ref.dt, ref.dt_mag, "fallback dT")
    t = lambda x: torch.from_numpy(x).to(dev)
    with pytest.raises(_lib.Sph3dError, match="pointwise_gemm_cond"):
        tf_gemm.linear_concat2_onehot(t(a1), t(a2), t(cat), t(w), t(bias), P)
    torch.cuda.synchronize()


def _model_run(dev, fused, pts, cat, label, monkeypatch):
    import torch
    from sph3d_gcn_amd import sph3gcn_util as s3g_util
    from sph3d_gcn_amd.harness import shapenet_net
    monkeypatch.setattr(s3g_util, "FUSE_LOGITS_ONEHOT", fused)
    model = shapenet_net.SPH3DShapeNetOneHot(50, 16, shapenet_net.small_config(512), device=dev, seed=3)
    pred, end = model(pts, cat, is_training=True)
    assert 'feats' not in dict.keys(end)
    loss = model.loss(pred, label)
    loss.backward()
    torch.cuda.synchronize()
    return model, pred.detach(), end['feats'].detach(), loss.detach()


def test_model_fused_against_literal(dev, monkeypatch):
    """SPH3DShapeNetOneHot(50, 16, small_config(512)), B = 3 with categories {2, 2, 11}: the two forms share everything up to the
    classifier, so the logits of each are held to the forward bound with `mag` from its own end_points['feats'] and the weights"""
    import torch
    from sph3d_gcn_amd.harness import synth
    pts = torch.from_numpy(synth.modelnet_batch(20, 3, 512)).to(dev)
    cat = torch.tensor([2, 2, 11], dtype=torch.int32, device=dev)
    label = torch.randint(0, 50, (3, 512), generator=torch.Generator().manual_seed(1)).to(dev)
    runs = {f: _model_run(dev, f, pts, cat, label, monkeypatch) for f in (True, False)}
    for fused, (model, pred, feats, loss) in runs.items():
        params = dict(model.named_parameters())
        w = params["store.params.logits/weights"]
        assert tuple(w.shape) == (48, 50) and pred.shape == (3, 512, 50) and feats.shape == (3, 512, 48)
        f64, w64 = feats.cpu().numpy().astype(np.float64).reshape(-1, 48), w.detach().cpu().numpy().astype(np.float64)
        cr.assert_bound(pred.cpu().numpy().reshape(-1, 50), f64 @ w64, np.abs(f64) @ np.abs(w64), 32 + 2,
                        "model logits (%s)" % ("fused" if fused else "literal"))
        g = w.grad[32:]
        assert g[[2, 11]].abs().sum() > 0 and not g[[c for c in range(16) if c not in (2, 11)]].any()
        for n, p in params.items():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    (mf, pf, ff, lf), (ml, pl, fl, ll) = runs[True], runs[False]
    print("features bit-equal between the forms: %s" % torch.equal(ff[:, :, :32], fl[:, :, :32]))
    torch.testing.assert_close(ff, fl, rtol=1e-5, atol=1e-5)
    assert torch.equal(ff[:, :, 32:], fl[:, :, 32:])
    torch.testing.assert_close(lf, ll, rtol=1e-5, atol=0)
    for (n, p), (n2, q) in zip(mf.named_parameters(), ml.named_parameters()):
        assert n == n2 and p.shape == q.shape
        scale = float(q.grad.abs().max())
        worst = float((p.grad - q.grad).abs().max())
        assert worst <= 2e-3 * scale, "%s: gradients differ by %.3e of the largest magnitude" % (n, worst / max(scale, 1e-30))


def test_protocol_two_training_steps_and_one_evaluation(dev):
    """ObjectFeed -> SPH3DShapeNetOneHot training steps (category from the feed) -> shapeeval.evaluate with the fixture's part
    table; the evaluation equals evaluate_reference fed the recorded logits"""
    import torch
    from sph3d_gcn_amd.harness import objfeed, shapeeval, shapenet_net
    names, part_lo, part_n = objfeed.read_class_info(CLASS_INFO)
    blocks = cr.proto_shapes(part_lo, part_n)
    pool = objfeed.ShapePool(blocks, cr.PROTO_CATEGORY, part_lo, part_n, device=dev)
    N = cr.PROTO_N
    model = shapenet_net.SPH3DShapeNetOneHot(50, len(names), shapenet_net.small_config(N), device=dev, seed=3)
    feed = objfeed.ObjectFeed(pool, cr.PROTO_BATCH, N, seed=cr.PROTO_SEED, dataset="shapenet")
    steps = 0
    for points, label, category, ready in feed:
        torch.cuda.current_stream().wait_event(ready)               # (label and category are read on the main stream)
        pred, _ = model(points, category, is_training=True, points_ready=ready)
        loss = model.loss(pred, label)
        feed.done(ready)
        loss.backward()
        assert pred.shape == (cr.PROTO_BATCH, N, 50) and torch.isfinite(loss)
        with torch.no_grad():
            for n, p in model.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
                p.add_(p.grad, alpha=-1e-3)
                p.grad = None
        steps += 1
    assert steps == 2

    index, logits = {}, {}

    def rec(batch_index, q, idx, lg):
        assert q == len(index.setdefault(batch_index, []))
        index[batch_index].append(idx.cpu().numpy())
        logits.setdefault(batch_index, []).append(lg.cpu().numpy())

    res = shapeeval.evaluate(lambda p, l, c: model(p, c, is_training=False)[0], pool, cr.PROTO_BATCH, N, cr.PROTO_SEED, 50,
                             min_count=cr.PROTO_MIN_COUNT, max_passes=cr.PROTO_MAX_PASSES, on_pass=rec)
    assert res.complete and res.batches == [0, 1] and res.nonfinite_rows == 0 and res.num_categories == 16

    def fn(i, q, idx):
        assert np.array_equal(idx, index[i][q])
        return logits[i][q]
    rows_label = np.concatenate([b[:, 6] for b in blocks])
    want = shapeeval.evaluate_reference(fn, cr.PROTO_SIZES, rows_label, np.asarray(cr.PROTO_CATEGORY, np.int32), cr.PROTO_BATCH, N,
                                        cr.PROTO_SEED, 50, part_lo, part_n, cr.PROTO_MIN_COUNT, cr.PROTO_MAX_PASSES)
    for name in ("shapes", "category", "shape_iou", "correct", "seen", "class_correct", "class_seen"):
        assert np.array_equal(getattr(res, name), getattr(want, name)), name
    assert np.array_equal(res.category_miou, want.category_miou, equal_nan=True)
    for name in ("mean_category_miou", "instance_miou", "accuracy", "nonfinite_rows", "num_categories", "batches", "passes", "complete"):
        assert getattr(res, name) == getattr(want, name), name
    assert res.seen.tolist() == cr.PROTO_SIZES
