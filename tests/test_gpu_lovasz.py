"""The Lovasz-softmax loss on the device (csrc/lovasz.hip) against the float64 statement (harness/lovasz.py), stage by stage and end
to end; tests/_lovasz_ref.py holds the inputs and derives the bounds.  The stages after probs are staged on the device's own probs:
the sorted order is an integer function of them and must be EXACT.
Measured on an MI355X, worst over the 28 shapes, as fractions of the bounds: probs 0.330, coef 0.608, class_loss 0.116, loss 0.088,
dlogits 0.373, end to end 0.017."""
import numpy as np
import pytest
import torch

import _lovasz_ref as R
from sph3d_gcn_amd import _lib, tf_loss
from sph3d_gcn_amd.harness import lovasz

pytestmark = pytest.mark.gpu

_ref = {}


def _case(N, C):
    if (N, C) not in _ref:
        x, label, inner = R.lovasz_inputs(4, N, C)
        _ref[(N, C)] = (x, label, inner, lovasz.lovasz_reference(x, label, inner))
    return _ref[(N, C)]


def _call(dev, x, label, inner, grad=True, order=True, ignore=R.IGNORE):
    """one C-ABI call on NaN-filled (order: -7-filled) outputs -> dict of numpy arrays"""
    l = _lib.lib()
    B, N, C = x.shape
    xs, ls = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, label))
    ms = torch.from_numpy(np.ascontiguousarray(inner)).to(dev) if inner is not None else None
    nan = float("nan")
    out = dict(probs=torch.full((B, N, C), nan, device=dev), coef=torch.full((B, N, C), nan, device=dev),
               class_loss=torch.full((B, C), nan, device=dev), loss=torch.full((B,), nan, device=dev),
               dlogits=torch.full((B, N, C), nan, device=dev) if grad else None,
               order=torch.full((B, C, N), -7, dtype=torch.int32, device=dev) if order else None)
    _lib.check(l.sph3d_lovasz_softmax(B, N, C, _lib.ptr(xs), _lib.ptr(ls), _lib.ptr(ms), ignore, _lib.ptr(out["probs"]),
                                      _lib.ptr(out["coef"]), _lib.ptr(out["class_loss"]), _lib.ptr(out["loss"]),
                                      _lib.ptr(out["dlogits"]), _lib.ptr(out["order"]), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _bits(a):
    return a.view(np.int32)


def _same_bits(a, b, keys=("probs", "coef", "class_loss", "loss", "dlogits", "order")):
    return all((a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_stages_vs_float64(dev, shape):
    N, C = shape
    x, label, inner, pure = _case(N, C)
    assert _lib.lib().sph3d_lovasz_softmax_supported(N, C) == 1
    got = _call(dev, x, label, inner)
    staged = lovasz.lovasz_reference(x, label, inner, probs=got["probs"])
    f = R.check_stages(got, x, label, inner, staged, pure)
    print("N=%d C=%d: fractions of the bounds: probs %.3f  coef %.3f  class_loss %.3f  loss %.3f  dlogits %.3f  end to end %.4f"
          % (N, C, f["probs"], f["coef"], f["class_loss"], f["loss"], f["dlogits"], f["end_to_end"]))
    assert f["order_equal"], "the sorted order differs from the statement on the device's probs"
    for k in ("probs", "coef", "class_loss", "loss", "dlogits", "end_to_end"):
        assert f[k] <= 1.0, (k, f[k])
    # the block without a valid row: exact zeros and an order of -1; rows that are not valid: exact zeros
    valid = R.valid_rows(label, inner)
    assert not _bits(got["loss"][:1]).any() and not got["class_loss"][0].any() and (got["order"][0] == -1).all()
    assert not got["coef"][~valid].any() and not got["dlogits"][~valid].any()
    # a second call: the same bits in every output
    assert _same_bits(_call(dev, x, label, inner), got)
    # order == NULL and dlogits == NULL: everything else, loss above all, keeps its bits
    for grad, order in ((True, False), (False, True), (False, False)):
        part = _call(dev, x, label, inner, grad=grad, order=order)
        assert (part["dlogits"] is None) == (not grad) and (part["order"] is None) == (not order)
        keys = ["probs", "coef", "class_loss", "loss"] + (["dlogits"] if grad else []) + (["order"] if order else [])
        assert _same_bits(part, got, keys), (grad, order)


def test_no_mask_and_another_ignore_value(dev):
    """inner == NULL counts every row; ignore = 3 drops the rows labelled 3 (the inputs' -1 labels become 3 first)"""
    N, C = 1025, 13
    x, label, _, _ = _case(N, C)
    label = np.where(label == R.IGNORE, 3, label)
    got = _call(dev, x, label, None, ignore=3)
    staged = lovasz.lovasz_reference(x, label, None, ignore=3, probs=got["probs"])
    pure = lovasz.lovasz_reference(x, label, None, ignore=3)
    assert not pure["present"][:, 3].any() and (pure["n_valid"] == (label != 3).sum(1)).all()
    # (check_stages takes the valid rows from label and mask: hand it a mask that says what ignore = 3 says)
    f = R.check_stages(got, x, np.where(label == 3, R.IGNORE, label), None, staged, pure)
    assert f["order_equal"] and all(f[k] <= 1.0 for k in ("probs", "coef", "class_loss", "loss", "dlogits", "end_to_end")), f


@pytest.mark.parametrize("shape", [(1025, 13), (8192, 2)], ids=lambda s: "N%d-C%d" % s)
def test_bad_label_makes_its_block_nan(dev, shape):
    N, C = shape
    x, label, inner, _ = _case(N, C)
    clean = _call(dev, x, label, inner)
    # on rows that are not valid a label outside the classes changes nothing
    off = label.copy()
    off[0, 0], off[0, N - 1] = R.BAD_LABELS
    out = np.flatnonzero(~R.valid_rows(label, inner)[3])
    off[3, out[0]], off[3, out[-1]] = R.BAD_LABELS
    assert _same_bits(_call(dev, x, off, inner), clean)
    # on a valid row: the block's loss and every row of its gradient are NaN; the other blocks keep their bits
    for b, n in ((1, N - 2), (3, np.flatnonzero(R.valid_rows(label, inner)[3])[1])):
        for v in R.BAD_LABELS:
            bad = label.copy()
            bad[b, n] = v
            got = _call(dev, x, bad, inner)
            assert np.isnan(got["loss"][b]) and np.isnan(got["dlogits"][b]).all()
            others = [k for k in range(4) if k != b]
            for key in ("probs", "coef", "class_loss", "loss", "dlogits", "order"):
                assert np.array_equal(_bits(got[key][others]), _bits(clean[key][others])), (b, key)
            assert (got["order"][b] >= -1).all() and (got["order"][b] < N).all()
    # logits that are not finite on a valid row do the same; on a row that is not valid they stay in that row
    xn = x.copy()
    xn[1, 2, 0] = np.nan                      # (rows 0..2 are never ignored)
    xn[2, 1, :] = np.inf
    got = _call(dev, xn, label, inner)
    assert np.isnan(got["loss"][1]) and np.isnan(got["dlogits"][1]).all()
    assert np.array_equal(_bits(got["loss"][[0, 2, 3]]), _bits(clean["loss"][[0, 2, 3]]))
    assert np.array_equal(_bits(got["dlogits"][[0, 2, 3]]), _bits(clean["dlogits"][[0, 2, 3]]))


def test_autograd_and_no_grad(dev):
    N, C = 8192, 13
    x, label, inner, _ = _case(N, C)
    direct = _call(dev, x, label, inner, order=False)
    pred = torch.from_numpy(x).to(dev).requires_grad_(True)
    lab, inn = torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], device=dev)
    out = tf_loss.lovasz_softmax(pred, lab, inn)
    assert out.shape == (4,) and np.array_equal(_bits(out.detach().cpu().numpy()), _bits(direct["loss"]))
    (out * w).sum().backward()
    want = direct["dlogits"] * w.cpu().numpy()[:, None, None]
    assert np.array_equal(_bits(pred.grad.cpu().numpy()), _bits(want))
    # without a mask: the statement with every row counted
    free = tf_loss.lovasz_softmax(pred.detach(), lab).cpu().numpy()
    ref = lovasz.lovasz_reference(x, label)
    assert (np.abs(free - ref["loss"]) <= R.end_to_end_bound(x, label, None, ref["loss"])).all() and ref["n_valid"][0] > 0
    # no_grad: no [B, N, C] gradient is allocated (the scratch is warm by now)
    nbytes = 4 * x.size
    for grad in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.enable_grad() if grad else torch.no_grad():
            res = tf_loss.lovasz_softmax(pred, lab, inn)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert (peak >= nbytes) == grad, (grad, peak, nbytes)
        assert np.array_equal(_bits(res.detach().cpu().numpy()), _bits(direct["loss"]))
    with pytest.raises(_lib.Sph3dError):
        tf_loss.lovasz_softmax(pred.detach().cpu(), lab.cpu(), inn.cpu())


def test_harness_loss_dispatch(dev):
    """loss() on device tensors is the kernels' sum and lies within the end-to-end bound of the torch statement (float64, same
    device); a block of more than 16384 points goes to the torch statement"""
    N, C = 4097, 13
    x, label, inner, pure = _case(N, C)
    pred, lab, inn = torch.from_numpy(x).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    got = lovasz.loss(pred, lab, inn)
    assert torch.equal(got, tf_loss.lovasz_softmax(pred, lab, inn).sum())
    blocks = lovasz.lovasz_torch(pred.double(), lab, inn)
    assert np.abs(blocks.cpu().numpy() - pure["loss"]).max() <= 1e-12
    direct = _call(dev, x, label, inner, order=True)
    staged = lovasz.lovasz_reference(x, label, inner, probs=direct["probs"])
    bound = R.check_stages(direct, x, label, inner, staged, pure)["end_to_end_bound"]
    assert abs(float(got) - float(blocks.sum())) <= bound.sum() + 4 * R.U * pure["loss"].sum()      # (+ the sum of four blocks)
    bx, bl, _ = R.lovasz_inputs(4, 16385, 2)
    big, big_label = torch.from_numpy(bx[1:2]).to(dev), torch.from_numpy(bl[1:2]).to(dev)
    assert not tf_loss.supported(16385, 2)
    assert torch.equal(lovasz.loss(big, big_label), lovasz.lovasz_torch(big, big_label).sum())
    with pytest.raises(_lib.Sph3dError):
        tf_loss.lovasz_softmax(big, big_label)


def _train(dev, loss_of, steps=3):
    """three deterministic Trainer steps (six blocks, B = 2) on small_config(1024) from one seed -> (mean loss, parameter bits)"""
    from sph3d_gcn_amd.harness import feed, optim, s3dis_net, train
    rng = np.random.RandomState(3)
    blocks = []
    for n in (1500, 1024, 900, 2000, 1100, 1300):
        b = np.empty((n, 8), np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array([1.0, 1.0, 1.5])
        b[:, 3:6] = rng.rand(n, 3)
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        blocks.append(b)
    pool = feed.BlockPool.from_blocks(blocks, dev)
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(1024), device=dev, seed=3)
    prime = feed.assemble(pool.rows, pool.offsets, torch.from_numpy(np.asarray([0, 1], np.int32)).to(dev), 1024, 5, 0, True)
    tr = train.Trainer(model, loss_of(model), lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, 2), 13,
                       prime=prime, seed=5, log=lambda s: None, log_every=1, deterministic=True)
    f = feed.DeviceFeed(pool, 2, 1024, seed=5, augment=True)
    tr.metrics.reset()
    for item in f:
        tr.train_step(item, f)
    r = tr.metrics.read()
    assert tr.global_step == steps and r.batches == steps
    assert np.isfinite(r.mean_loss) and r.nonfinite == 0 and r.update_nonfinite == 0 and r.bad_label == 0
    return r.mean_loss, tr.flat.flat_param.detach().clone().view(torch.int32)


def test_training_with_the_loss_added(dev):
    la, pa = _train(dev, lambda m: lovasz.with_xent(m.loss, 1.0))
    lb, pb = _train(dev, lambda m: lovasz.with_xent(m.loss, 1.0))
    assert la == lb and torch.isfinite(pa.view(torch.float32)).all() and torch.equal(pa, pb)
    _, p0 = _train(dev, lambda m: lovasz.with_xent(m.loss, 0.0))
    _, plain = _train(dev, lambda m: m.loss)
    assert torch.equal(p0, plain), "with_xent(weight=0) changes the run"
    assert not torch.equal(pa, plain), "the added loss changes nothing"
    _ref.clear()
