"""The Lovasz-softmax loss with the sort in global memory (csrc/lovasz.hip: sph3d_lovasz_softmax_large) on the device against the
float64 statement (harness/lovasz.py), stage by stage and end to end, as tests/test_gpu_lovasz.py holds the existing entry;
tests/_lovasz_large_ref.py restates the one bound that differs (the summation tree of class_loss).  The sorted order must be EXACT,
and probs, order and coef must carry the existing entry's bits wherever both cover the shape: that is the cheapest strong check of
the merge.  A forced run length of 1024 reaches every merge shape at small N (one run, a second run of one row, odd run counts, a
last run alone in its pass); forced slabs must not change a bit.
Measured on an MI355X, worst over the 19 shapes, as fractions of the bounds: probs 0.297, coef 0.646, class_loss 0.123, loss 0.067,
dlogits 0.372, end to end 0.015."""
import ctypes

import numpy as np
import pytest
import torch

import _lovasz_large_forms as S
import _lovasz_large_ref as RL
import _lovasz_ref as R
from sph3d_gcn_amd import _lib, tf_loss
from sph3d_gcn_amd.harness import lovasz

pytestmark = pytest.mark.gpu

FORCED = [(N, C, 10) for N in (1, 1024, 1025, 2049, 3072, 4097, 5121, 8192) for C in (2, 13)]
DEFAULT = [(16385, 2, 0), (40000, 13, 0), (65536, 2, 0)]
KEYS = ("probs", "coef", "class_loss", "loss", "dlogits", "order")

_ref = {}


def _case(N, C):
    if (N, C) not in _ref:
        x, label, inner = R.lovasz_inputs(4, N, C)
        _ref[(N, C)] = (x, label, inner, lovasz.lovasz_reference(x, label, inner))
    return _ref[(N, C)]


def _outputs(dev, B, N, C, grad, order):
    nan = float("nan")
    return dict(probs=torch.full((B, N, C), nan, device=dev), coef=torch.full((B, N, C), nan, device=dev),
                class_loss=torch.full((B, C), nan, device=dev), loss=torch.full((B,), nan, device=dev),
                dlogits=torch.full((B, N, C), nan, device=dev) if grad else None,
                order=torch.full((B, C, N), -7, dtype=torch.int32, device=dev) if order else None)


def _call(dev, x, label, inner, tile_log2=0, slab=0, grad=True, order=True, ignore=R.IGNORE, large=True):
    """one C-ABI call on NaN-filled (order: -7-filled) outputs and a 0xff-filled workspace -> dict of numpy arrays"""
    l = _lib.lib()
    B, N, C = x.shape
    xs, ls = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, label))
    ms = torch.from_numpy(np.ascontiguousarray(inner)).to(dev) if inner is not None else None
    out = _outputs(dev, B, N, C, grad, order)
    head = [B, N, C, _lib.ptr(xs), _lib.ptr(ls), _lib.ptr(ms), ignore, _lib.ptr(out["probs"]), _lib.ptr(out["coef"]),
            _lib.ptr(out["class_loss"]), _lib.ptr(out["loss"]), _lib.ptr(out["dlogits"]), _lib.ptr(out["order"])]
    if large:
        fields = (ctypes.c_longlong * len(S.FIELDS))()
        _lib.check(l.sph3d_lovasz_softmax_large_plan(B, N, C, tile_log2, slab, ctypes.addressof(fields)))
        nbytes = dict(zip(S.FIELDS, fields))["workspace_bytes"]
        assert nbytes == S.plan(B, N, C, tile_log2, slab)["workspace_bytes"]
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)
        _lib.check(l.sph3d_lovasz_softmax_large(*head, _lib.ptr(ws), nbytes, tile_log2, slab, _lib.stream_ptr()))
    else:
        _lib.check(l.sph3d_lovasz_softmax(*head, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _bits(a):
    return a.view(np.int32)


def _same_bits(a, b, keys=KEYS):
    return all((a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


@pytest.mark.parametrize("shape", FORCED + DEFAULT, ids=lambda s: "N%d-C%d-tile%d" % s)
def test_stages_vs_float64(dev, shape):
    N, C, t = shape
    tile = 1 << (t or S.DEFAULT_TILE_LOG2)
    x, label, inner, pure = _case(N, C)
    assert _lib.lib().sph3d_lovasz_softmax_large_supported(N, C) == 1
    got = _call(dev, x, label, inner, t)
    staged = lovasz.lovasz_reference(x, label, inner, probs=got["probs"])
    f = RL.check_stages_large(got, x, label, inner, staged, pure, tile)
    print("N=%d C=%d tile=%d: fractions of the bounds: probs %.3f  coef %.3f  class_loss %.3f  loss %.3f  dlogits %.3f  end to end %.4f"
          % (N, C, tile, f["probs"], f["coef"], f["class_loss"], f["loss"], f["dlogits"], f["end_to_end"]))
    assert f["order_equal"], "the sorted order differs from the statement on the device's probs"
    for k in ("probs", "coef", "class_loss", "loss", "dlogits", "end_to_end"):
        assert f[k] <= 1.0, (k, f[k])
    # the block without a valid row: exact zeros and an order of -1; rows that are not valid: exact zeros
    valid = R.valid_rows(label, inner)
    assert not _bits(got["loss"][:1]).any() and not got["class_loss"][0].any() and (got["order"][0] == -1).all()
    assert not got["coef"][~valid].any() and not got["dlogits"][~valid].any()
    assert not got["class_loss"][~staged["present"]].any() and not got["coef"][np.broadcast_to(~staged["present"][:, None, :], got["coef"].shape)].any()
    # a second call: the same bits in every output
    assert _same_bits(_call(dev, x, label, inner, t), got)
    # order == NULL and dlogits == NULL: everything else, loss above all, keeps its bits
    for grad, order in ((True, False), (False, True), (False, False)):
        part = _call(dev, x, label, inner, t, grad=grad, order=order)
        assert (part["dlogits"] is None) == (not grad) and (part["order"] is None) == (not order)
        keys = ["probs", "coef", "class_loss", "loss"] + (["dlogits"] if grad else []) + (["order"] if order else [])
        assert _same_bits(part, got, keys), (grad, order)
    # where the existing entry covers the shape: its bits in probs, order and coef
    if N <= lovasz.MAX_N:
        assert _same_bits(_call(dev, x, label, inner, large=False), got, ("probs", "order", "coef"))


def test_slabs_keep_every_bit(dev):
    N, C = 4097, 13
    x, label, inner, _ = _case(N, C)
    whole = _call(dev, x, label, inner, 10, 0)
    assert S.plan(4, N, C, 10, 0)["slabs"] == 1
    for slab in (1, 5):
        assert S.plan(4, N, C, 10, slab)["slabs"] == -(-C // slab) > 1
        assert _same_bits(_call(dev, x, label, inner, 10, slab), whole), slab


def test_bad_label_makes_its_block_nan(dev):
    """labels far outside the classes and logits that are not finite, on valid rows: no read leaves its array (the count kernel checks
    a label before it indexes with it, the sort only compares it, every other index is a row below N or a class below C)"""
    N, C, t = 1025, 13, 10
    x, label, inner, _ = _case(N, C)
    clean = _call(dev, x, label, inner, t)
    # on rows that are not valid a label outside the classes changes nothing
    off = label.copy()
    off[0, 0], off[0, N - 1] = R.BAD_LABELS
    out = np.flatnonzero(~R.valid_rows(label, inner)[3])
    off[3, out[0]], off[3, out[-1]] = R.BAD_LABELS
    assert _same_bits(_call(dev, x, off, inner, t), clean)
    others = lambda b: [k for k in range(4) if k != b]
    for b, n in ((1, N - 2), (3, np.flatnonzero(R.valid_rows(label, inner)[3])[1])):
        for v in R.BAD_LABELS:
            bad = label.copy()
            bad[b, n] = v
            got = _call(dev, x, bad, inner, t)
            assert np.isnan(got["loss"][b]) and np.isnan(got["dlogits"][b]).all()
            for key in KEYS:
                assert np.array_equal(_bits(got[key][others(b)]), _bits(clean[key][others(b)])), (b, key)
            assert (got["order"][b] >= -1).all() and (got["order"][b] < N).all()
    # logits that are not finite on a valid row do the same; on a row that is not valid they stay in that row
    xn = x.copy()
    xn[1, 2, 0] = np.nan                      # (rows 0..2 are never ignored)
    xn[2, 1, :] = np.inf
    got = _call(dev, xn, label, inner, t)
    assert np.isnan(got["loss"][1]) and np.isnan(got["dlogits"][1]).all()
    assert (got["order"] >= -1).all() and (got["order"] < N).all()
    for key in ("loss", "dlogits", "class_loss", "coef", "order"):
        assert np.array_equal(_bits(got[key][others(1)]), _bits(clean[key][others(1)])), key


def test_batch_scope(dev):
    N, C = 1025, 13
    x, label, inner, _ = _case(N, C)
    pred, lab, inn = torch.from_numpy(x).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    got = tf_loss.lovasz_softmax_large(pred, lab, inn, scope="batch")
    flat = tf_loss.lovasz_softmax_large(pred.reshape(1, 4 * N, C), lab.reshape(1, -1), inn.reshape(1, -1))
    assert got.shape == (1,) and torch.equal(got.view(torch.int32), flat.view(torch.int32))
    direct = _call(dev, x.reshape(1, 4 * N, C), label.reshape(1, -1), inner.reshape(1, -1), grad=False, order=False)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(direct["loss"]))
    ref = lovasz.lovasz_reference(x, label, inner, scope="batch")
    bound = RL.end_to_end_bound_large(x.reshape(1, 4 * N, C), label.reshape(1, -1), inner.reshape(1, -1), ref["loss"])
    err = abs(float(got) - ref["loss"][0])
    print("batch scope [4, %d, %d]: end to end %.4f of the bound" % (N, C, err / bound[0]))
    assert ref["loss"][0] > 0 and err <= bound[0]
    with pytest.raises(ValueError):
        tf_loss.lovasz_softmax_large(pred, lab, inn, scope="image")


def test_autograd_and_no_grad(dev):
    N, C = 4097, 13
    x, label, inner, _ = _case(N, C)
    direct = _call(dev, x, label, inner, order=False)
    pred = torch.from_numpy(x).to(dev).requires_grad_(True)
    lab, inn = torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], device=dev)
    out = tf_loss.lovasz_softmax_large(pred, lab, inn)
    assert out.shape == (4,) and np.array_equal(_bits(out.detach().cpu().numpy()), _bits(direct["loss"]))
    (out * w).sum().backward()
    want = direct["dlogits"] * w.cpu().numpy()[:, None, None]
    assert np.array_equal(_bits(pred.grad.cpu().numpy()), _bits(want))
    # no_grad: no [B, N, C] gradient is allocated (the scratch is warm by now)
    nbytes = 4 * x.size
    for grad in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.enable_grad() if grad else torch.no_grad():
            res = tf_loss.lovasz_softmax_large(pred, lab, inn)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert (peak >= nbytes) == grad, (grad, peak, nbytes)
        assert np.array_equal(_bits(res.detach().cpu().numpy()), _bits(direct["loss"]))
    with pytest.raises(_lib.Sph3dError):
        tf_loss.lovasz_softmax_large(pred.detach().cpu(), lab.cpu(), inn.cpu())


def test_harness_loss_dispatch(dev):
    """large=True: blocks the LDS sort covers stay with it, larger ones go to the global sort; without it nothing changes"""
    bx, bl, _ = R.lovasz_inputs(4, 16385, 2)
    big, big_label = torch.from_numpy(bx[1:2]).to(dev), torch.from_numpy(bl[1:2]).to(dev)
    assert not tf_loss.supported(16385, 2) and tf_loss.supported_large(16385, 2)
    got = lovasz.loss(big, big_label, large=True)
    assert torch.equal(got, tf_loss.lovasz_softmax_large(big, big_label).sum())
    plain = lovasz.loss(big, big_label)
    assert torch.equal(plain, lovasz.lovasz_torch(big, big_label).sum())
    ref = lovasz.lovasz_reference(bx[1:2], bl[1:2])
    assert abs(float(got) - ref["loss"][0]) <= RL.end_to_end_bound_large(bx[1:2], bl[1:2], None, ref["loss"])[0]
    x, label, inner, _ = _case(4097, 13)
    pred, lab, inn = torch.from_numpy(x).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)
    assert torch.equal(lovasz.loss(pred, lab, inn, large=True), tf_loss.lovasz_softmax(pred, lab, inn).sum())
    # batch scope: 4 * 4097 rows are one block beyond the LDS sort; 4 * 1025 are not
    assert torch.equal(lovasz.loss(pred, lab, inn, scope="batch", large=True), tf_loss.lovasz_softmax_large(pred, lab, inn, scope="batch").sum())
    assert torch.equal(lovasz.loss(pred, lab, inn, scope="batch"), lovasz.lovasz_torch(pred, lab, inn, scope="batch").sum())
    small = _case(1025, 13)
    ps, ls, ms = (torch.from_numpy(a).to(dev) for a in small[:3])
    want = tf_loss.lovasz_softmax(ps.reshape(1, -1, 13), ls.reshape(1, -1), ms.reshape(1, -1)).sum()
    assert torch.equal(lovasz.loss(ps, ls, ms, scope="batch"), want) and torch.equal(lovasz.loss(ps, ls, ms, scope="batch", large=True), want)


def test_descent_with_the_batch_loss_added(dev):
    """three steps of plain gradient descent on the logits themselves, no Trainer and no model, with
    with_xent(..., scope="batch", large=True) as the loss: finite and decreasing"""
    N, C = 4097, 13
    x, label, inner, _ = _case(N, C)
    pred = torch.from_numpy(x).to(dev).requires_grad_(True)
    lab, inn = torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)

    def xent(p, l, *rest):
        return tf_loss.softmax_xent(p, l, *rest[:1], ignore=R.IGNORE, scope="batch").sum()
    loss_fn = lovasz.with_xent(xent, 1.0, scope="batch", large=True)
    losses = []
    for _ in range(3):
        pred.grad = None
        value = loss_fn(pred, lab, inn)
        value.backward()
        losses.append(float(value.detach()))
        with torch.no_grad():
            pred -= 100.0 * pred.grad
    assert np.isfinite(losses).all() and torch.isfinite(pred).all() and losses[0] > losses[1] > losses[2], losses
    alone = float(xent(torch.from_numpy(x).to(dev), lab, inn))
    assert losses[0] > alone, "the added loss adds nothing"
    _ref.clear()
