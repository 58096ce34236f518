"""Every launch form of the training loss (csrc/loss.hip; tests/_head_ref.py: FORM_CASES) through the C ABI against the float64
statement, part by part and element by element: loss_part and dlogits start as NaN; every case holds a block without inner points
(all zeros, exactly), a block of inner points only, a block with exactly three inner points and a block whose mask is drawn from
0, 1, 2.5, -1 and NaN; the logit rows come at scale 1 and 30, with all classes equal, with one dominant class (+80) and shifted by
+-1000.  Bounds, u = 2^-24:
    gradient element   8 u inv_b (p (1 + |x| + |m|) + onehot)      (+ the smallest normal float32: p / cnt is below it where one
                                                                      class dominates by 80 in a block of 40 000 inner points)
    loss part          (8 + trips + 26) u sum over the part's inner rows of (|m| + |lse - m| + |x_y| + 1) / cnt_b
The float32 restatement of the kernel reaches 1.5 (loss) and 3.1 (gradient) of these units on the CPU with numpy's exp and log
(tests/test_head_ref.py).  Measured on an MI355X, worst over the cases: loss part 1.5 units, gradient element 3.1 units."""
import numpy as np
import pytest
import torch

import _head_ref as H
from sph3d_gcn_amd import _lib

pytestmark = pytest.mark.gpu

_ref = {}


def _case(B, N, C):
    """inputs and float64 statement, once per shape"""
    if (B, N, C) not in _ref:
        x, label, inner = H.xent_inputs(B, N, C)
        _ref[(B, N, C)] = (x, label, inner, H.xent_ref(x, label, inner))
    return _ref[(B, N, C)]


def _call(dev, x, label, inner, grad=True, B=None):
    """one call on NaN-filled outputs -> (loss_part [B, S], dlogits or None) as numpy"""
    l = _lib.lib()
    Bx, N, C = x.shape
    S = l.sph3d_masked_softmax_xent_parts(N)
    xs, ls, ms = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, label, inner))
    loss_part = torch.full((Bx, S), float("nan"), device=dev)
    d = torch.full((Bx, N, C), float("nan"), device=dev) if grad else None
    _lib.check(l.sph3d_masked_softmax_xent(Bx if B is None else B, N, C, _lib.ptr(xs), _lib.ptr(ls), _lib.ptr(ms), _lib.ptr(loss_part),
                                           _lib.ptr(d), _lib.stream_ptr()))
    return loss_part.cpu().numpy(), (d.cpu().numpy() if grad else None)


def _bits(a):
    return a.view(np.int32)


@pytest.mark.parametrize("case", H.FORM_CASES["xent"], ids=lambda c: "N%d-C%d" % c[2:])
def test_loss_form_vs_float64(dev, case):
    name, B, N, C = case
    x, label, inner, ref = _case(B, N, C)
    f = ref["form"]
    assert H.FORMS["xent"][name](f, case[1:]) and _lib.lib().sph3d_masked_softmax_xent_parts(N) == f["S"]
    loss_part, d = _call(dev, x, label, inner)
    assert loss_part.shape == ref["loss_part"].shape
    r_loss, r_grad = H.xent_check(loss_part, d, ref)
    print("N=%d C=%d (%s): worst loss part %.2f u of %d, worst gradient element %.2f u of %d"
          % ((N, C, name, r_loss) + (H.xent_allowed(ref)[0], r_grad, H.xent_allowed(ref)[1])))
    a_loss, a_grad = H.xent_allowed(ref)
    assert r_loss <= a_loss and r_grad <= a_grad, (r_loss, a_loss, r_grad, a_grad)
    # the block without inner points: exactly zero, every part and every element; rows that are not inner: exactly zero
    assert not _bits(loss_part[0]).any() and not d[0].any() and not d[~(inner > 0)].any()
    # the loss-only form (dlogits == NULL) and a second call: the same bits
    only, none = _call(dev, x, label, inner, grad=False)
    assert none is None and np.array_equal(_bits(only), _bits(loss_part))
    again, d2 = _call(dev, x, label, inner)
    assert np.array_equal(_bits(again), _bits(loss_part)) and np.array_equal(_bits(d2), _bits(d))


@pytest.mark.parametrize("shape", [(4, 16385, 13), (4, 1025, 2)], ids=lambda s: "N%d-C%d" % s[1:])
def test_labels_outside_the_classes(dev, shape):
    """labels 2^32 + 3 and -2^40 (the kernel's class comparison casts a label to int): on inner rows the row's part and its
    gradient row are NaN, the neighbouring rows and every other part and block stay finite and within bound; on rows that are not
    inner they change nothing"""
    B, N, C = shape
    x, label, inner, ref = _case(B, N, C)
    clean_part, clean_d = _call(dev, x, label, inner)
    # rows that are not inner: blocks 0 (no inner point), 2 (three inner points) and 3 (the drawn mask)
    off = label.copy()
    off[0, 0], off[0, N - 1] = H.BAD_LABELS
    off[2, 2], off[2, N - 3] = H.BAD_LABELS
    out = np.flatnonzero(~(inner[3] > 0))
    off[3, out[0]], off[3, out[-1]] = H.BAD_LABELS
    part, d = _call(dev, x, off, inner)
    assert np.array_equal(_bits(part), _bits(clean_part)) and np.array_equal(_bits(d), _bits(clean_d))
    # inner rows: blocks 1 (all inner; its first part and its last) and 3 (the mask's second and last but one inner row)
    bad = label.copy()
    rows = np.flatnonzero(inner[3] > 0)
    where = [(1, 5), (1, N - 1), (3, rows[1]), (3, rows[-2])]
    for i, (b, n) in enumerate(where):
        bad[b, n] = H.BAD_LABELS[i % 2]
    rb = H.xent_ref(x, bad, inner)
    assert int(np.isnan(rb["dlogits"]).sum()) == len(where) * C and 2 <= int(np.isnan(rb["loss_part"]).sum()) <= 4
    part, d = _call(dev, x, bad, inner)
    for b, n in where:
        assert np.isnan(d[b, n]).all() and np.isnan(part[b, n // rb["form"]["chunk"]])
        assert np.isfinite(d[b, n - 1]).all() and (n + 1 == N or np.isfinite(d[b, n + 1]).all())
    r_loss, r_grad = H.xent_check(part, d, rb)                                # (inf unless NaN stands exactly where the statement has it)
    print("N=%d C=%d, labels outside the classes: worst loss part %.2f u, worst gradient element %.2f u" % (N, C, r_loss, r_grad))
    a_loss, a_grad = H.xent_allowed(rb)
    assert r_loss <= a_loss and r_grad <= a_grad, (r_loss, a_loss, r_grad, a_grad)
    assert np.isfinite(part[[0, 2]]).all() and np.isfinite(d[[0, 2]]).all()
    # three blocks (B = 3): the same bits as the first three of four
    part3, d3 = _call(dev, x[:3], bad[:3], inner[:3])
    assert np.array_equal(_bits(part3), _bits(part[:3])) and np.array_equal(_bits(d3), _bits(d[:3]))


def test_no_block_writes_nothing(dev):
    x, label, inner, _ = _case(4, 1025, 13)
    part, d = _call(dev, x, label, inner, B=0)
    assert np.isnan(part).all() and np.isnan(d).all()
    _ref.clear()
