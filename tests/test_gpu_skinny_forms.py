"""Every launch form of the logits layer (csrc/skinny.hip; tests/_head_ref.py: FORM_CASES, the smallest shape that reaches each form)
through the C ABI: sph3d_pointwise_gemm_skinny and sph3d_pointwise_gemm_skinny_tn on outputs that start as NaN and a workspace of
exactly ..._tn_workspace bytes that starts as 0xFF, so an element no lane stores, or a slab that is summed without having been
written, fails.  Two operand sets per case:
  exact    small integers (|a|, |w|, |dY| <= 4, an integer bias), different in every row and column: every partial sum is an integer
           below 2^24, so the result must equal the int64 product cast to float32 bit for bit — whatever R, a single dropped,
           doubled or misplaced row or channel shows;
  rounded  the operands of tests/test_gpu_gemm_forms.py (row operands over ~12 binades with both signs, weights / sqrt(K)) against
           the float64 statement under the products' bound of tests/test_gpu_gemm_split.py: |error| <= 1e-5 x the element's summed
           term magnitudes.  Measured worst ratios on an MI355X: forward 2.2e-7, weight gradient 1.9e-7, input gradients 3.2e-7.
A second call is bit-equal (the summation order is fixed).  Refusals launch nothing and leave the output NaN."""
import numpy as np
import pytest
import torch

import _gemm_forms as G
import _head_ref as H
import test_gpu_gemm_forms as gemm_forms
from sph3d_gcn_amd import _lib

pytestmark = pytest.mark.gpu

BOUND = 1e-5
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _rounded(dev, product, R, K1, K2, N):
    """the operands of test_gpu_gemm_forms._operands at (R, K1 + K2, N), the row operand cut into the two halves"""
    a, b = gemm_forms._operands(dev, product, R, K1 + K2, N)[:2]
    gemm_forms._runs.pop(("ops", product, R, K1 + K2, N), None)              # (that module's cache: nothing of ours stays in it)
    return a[:, :K1].contiguous(), (a[:, K1:].contiguous() if K2 else None), b


def _nn_operands(dev, kind, R, K1, K2, N, bias):
    """-> (a1, a2, w, bias) on the device"""
    if kind == "exact":
        return (_dev(H.int_operand(R, K1, 1), dev), _dev(H.int_operand(R, K2, 2), dev) if K2 else None,
                _dev(H.int_operand(K1 + K2, N, 3), dev), _dev(H.int_operand(1, N, 4, lim=9)[0], dev) if bias else None)
    a1, a2, w = _rounded(dev, G.NN, R, K1, K2, N)
    g = torch.Generator(device=dev).manual_seed(R + N)
    return a1, a2, w, torch.randn(N, device=dev, generator=g) if bias else None


def _tn_operands(dev, kind, R, K1, K2, N):
    """-> (a1, a2, dy) on the device"""
    if kind == "exact":
        return _dev(H.int_operand(R, K1, 5), dev), _dev(H.int_operand(R, K2, 6), dev) if K2 else None, _dev(H.int_operand(R, N, 7), dev)
    return _rounded(dev, G.TN, R, K1, K2, N)


def _call_nn(dev, R, K1, K2, N, a1, a2, w, bias):
    y = torch.full((R, N), float("nan"), device=dev)
    rc = _lib.lib().sph3d_pointwise_gemm_skinny(R, K1, K2, N, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y),
                                                _lib.stream_ptr())
    return rc, y


def _call_tn(dev, R, K1, K2, N, a1, a2, dy, short=0):
    l = _lib.lib()
    nbytes = l.sph3d_pointwise_gemm_skinny_tn_workspace(R, K1, K2, N)
    assert nbytes == H.skinny_tn_form(R, K1, K2)["slabs_bytes"]
    ws = torch.full((nbytes - short,), 255, dtype=torch.uint8, device=dev)
    dw = torch.full((K1 + K2, N), float("nan"), device=dev)
    rc = l.sph3d_pointwise_gemm_skinny_tn(R, K1, K2, N, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(ws), nbytes - short,
                                          _lib.stream_ptr())
    return rc, dw


def _check(what, kind, got, ops, statement, exact):
    """got (a device tensor) against the int64 product (exact) or the float64 statement under the bound (rounded)"""
    got, ops = _np(got), [_np(t) for t in ops]
    assert not np.isnan(got).any(), "%s %s: %d elements were not written" % (what, kind, int(np.isnan(got).sum()))
    if kind == "exact":
        want = exact(*ops)
        wrong = np.argwhere(got.view(np.int32) != want.view(np.int32))
        assert len(wrong) == 0, "%s exact: %d elements differ from the integer product, first at %s: %r != %r" % (
            what, len(wrong), tuple(wrong[0]), got[tuple(wrong[0])], want[tuple(wrong[0])])
        return 0.0
    want, mag = statement(*ops)
    ratio = float((np.abs(got.astype(np.float64) - want) / mag).max())
    print("%s: worst |error| / summed term magnitudes %.3g" % (what, ratio))
    assert ratio <= BOUND, (what, ratio)
    return ratio


@pytest.mark.parametrize("kind", ["exact", "rounded"])
@pytest.mark.parametrize("case", H.FORM_CASES["nn"], ids=lambda c: "R%d-K%d+%d-N%d-bias%d" % c[1:])
def test_forward_form(dev, case, kind):
    name, R, K1, K2, N, bias = case
    assert H.FORMS["nn"][name](H.skinny_nn_form(R, K1, K2, N), case[1:]) and _lib.lib().sph3d_pointwise_gemm_skinny_supported(R, K1, K2, N) == 1
    ops = _nn_operands(dev, kind, R, K1, K2, N, bias)
    assert all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) for t in ops[:2]) and (ops[3] is None) == (not bias)
    rc, y = _call_nn(dev, R, K1, K2, N, *ops)
    _lib.check(rc)
    _check("forward %s (%s)" % (case[1:], name), kind, y, ops, H.skinny_ref, H.int_product)
    rc, y2 = _call_nn(dev, R, K1, K2, N, *ops)
    _lib.check(rc)
    assert torch.equal(y2, y)


@pytest.mark.parametrize("kind", ["exact", "rounded"])
@pytest.mark.parametrize("case", H.FORM_CASES["tn"], ids=lambda c: "R%d-K%d+%d-N%d" % c[1:])
def test_weight_gradient_form(dev, case, kind):
    name, R, K1, K2, N = case
    assert H.FORMS["tn"][name](H.skinny_tn_form(R, K1, K2), case[1:]) and _lib.lib().sph3d_pointwise_gemm_skinny_supported(R, K1, K2, N) == 1
    ops = _tn_operands(dev, kind, R, K1, K2, N)
    assert all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) for t in ops[:2])
    rc, dw = _call_tn(dev, R, K1, K2, N, *ops)
    _lib.check(rc)
    _check("weight gradient %s (%s)" % (case[1:], name), kind, dw, ops, H.skinny_tn_ref, lambda a1, a2, dy: H.int_product(a1, a2, dy, transpose=True))
    rc, dw2 = _call_tn(dev, R, K1, K2, N, *ops)
    _lib.check(rc)
    assert torch.equal(dw2, dw)


def test_refusals_launch_nothing(dev):
    l = _lib.lib()

    def refused(want, R, K1, K2, N, a1, a2, b, short=0):
        """both entry points (b: the weights and, as [R, N] rows, the upstream gradient) refuse and leave their outputs NaN"""
        if short == 0:
            rc, y = _call_nn(dev, R, K1, K2, N, a1, a2, b, None)
            assert rc == want[0] and torch.isnan(y).all(), ("forward", R, K1, K2, N, rc)
        rc, dw = _call_tn(dev, R, K1, K2, N, a1, a2, torch.ones((R, N), device=dev), short=short)
        assert rc == want[1] and torch.isnan(dw).all(), ("weight gradient", R, K1, K2, N, rc)
        assert b"skinny" in l.sph3d_last_error()

    def ones(*shape):
        return torch.ones(shape, device=dev)

    R = 64
    # an operand that is 4-byte but not 16-byte aligned: a contiguous view at a storage offset of one float
    for K1, K2 in ((32, 0), (32, 32)):
        off = torch.ones(R * 32 + 1, device=dev)[1:].view(R, 32)
        assert off.is_contiguous() and off.data_ptr() % 16 == 4
        refused((EINVAL, EINVAL), R, K1, K2, 13, off, ones(R, 32) if K2 else None, ones(K1 + K2, 13))
        if K2:
            refused((EINVAL, EINVAL), R, K1, K2, 13, ones(R, 32), off, ones(K1 + K2, 13))
    # a workspace one byte short
    refused((None, EWORKSPACE), R, 32, 32, 13, ones(R, 32), ones(R, 32), None, short=1)
    # N = 17; K1 = 24; five started groups of 64 channels (16 + 240, 240 + 16, 112 + 144); K2 > 0 without its operand
    refused((EUNSUPPORTED, EUNSUPPORTED), R, 32, 32, 17, ones(R, 32), ones(R, 32), ones(64, 17))
    refused((EUNSUPPORTED, EUNSUPPORTED), R, 24, 0, 13, ones(R, 24), None, ones(24, 13))
    for R5, K1, K2, N in H.REFUSED_GROUPS:
        assert l.sph3d_pointwise_gemm_skinny_supported(R5, K1, K2, N) == 0
        refused((EUNSUPPORTED, EUNSUPPORTED), R5, K1, K2, N, ones(R5, K1), ones(R5, K2), ones(K1 + K2, N))
    refused((EUNSUPPORTED, EUNSUPPORTED), R, 32, 32, 13, ones(R, 32), None, ones(64, 13))
    torch.cuda.synchronize()


def _layer(a1, a2, w, bias, dy):
    """tf_gemm.linear_concat2 forward and backward -> (y, da1, da2 or None, dw, dbias or None)"""
    from sph3d_gcn_amd import tf_gemm
    leaves = [t.detach().clone().requires_grad_(True) if t is not None else None for t in (a1, a2, w, bias)]
    if not a1.is_contiguous():                                                # (keep the layout under test)
        leaves[0] = a1.detach().requires_grad_(True)
    y = tf_gemm.linear_concat2(*leaves)
    y.backward(dy)
    return (y.detach(),) + tuple(None if t is None else t.grad for t in (leaves[0], leaves[1], leaves[2], leaves[3]))


@pytest.mark.parametrize("kind", ["exact", "rounded"])
@pytest.mark.parametrize("shape", [(300, 48, 80, 13, 1), (77, 64, 0, 16, 0)], ids=lambda s: "R%d-K%d+%d-N%d-bias%d" % s)
def test_layer_through_the_wrappers(dev, shape, kind):
    """a non-contiguous a1 and a non-contiguous upstream gradient give the bits of the contiguous call; a2 = None and bias = None
    work; the input gradients of both halves against dY W[:K1]^T and dY W[K1:]^T under the same two checks"""
    R, K1, K2, N, has_bias = shape
    a1, a2, w, bias = _nn_operands(dev, kind, R, K1, K2, N, has_bias)
    dy = _tn_operands(dev, kind, R, K1, K2, N)[2]
    y, da1, da2, dw, db = _layer(a1, a2, w, bias, dy)
    what = "layer %s" % (shape,)
    _check(what + " y", kind, y, (a1, a2, w, bias), H.skinny_ref, H.int_product)
    _check(what + " dw", kind, dw, (a1, a2, dy), H.skinny_tn_ref, lambda p, q, g: H.int_product(p, q, g, transpose=True))
    halves = [(da1, w[:K1])] + ([(da2, w[K1:])] if K2 else [])
    for i, (got, wh) in enumerate(halves):
        assert got.shape == (R, wh.shape[0])
        _check(what + " da%d" % (i + 1), kind, got, (dy, None, wh.t().contiguous(), None), H.skinny_ref, H.int_product)
    assert (da2 is None) == (K2 == 0) and (db is None) == (not has_bias)
    if has_bias:
        assert db.shape == (N,) and float((db.double() - dy.double().sum(0)).abs().max()) <= 1e-5 * float(dy.double().abs().sum(0).max())
    # the same operands in other layouts: every second column of a wider a1, every second column of a wider upstream gradient
    wide = torch.empty((R, 2 * K1), device=dev)
    wide[:, ::2] = a1
    a1_nc = wide[:, ::2]
    gwide = torch.empty((R, 2 * N), device=dev)
    gwide[:, ::2] = dy
    assert not a1_nc.is_contiguous() and not gwide[:, ::2].is_contiguous()
    for other in (_layer(a1_nc, a2, w, bias, dy), _layer(a1, a2, w, bias, gwide[:, ::2])):
        for got, want in zip(other, (y, da1, da2, dw, db)):
            assert (got is None) == (want is None) and (got is None or torch.equal(got, want))
