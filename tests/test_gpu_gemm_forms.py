"""Every launch form of the pointwise products (tests/_gemm_forms.py: FORM_CASES, the smallest shape that reaches each form) through
the C ABI against float64, under the products' bounds of tests/test_gpu_gemm_split.py: |error| <= 1e-5 of the element's summed term
magnitudes and, for the split forms, <= max(4 x the fp32 kernel's own error at the same shape, 4e-7); outputs start as NaN and the
workspace as 0xFF bytes, so an element no workgroup writes, or a slab that is summed without having been written, fails.  The
statistics forms also compare their partial sums, the exchange forms a second call bit for bit.  The guarded forms are reached
through ragged dimensions; operands are 16-byte aligned throughout (misaligned pointers: tests/test_gemm_forms.py, on the host)."""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_forms as G
from sph3d_gcn_amd import _lib

pytestmark = pytest.mark.gpu

CASES = [c for c in G.FORM_CASES if c[5] == 1 and not c[0].endswith("none")]
_runs = {}


@pytest.fixture
def modes():
    l = _lib.lib()
    prev = l.sph3d_pointwise_gemm_mode(-1)
    yield l
    l.sph3d_pointwise_gemm_mode(prev)


def _operands(dev, product, R, Ci, Co):
    """-> (a, b, bias, float64 product, summed term magnitudes), computed once per product and shape"""
    key = ("ops", product, R, Ci, Co)
    if key not in _runs:
        g = torch.Generator(device=dev).manual_seed(1000 * product + R + Ci + Co)
        if product == G.NNS:
            # as test_split_statistics_epilogue: operands of one scale, a bias
            x, w = torch.randn(R, Ci, device=dev, generator=g), torch.randn(Ci, Co, device=dev, generator=g) / Ci ** 0.5
            bias = torch.randn(Co, device=dev, generator=g)
            _runs[key] = (x, w, bias, x.double() @ w.double() + bias.double(), x.double().abs() @ w.double().abs() + bias.double().abs())
            return _runs[key]
        # as test_split_products_vs_float64_and_fp32_kernels: the row operands over ~12 binades with both signs
        a = torch.randn(R, Ci, device=dev, generator=g) * torch.exp2(torch.randint(-6, 6, (R, Ci), device=dev, generator=g).float())
        if product == G.TN:
            b = torch.randn(R, Co, device=dev, generator=g) * torch.exp2(torch.randint(-6, 6, (R, Co), device=dev, generator=g).float())
            want, mag = a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs()
        elif product == G.NT:
            b = torch.randn(Co, Ci, device=dev, generator=g) / Ci ** 0.5                        # W stored [Cout][Cin]
            want, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
        else:
            b = torch.randn(Ci, Co, device=dev, generator=g) / Ci ** 0.5
            want, mag = a.double() @ b.double(), a.double().abs() @ b.double().abs()
        _runs[key] = (a, b, None, want, mag)
    return _runs[key]


def _call(l, dev, product, R, Ci, Co):
    """one call through the C ABI on a NaN-filled output and a 0xFF-filled workspace -> (output, partial sums or None)"""
    a, b, bias, _, _ = _operands(dev, product, R, Ci, Co)
    st = _lib.stream_ptr()
    if product == G.TN:
        out = torch.full((Ci, Co), float("nan"), device=dev)
        nbytes = l.sph3d_pointwise_gemm_tn_workspace(R, Ci, Co)
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(l.sph3d_pointwise_gemm_tn(R, Ci, Co, _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), _lib.ptr(ws), nbytes, st))
        return out, None
    out = torch.full((R, Co), float("nan"), device=dev)
    if product == G.NNS:
        partial = torch.full((l.sph3d_pointwise_gemm_bnstats_blocks(R, Ci, Co), 2, Co), float("nan"), device=dev)
        _lib.check(l.sph3d_pointwise_gemm_bnstats(R, Ci, Co, _lib.ptr(a), _lib.ptr(b), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(partial), st))
        return out, partial
    _lib.check(l.sph3d_pointwise_gemm(R, Ci, Co, _lib.ptr(a), _lib.ptr(b), None, 0, int(product == G.NT), _lib.ptr(out), st))
    return out, None


def _error(l, dev, product, R, Ci, Co, mode):
    """max over the elements of |error| / summed term magnitudes in `mode`; the fp32 kernels' (mode 0) once per product and shape"""
    key = ("err", product, R, Ci, Co, mode)
    if key not in _runs:
        l.sph3d_pointwise_gemm_mode(mode)
        _, _, _, want, mag = _operands(dev, product, R, Ci, Co)
        out, partial = _call(l, dev, product, R, Ci, Co)
        _runs[key] = (float(((out.double() - want).abs() / mag).max()), out, partial)        # (NaN if an element was not written)
    return _runs[key]


def _plan(l, product, R, Ci, Co, mode):
    out = (ctypes.c_int * len(G.FIELDS))()
    assert l.sph3d_pointwise_gemm_plan(product, R, Ci, Co, 1, mode, 1, ctypes.cast(out, ctypes.c_void_p)) == 0
    return dict(zip(G.FIELDS, out))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0].replace(" ", "-"))
def test_form_vs_float64(dev, modes, case):
    tag, product, R, Ci, Co, _, mode, _ = case
    plan = _plan(modes, product, R, Ci, Co, mode)
    assert G.tag(product, plan) == tag
    a, b, bias, want, _ = _operands(dev, product, R, Ci, Co)
    assert all(t is None or t.data_ptr() % 16 == 0 for t in (a, b, bias))
    err, out, partial = _error(modes, dev, product, R, Ci, Co, mode)
    print("%s: error / term magnitudes %.3g" % (tag, err))
    assert err <= 1e-5, (tag, err)
    if plan["pipe"] == G.SPLIT:
        e_f32 = _error(modes, dev, product, R, Ci, Co, 0)[0]
        print("%s: fp32 kernels %.3g" % (tag, e_f32))
        assert err <= max(4 * e_f32, 4e-7), (tag, err, e_f32)
    if product == G.NNS:
        assert plan["stats_blocks"] == partial.shape[0] > 0
        z = torch.where(want > 0, want, torch.expm1(want))
        p = partial.double().sum(0)
        np.testing.assert_allclose(out.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose((p[0] / R).cpu().numpy(), (z.sum(0) / R).cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose((p[1] / R).cpu().numpy(), ((z * z).sum(0) / R).cpu().numpy(), rtol=1e-5, atol=1e-6)
    if plan["xs"] > 1:
        # fixed summation order, arrival counters back at zero: a second call is bit-equal
        modes.sph3d_pointwise_gemm_mode(mode)
        out2, partial2 = _call(modes, dev, product, R, Ci, Co)
        assert torch.equal(out2, out) and (partial is None or torch.equal(partial2, partial))


def test_no_exchange_gave_up_waiting_and_references_are_released(dev):
    assert _lib.lib().sph3d_pointwise_gemm_exchange_failures() == 0
    _runs.clear()
