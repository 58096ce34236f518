"""``_op.differentiable``: one setup and one backward give the dispatcher registration AND the eager Function of an op.  A toy op
pair over CPU tensors (namespace ``sph3d_test``) shows that the two paths agree bit for bit, which gradient callable each one
hands to the backward, what happens to a non-differentiable output and to an input that needs no gradient; a static part holds
the package's seven ops to the list ``_op.WIRED``.  No device library is loaded."""
import collections
from typing import Tuple

import pytest
import torch

from sph3d_gcn_amd import _op, tf_conv3d, tf_gemm, tf_pool3d, tf_unpool3d

CHECKS = ("test_schema", "test_faketensor", "test_autograd_registration")


# ---- the toy ops: a gather-max with a non-differentiable index output (the shape of max_pool3d) and a two-input product whose
# gradient is the op itself (the shape of pointwise_gemm) ----
def _gather_max_impl(x: torch.Tensor, index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [N, C], index [M, K] -> out [M, C] = max_k x[index[m, k], c], arg [M, C] = the winning row of x"""
    vals, slot = x[index].max(dim=1)                                   # [M, K, C] -> [M, C]
    return vals, index.gather(1, slot)


def _gather_max_grad_impl(x: torch.Tensor, grad_out: torch.Tensor, arg: torch.Tensor) -> torch.Tensor:
    return torch.zeros_like(x).scatter_add(0, arg, grad_out)


def _product_impl(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a * b


Toy = collections.namedtuple("Toy", "gather_max gather_max_grad product seen counts")


@pytest.fixture(scope="module")
def toy():
    seen, counts = [], collections.Counter()
    gmax = torch.library.custom_op("sph3d_test::gather_max", mutates_args=())(_gather_max_impl)
    gmax.register_fake(lambda x, index: (x.new_empty((index.shape[0], x.shape[1])),
                                         index.new_empty((index.shape[0], x.shape[1]))))
    gmax_grad = torch.library.custom_op("sph3d_test::gather_max_grad", mutates_args=())(_gather_max_grad_impl)
    gmax_grad.register_fake(lambda x, grad_out, arg: torch.empty_like(x))
    prod = torch.library.custom_op("sph3d_test::product", mutates_args=())(_product_impl)
    prod.register_fake(lambda a, b: torch.empty_like(a))

    def gmax_setup(ctx, inputs, output):
        ctx.save_for_backward(inputs[0], output[1])
        ctx.mark_non_differentiable(output[1])

    def gmax_backward(grad, ctx, grad_out, grad_arg):
        seen.append(grad)
        x, arg = ctx.saved_tensors
        return grad(x, grad_out, arg), None

    def prod_setup(ctx, inputs, output):
        ctx.save_for_backward(*inputs)

    def prod_backward(grad, ctx, g):
        a, b = ctx.saved_tensors
        da = db = None
        if ctx.needs_input_grad[0]:
            counts["a"] += 1
            da = grad(g, b)
        if ctx.needs_input_grad[1]:
            counts["b"] += 1
            db = grad(g, a)
        return da, db

    n = len(_op.WIRED)
    t = Toy(_op.differentiable(gmax, _gather_max_impl, gmax_setup, gmax_backward, gmax_grad, _gather_max_grad_impl), gmax_grad,
            _op.differentiable(prod, _product_impl, prod_setup, prod_backward, prod, _product_impl), seen, counts)
    assert [op for op, _ in _op.WIRED[n:]] == [gmax, prod] and _op.WIRED[n][1] is t.gather_max
    del _op.WIRED[n:]                              # the list stays the package's own: other tests iterate over it
    return t


def _inputs():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 3, generator=g)
    index = torch.randint(0, 7, (5, 4), generator=g)
    go = torch.randn(5, 3, generator=g)
    return x, index, go


def test_both_paths_give_equal_outputs_and_gradients(toy):
    x, index, go = _inputs()
    ref, _ = x[index].max(dim=1)
    grads = []
    for fn in (torch.ops.sph3d_test.gather_max, toy.gather_max):
        leaf = x.clone().requires_grad_(True)
        out, arg = fn(leaf, index)
        assert out.requires_grad and not arg.requires_grad                # the index output is non-differentiable on both paths
        assert arg.dtype == torch.int64
        torch.testing.assert_close(out.detach(), ref, rtol=0, atol=0)
        out.backward(go)
        grads.append((out.detach(), arg, leaf.grad))
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    want = torch.zeros_like(x).index_put((grads[0][1], torch.arange(3).expand(5, 3)), go, accumulate=True)
    torch.testing.assert_close(grads[0][2], want, rtol=0, atol=0)


def test_backward_receives_the_registered_op_or_the_impl(toy):
    x, index, go = _inputs()
    del toy.seen[:]
    torch.ops.sph3d_test.gather_max(x.clone().requires_grad_(True), index)[0].backward(go)
    toy.gather_max(x.clone().requires_grad_(True), index)[0].backward(go)
    assert toy.seen == [toy.gather_max_grad, _gather_max_grad_impl]


def test_an_input_that_needs_no_gradient_gets_none_computed(toy):
    g = torch.Generator().manual_seed(1)
    a0, b0, go = (torch.randn(6, generator=g) for _ in range(3))
    for fn in (torch.ops.sph3d_test.product, toy.product):
        toy.counts.clear()
        a, b = a0.clone().requires_grad_(True), b0.clone()               # b: a leaf with requires_grad=False
        fn(a, b).backward(go)
        assert dict(toy.counts) == {"a": 1} and b.grad is None
        torch.testing.assert_close(a.grad, go * b0, rtol=0, atol=0)
        toy.counts.clear()
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        fn(a, b).backward(go)
        assert dict(toy.counts) == {"a": 1, "b": 1}
        torch.testing.assert_close(b.grad, go * a0, rtol=0, atol=0)


def test_opcheck_of_the_toy_ops(toy):
    x, index, _ = _inputs()
    torch.library.opcheck(torch.ops.sph3d_test.gather_max, (x.clone().requires_grad_(True), index), test_utils=CHECKS)
    torch.library.opcheck(torch.ops.sph3d_test.product, (x.clone().requires_grad_(True), x.clone().requires_grad_(True)),
                          test_utils=CHECKS)


# ---- the package's seven ops ----
PUBLIC = {   # registered op -> (module, public function, the module's name for the apply that differentiable() returned)
    "sph3d::depthwise_conv3d": (tf_conv3d, "depthwise_conv3d", "_depthwise_conv3d_apply"),
    "sph3d::fuzzy_depthwise_conv3d": (tf_conv3d, "fuzzy_depthwise_conv3d", "_fuzzy_depthwise_conv3d_apply"),
    "sph3d::max_pool3d": (tf_pool3d, "max_pool3d", "_max_pool3d_apply"),
    "sph3d::avg_pool3d": (tf_pool3d, "avg_pool3d", "_avg_pool3d_apply"),
    "sph3d::mean_interpolate": (tf_unpool3d, "mean_interpolate", "_mean_interpolate_apply"),
    "sph3d::weighted_interpolate": (tf_unpool3d, "weighted_interpolate", "_weighted_interpolate_apply"),
    "sph3d::pointwise_gemm": (tf_gemm, "matmul", "_pointwise_gemm_apply"),
}


def test_the_seven_public_functions_call_the_recorded_apply(toy, monkeypatch):
    wired = {op._qualname: apply for op, apply in _op.WIRED}
    assert len(wired) == len(_op.WIRED) and set(wired) == set(PUBLIC)
    for qualname, (module, public, apply_name) in PUBLIC.items():
        assert getattr(module, apply_name) is wired[qualname], qualname
        assert getattr(torch.ops.sph3d, qualname.split("::")[1]) is not None
        # the public function hands its arguments to that apply and to nothing else: stand in for it and call
        calls = []
        monkeypatch.setattr(module, apply_name, lambda *args: calls.append(args) or "out")
        fn = getattr(module, public)
        n_args = fn.__code__.co_argcount - len(fn.__defaults__ or ())
        args = tuple(object() for _ in range(n_args))
        assert fn(*args) == "out" and len(calls) == 1 and calls[0][:n_args] == args, qualname
    assert calls[0] == args + (False,)                                   # matmul(x, w): the eager path passes trans_w=False


def test_the_old_wirings_are_gone():
    gone = {tf_conv3d: ("_DepthwiseConv3dFn", "_FuzzyDepthwiseConv3dFn", "_conv_backward", "_fuzzy_backward"),
            tf_pool3d: ("_MaxPool3dFn", "_AvgPool3dFn", "_max_backward", "_avg_backward", "_check_pool"),
            tf_unpool3d: ("_MeanInterpolateFn", "_WeightedInterpolateFn", "_mean_backward", "_w_backward", "_check"),
            tf_gemm: ("_PointwiseGemmFn", "_gemm_backward")}
    for module, names in gone.items():
        for name in names:
            assert not hasattr(module, name), (module.__name__, name)
    assert hasattr(tf_pool3d, "_MaxPool3dSkipFn")                        # no dispatcher twin: stays a class of its own
