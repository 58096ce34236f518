"""Graph pooling — mirrors tf_ops/pooling/tf_pool3d.py:9-28.

Custom ops ``sph3d::max_pool3d`` (+ ``max_pool3d_grad``) and ``sph3d::avg_pool3d``
(+ ``avg_pool3d_grad``); gradients wired as the reference's RegisterGradient blocks, once for the dispatcher and the eager path
(_op.differentiable).
"""
from typing import Tuple

import torch

from . import _lib, _op, _tgraph


def _max_pool3d_impl(input: torch.Tensor, nn_index: torch.Tensor, nn_count: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _lib.require_device(input, nn_index, nn_count)
    _op.check_graph_ranks(input, nn_index, nn_count)
    input, nn_index, nn_count = _lib.f32(input), _lib.i32(nn_index), _lib.i32(nn_count)
    B, N, C = input.shape
    M, K = nn_index.shape[1], nn_index.shape[2]
    output = torch.empty((B, M, C), dtype=torch.float32, device=input.device)
    max_index = torch.empty((B, M, C), dtype=torch.int32, device=input.device)
    _lib.check(_lib.lib().sph3d_max_pool3d(B, N, M, C, K, _lib.ptr(nn_index), _lib.ptr(nn_count), _lib.ptr(input),
                                           _lib.ptr(output), _lib.ptr(max_index), _lib.stream_ptr()))
    return output, max_index


_max_pool3d = torch.library.custom_op("sph3d::max_pool3d", mutates_args=())(_max_pool3d_impl)


@_max_pool3d.register_fake
def _(input, nn_index, nn_count):
    shape = (input.shape[0], nn_index.shape[1], input.shape[2])
    return input.new_empty(shape), input.new_empty(shape, dtype=torch.int32)


def _max_pool3d_grad_impl(input: torch.Tensor, grad_output: torch.Tensor, max_index: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, grad_output, max_index)
    grad_output, max_index = _lib.f32(grad_output), _lib.i32(max_index)
    B, N, C = input.shape
    M = grad_output.shape[1]
    grad_input = torch.empty((B, N, C), dtype=torch.float32, device=input.device)
    _lib.check(_lib.lib().sph3d_max_pool3d_grad(B, N, M, C, _lib.ptr(max_index), _lib.ptr(grad_output),
                                                _lib.ptr(grad_input), _lib.stream_ptr()))
    return grad_input


_max_pool3d_grad = torch.library.custom_op("sph3d::max_pool3d_grad", mutates_args=())(_max_pool3d_grad_impl)


@_max_pool3d_grad.register_fake
def _(input, grad_output, max_index):
    return torch.empty_like(input)


def _avg_pool3d_impl(input: torch.Tensor, nn_index: torch.Tensor, nn_count: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, nn_index, nn_count)
    _op.check_graph_ranks(input, nn_index, nn_count)
    input, nn_index, nn_count = _lib.f32(input), _lib.i32(nn_index), _lib.i32(nn_count)
    B, N, C = input.shape
    M, K = nn_index.shape[1], nn_index.shape[2]
    output = torch.empty((B, M, C), dtype=torch.float32, device=input.device)
    _lib.check(_lib.lib().sph3d_avg_pool3d(B, N, M, C, K, _lib.ptr(nn_index), _lib.ptr(nn_count), _lib.ptr(input),
                                           _lib.ptr(output), _lib.stream_ptr()))
    return output


_avg_pool3d = torch.library.custom_op("sph3d::avg_pool3d", mutates_args=())(_avg_pool3d_impl)


@_avg_pool3d.register_fake
def _(input, nn_index, nn_count):
    return input.new_empty((input.shape[0], nn_index.shape[1], input.shape[2]))


def _avg_pool3d_grad_impl(input: torch.Tensor, grad_output: torch.Tensor, nn_index: torch.Tensor,
                     nn_count: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, grad_output, nn_index, nn_count)
    grad_output, nn_index, nn_count = _lib.f32(grad_output), _lib.i32(nn_index), _lib.i32(nn_count)
    B, N, C = input.shape
    M, K = nn_index.shape[1], nn_index.shape[2]
    grad_input = torch.empty((B, N, C), dtype=torch.float32, device=input.device)
    offsets, ent_key, ent_scale, _ = _tgraph.transpose(nn_index, nn_count, N)
    _lib.check(_lib.lib().sph3d_scatter_grad_t(B, N, M, C, _lib.ptr(offsets), _lib.ptr(ent_key), _lib.ptr(ent_scale),
                                               _lib.ptr(grad_output), _lib.ptr(grad_input), _lib.stream_ptr()))
    return grad_input


_avg_pool3d_grad = torch.library.custom_op("sph3d::avg_pool3d_grad", mutates_args=())(_avg_pool3d_grad_impl)


@_avg_pool3d_grad.register_fake
def _(input, grad_output, nn_index, nn_count):
    return torch.empty_like(input)


def _avg_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _avg_vjp(grad, ctx, grad_output):
    input, nn_index, nn_count = ctx.saved_tensors
    return grad(input, grad_output, nn_index, nn_count), None, None


_avg_pool3d_apply = _op.differentiable(_avg_pool3d, _avg_pool3d_impl, _avg_setup, _avg_vjp, _avg_pool3d_grad, _avg_pool3d_grad_impl)


def _max_pool3d_grad_t_impl(input, grad_output, max_index, nn_count, tg, addend=None):
    """the gradient as a gather over the transposed pooling graph tg = (offsets, ent_key, ...) (sph3d_max_pool3d_grad_t);
    addend: another gradient of `input` ([B,N,C]), added in by the same kernel"""
    grad_output, max_index = _lib.f32(grad_output), _lib.i32(max_index)
    addend = None if addend is None else _lib.f32(addend)
    B, N, C = input.shape
    M = grad_output.shape[1]
    grad_input = torch.empty((B, N, C), dtype=torch.float32, device=input.device)
    _lib.check(_lib.lib().sph3d_max_pool3d_grad_t(B, N, M, C, _lib.ptr(tg[0]), _lib.ptr(tg[1]), _lib.ptr(nn_count),
                                                  _lib.ptr(max_index), _lib.ptr(grad_output), _lib.ptr(addend), _lib.ptr(grad_input),
                                                  _lib.stream_ptr()))
    return grad_input


def _max_pool3d_grad_rows_impl(input, grad_output, max_index, nn_count, link, addend=None):
    """the same gradient without a transposed pooling graph: link = _tgraph.row_link(...) = (first, next, the transposed INTRA
    graph, its bins per source) of a pooling graph made by sph3gcn_util.gather_pooling_rows (sph3d_max_pool3d_grad_rows)"""
    first, nxt, tg, F = link
    grad_output, max_index = _lib.f32(grad_output), _lib.i32(max_index)
    addend = None if addend is None else _lib.f32(addend)
    B, N, C = input.shape
    M = grad_output.shape[1]
    grad_input = torch.empty((B, N, C), dtype=torch.float32, device=input.device)
    _lib.check(_lib.lib().sph3d_max_pool3d_grad_rows(B, N, M, C, F, _lib.ptr(tg[0]), _lib.ptr(tg[1]), _lib.ptr(first), _lib.ptr(nxt),
                                                     _lib.ptr(nn_count), _lib.ptr(max_index), _lib.ptr(grad_output), _lib.ptr(addend),
                                                     _lib.ptr(grad_input), _lib.stream_ptr()))
    return grad_input


def _gather_form(input, nn_index, nn_count):
    """how the gradient can run as a gather -> ("t", transposed pooling graph) | ("rows", row link) | None.  In this order: a
    transposed pooling graph someone built ahead of time WITH the promise that no row repeats a point; the row link of a pooling
    graph made of intra-graph rows, while the intra graph's transposed graph is cached (sph3gcn_util.gather_pooling_rows: the
    harness, on its graph stream)"""
    if not (input.is_cuda and nn_index.dtype == torch.int32 and nn_count.dtype == torch.int32):
        return None
    tg = _tgraph.peek(nn_index, nn_count, input.shape[1], need_unique_rows=True)
    if tg is not None:
        return "t", tg
    link = _tgraph.row_link(nn_index, nn_count)
    if link is None or tuple(link[0].shape) != tuple(input.shape[:2]):         # (first [B, N]: the intra graph's points are the input's)
        return None
    return "rows", link


def _no_scatter_when_deterministic():
    """deterministic mode: the max-pool gradient is the gather over a unique-rows transposed pooling graph or an error, never the
    scatter with its float atomics"""
    if _tgraph.is_deterministic():
        raise RuntimeError("max_pool3d backward: deterministic mode is on and no transposed pooling graph with unique rows is cached for "
                           "this (nn_index, nn_count); the scatter form adds with float atomics.  Build the pooling graph with "
                           "unique_rows=True (sph3gcn_util.gather_pooling_graph, or _tgraph.transpose(nn_index, nn_count, N, "
                           "unique_rows=True)) while the mode is on")


def _max_grad(scatter, input, grad_output, max_index, nn_index, nn_count, addend=None):
    """a gather, no atomics, where _gather_form finds one (rows of the ball query: no row repeats a point); otherwise `scatter`,
    the reference's form, which adds a point's gradient once however often a row lists it (tf_pool3d_gpu.cu:38-50)"""
    form = _gather_form(input, nn_index, nn_count)
    if form is not None:
        impl = _max_pool3d_grad_t_impl if form[0] == "t" else _max_pool3d_grad_rows_impl
        return impl(input, grad_output, max_index, nn_count, form[1], addend=addend)
    _no_scatter_when_deterministic()
    g = scatter(input, grad_output, max_index)
    return g if addend is None else g + addend


def _max_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output[1], inputs[1], inputs[2])
    ctx.mark_non_differentiable(output[1])


def _max_vjp(grad, ctx, grad_output, grad_index):
    input, max_index, nn_index, nn_count = ctx.saved_tensors
    return _max_grad(grad, input, grad_output, max_index, nn_index, nn_count), None, None


_max_pool3d_apply = _op.differentiable(_max_pool3d, _max_pool3d_impl, _max_setup, _max_vjp, _max_pool3d_grad, _max_pool3d_grad_impl)


def max_pool3d(input, nn_index, nn_count):
    return _max_pool3d_apply(input, nn_index, nn_count)


class _MaxPool3dSkipFn(torch.autograd.Function):
    """max_pool3d whose input is ALSO used by a skip connection: returns (pooled, max_index, input as the skip tensor); the two
    gradients of the input — through the pooling and through the skip — meet inside the pooling gradient's gather kernel
    instead of in autograd's elementwise accumulation (three tensors through memory)."""

    @staticmethod
    def forward(ctx, input, nn_index, nn_count):
        output, max_index = _max_pool3d_impl(input, nn_index, nn_count)
        ctx.save_for_backward(input, max_index, nn_index, nn_count)
        ctx.mark_non_differentiable(max_index)
        return output, max_index, input.view_as(input)

    @staticmethod
    def backward(ctx, grad_output, grad_index, grad_skip):
        input, max_index, nn_index, nn_count = ctx.saved_tensors
        if grad_output is None:
            return grad_skip, None, None
        skip = grad_skip.contiguous() if grad_skip is not None else None
        return _max_grad(_max_pool3d_grad_impl, input, grad_output, max_index, nn_index, nn_count, addend=skip), None, None


def max_pool3d_with_skip(input, nn_index, nn_count):
    """-> (pooled, max_index, skip): `skip` is `input` for whoever else consumes it (see _MaxPool3dSkipFn)"""
    return _MaxPool3dSkipFn.apply(input, nn_index, nn_count)


def max_pool3d_grad(input, grad_output, max_index):
    return _max_pool3d_grad_impl(input, grad_output, max_index)


def avg_pool3d(input, nn_index, nn_count):
    return _avg_pool3d_apply(input, nn_index, nn_count)


def avg_pool3d_grad(input, grad_output, nn_index, nn_count):
    return _avg_pool3d_grad_impl(input, grad_output, nn_index, nn_count)
